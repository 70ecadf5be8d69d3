"""numpy restatement of adaptive sampling (rt3_render_path_adaptive) over the CPU oracle.

Test infrastructure only.  The samples come from oracle_lib.render_path_range with FLAG_VARIANCE (sums and squares in sample order); this module
restates what is new: the convergence rule in float32 with every operation rounded on its own, the 3 x 3 dilation over the shard's own pixels in
FRAME rows, the active set that only shrinks, and sums that freeze when a pixel leaves.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

F = np.float32


def unconverged(acc, sq, n, threshold, dark):
    """The rule for every pixel: acc / sq float32 [rows, w, 4] sums and sums of squares, n the (uint32 [rows, w]) samples behind them."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = n.astype(F)
        m = acc[..., :3] / nf[..., None]
        v = sq[..., :3] / nf[..., None] - m * m
        v = np.where(v > 0, v, F(0))
        e2 = ((v[..., 0] + v[..., 1]) + v[..., 2]) / nf
        d = ((m[..., 0] + m[..., 1]) + m[..., 2]) + F(dark)
        lim = F(threshold) * d
        assert e2.dtype == F and lim.dtype == F
        return e2 > lim * lim


def frame_rows(params):
    """Frame row of every local row of the shard params describes."""
    rows = O.lib().oracle_rows_owned(C.byref(params))
    if params.tile_count <= 1:
        return np.arange(rows)
    l = np.arange(rows)
    return ((l // params.tile_rows) * params.tile_count + params.tile_index) * params.tile_rows + l % params.tile_rows


def dilate(u, rows_in_frame):
    """any(u) over the owned pixels q with |x_q - x_p| <= 1 and |framerow_q - framerow_p| <= 1."""
    rows, w = u.shape
    h = u.copy()
    h[:, 1:] |= u[:, :-1]
    h[:, :-1] |= u[:, 1:]
    out = h.copy()
    for l in range(rows):
        for dl in (-1, 1):
            lq = l + dl
            if 0 <= lq < rows and rows_in_frame[lq] == rows_in_frame[l] + dl:
                out[l] |= h[lq]
    return out


def render_adaptive(cam, params, threshold, min_spp, step_spp, dark, **scene):
    """-> dict(counts, active_counts, levels): counts uint32 [rows, w]; active_counts the number of active pixels per round; levels maps every
    sample count n a round ended at to the oracle's (frame, acc, sq) over samples [0, n) of params.spp.  params.flags must hold FLAG_VARIANCE."""
    assert params.flags & O.FLAG_VARIANCE and 2 <= min_spp <= params.spp and step_spp >= 1
    fr = frame_rows(params)
    img, acc, sq, _ = O.render_path_range(cam, params, 0, min_spp, **scene)
    counts = np.full(img.shape, min_spp, np.uint32)
    active = np.ones(img.shape, bool)
    f_acc, f_sq = acc.copy(), sq.copy()                                # the adaptive accumulation: frozen where a pixel left
    levels = {min_spp: (img.copy(), acc.copy(), sq.copy())}
    active_counts = [int(active.sum())]
    done = min_spp
    while done < params.spp:
        active &= dilate(unconverged(f_acc, f_sq, counts, threshold, dark), fr)
        if not active.any():
            break
        ns = min(step_spp, params.spp - done)
        img, acc, sq, _ = O.render_path_range(cam, params, done, ns, acc, sq, **scene)
        done += ns
        levels[done] = (img.copy(), acc.copy(), sq.copy())
        f_acc[active] = acc[active]
        f_sq[active] = sq[active]
        counts[active] = done
        active_counts.append(int(active.sum()))
    return dict(counts=counts, active_counts=active_counts, levels=levels, acc=f_acc, sq=f_sq)


def expected_frame(ref):
    """The frame an adaptive render must return: every pixel from the oracle's frame of its own level."""
    out = np.zeros(ref["counts"].shape, np.uint32)
    for n, (img, _, _) in ref["levels"].items():
        out[ref["counts"] == n] = img[ref["counts"] == n]
    return out


def expected_resolve(ref):
    """rt3_accum_resolve after an adaptive render: (sum / n, 0) per pixel, n its own count."""
    out = np.zeros(ref["acc"].shape, np.float32)
    out[..., :3] = ref["acc"][..., :3] / ref["counts"].astype(F)[..., None]
    return out
