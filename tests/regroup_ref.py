"""The group order rt3_regroup builds, restated in numpy: median_split_order's rule with a stable full sort per part.

Start from the region's primitive ids in ascending order; every part larger than `group` is stable-sorted by its centres' f32 coordinate
along the longest axis of their box (first maximum of hi - lo in f32; -0 and +0 equal; ties keep their order) and cut after `half`
entries; parts of at most `group` entries keep the order their parent's sort left them in."""
import numpy as np

GROUP, SUPER = 8, 8
PAD = 0xFFFFFFFF


def split_half(count, group=GROUP, sup=SUPER):
    """The host's cut (median_split_order): the left part is a multiple of `unit`; count > group."""
    unit = group * sup if count > group * sup else group
    half = (count // 2 + unit - 1) // unit * unit
    if half >= count:
        half = count - unit
    return half


def parts_of(count, group=GROUP, sup=SUPER):
    """Every part (begin, end) the split visits, parents before children: they depend on the count alone."""
    out, stack = [], [(0, count)]
    while stack:
        b, e = stack.pop()
        out.append((b, e))
        if e - b > group:
            h = split_half(e - b, group, sup)
            stack.append((b + h, e))
            stack.append((b, b + h))
    return out


def split_axis(c):
    """Longest extent of the centres' box, the first maximum winning, computed in f32 as hi - lo."""
    ext = (c.max(axis=0) - c.min(axis=0)).astype(np.float32)
    axis = 0
    for a in (1, 2):
        if ext[a] > ext[axis]:
            axis = a
    return axis


def regroup_order(ids, centres, group=GROUP, sup=SUPER):
    """ids: the region's primitive ids (any order; sorted here); centres: (n_primitives, 3) float32, indexed by primitive id, unusable
    records already replaced by the class's filter centre.  Returns the ids in the specified order."""
    ids = np.sort(np.asarray(ids, np.uint32))
    centres = np.asarray(centres, np.float32)
    stack = [(0, len(ids))]
    while stack:
        b, e = stack.pop()
        if e - b <= group:
            continue
        c = centres[ids[b:e]]
        key = c[:, split_axis(c)] + np.float32(0.0)                   # (-0 + 0 = +0: the two zeros are one key)
        ids[b:e] = ids[b:e][np.argsort(key, kind="stable")]
        h = split_half(e - b, group, sup)
        stack.append((b + h, e))
        stack.append((b, b + h))
    return ids


def padded(order, group=GROUP, sup=SUPER):
    """The order as the device keeps it: padded with 0xFFFFFFFF to whole rows of group x sup positions."""
    n = (len(order) + group * sup - 1) // (group * sup) * (group * sup)
    out = np.full(n, PAD, np.uint32)
    out[:len(order)] = order
    return out


def sphere_centres(center_radius, filter_centre=(0.0, 0.0, 0.0)):
    """The coordinates spheres are sorted by: the centre of (cx, cy, cz, r), the filter centre where the record is not usable."""
    cr = np.asarray(center_radius, np.float32).reshape(-1, 4)
    with np.errstate(over="ignore", invalid="ignore"):
        good = (cr[:, 3] > 0) & np.isfinite(cr).all(axis=1) & np.isfinite(cr[:, 3] * cr[:, 3])
    c = cr[:, :3].copy()
    c[~good] = np.asarray(filter_centre, np.float32)
    return c


def mesh_filter_centre(verts):
    """The centre the faces' filter coordinates are taken about: the middle of the box of the finite vertex coordinates AT COMMIT TIME
    (box_centre: in double, rounded to f32; 0 on an axis without a finite coordinate)."""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3]
    out = np.zeros(3, np.float32)
    for a in range(3):
        c = v[:, a][np.isfinite(v[:, a])]
        if len(c):
            m = np.float32(0.5 * (np.float64(c.min()) + np.float64(c.max())))
            out[a] = m if np.isfinite(m) else np.float32(0.0)
    return out


def face_centres(faces, verts, filter_centre=(0.0, 0.0, 0.0)):
    """The coordinates faces are sorted by: the centre of the bound as k_commit_mesh stores it (the centroid in double, rounded to f32);
    the filter centre for a face whose bound is not usable: a non-finite centre, or no bounded hit region (coincident or collinear
    vertices: the cross product of the edges, in double, is exactly zero)."""
    v = np.asarray(verts, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    p1, p2, p3 = v[faces["v1"]], v[faces["v2"]], v[faces["v3"]]
    with np.errstate(invalid="ignore", over="ignore"):
        c = ((p1 + p2 + p3) / 3.0).astype(np.float32)
        degenerate = (np.cross(p2 - p1, p3 - p1) == 0.0).all(axis=1)
    c[degenerate | ~np.isfinite(c).all(axis=1)] = np.asarray(filter_centre, np.float32)
    return c


def leaf_sets(order, group=GROUP):
    """The set of primitive ids in every leaf group of `group` positions (pads dropped)."""
    order = np.asarray(order, np.uint32).reshape(-1, group)
    return [frozenset(int(i) for i in row if i != PAD) for row in order]
