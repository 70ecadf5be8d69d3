"""Batched ray queries (rt3_intersect / rt3_occluded) without a GPU: the wire structs, the Python packing helper, and the
"no device" behaviour every device entry point shares."""
import ctypes as C

import numpy as np
import pytest


def test_query_structs_sizes_and_offsets(rt3):
    assert C.sizeof(rt3.rt3_ray) == 32 and rt3.RAY.itemsize == 32
    assert C.sizeof(rt3.rt3_hit) == 16 and rt3.HIT.itemsize == 16
    assert [getattr(rt3.rt3_ray, f).offset for f in ("origin", "t_max", "direction", "_pad")] == [0, 12, 16, 28]
    assert [rt3.RAY.fields[f][1] for f in ("origin", "t_max", "direction", "_pad")] == [0, 12, 16, 28]
    assert [getattr(rt3.rt3_hit, f).offset for f in ("t", "kind", "index", "_pad")] == [0, 4, 8, 12]
    assert [rt3.HIT.fields[f][1] for f in ("t", "kind", "index", "_pad")] == [0, 4, 8, 12]
    assert (rt3.HIT_NONE, rt3.HIT_FACE, rt3.HIT_SPHERE, rt3.HIT_INVALID) == (0, 1, 2, 3)


def test_header_declares_the_query_abi(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    for s in ("rt3_intersect", "rt3_occluded", "rt3_intersect_device", "rt3_occluded_device"):
        assert s in names and s in rt3.EXPORTS
    L = rt3.lib()
    assert all(hasattr(L, s) for s in ("rt3_intersect", "rt3_occluded", "rt3_intersect_device", "rt3_occluded_device"))
    assert L.rt3_abi_version() == 3                                   # additions only: every existing struct is unchanged


def test_make_rays_normalises_and_packs(rt3):
    rng = np.random.default_rng(5)
    o = rng.normal(0.0, 10.0, (1000, 3)).astype(np.float32)
    d = (rng.normal(0.0, 1.0, (1000, 3)) * rng.uniform(1e-3, 1e3, (1000, 1))).astype(np.float32)
    t_max = rng.uniform(0.0, 50.0, 1000).astype(np.float32)
    rays = rt3.make_rays(o, d, t_max)
    assert rays.dtype == rt3.RAY and rays.shape == (1000,)
    assert np.array_equal(rays["origin"], o) and np.array_equal(rays["t_max"], t_max) and (rays["_pad"] == 0).all()
    u = rays["direction"]
    # the validity rule of the kernels: |fma(dz, dz, fma(dy, dy, dx * dx)) - 1| <= 2^-20, in float32 (float64 products of float32 values
    # are exact, so this bounds the fused chain too)
    dd = (u.astype(np.float64) ** 2).sum(axis=1)
    assert np.abs(dd - 1.0).max() <= 2.0 ** -21
    cosang = (u.astype(np.float64) * d).sum(axis=1) / np.linalg.norm(d.astype(np.float64), axis=1)
    assert (cosang > 1.0 - 1e-6).all()                                # same direction
    assert np.isinf(rt3.make_rays(o[:3], d[:3])["t_max"]).all()       # default: no limit
    # (N, 8) float32 view: origin, t_max, direction, pad
    flat = rays.view(np.float32).reshape(-1, 8)
    assert np.array_equal(flat[:, :3], o) and np.array_equal(flat[:, 3], t_max) and np.array_equal(flat[:, 4:7], u)
    # a zero direction cannot be normalised: it stays non-finite, which the kernels reject as invalid
    z = rt3.make_rays([[0, 0, 0]], [[0, 0, 0]])
    assert not np.isfinite(z["direction"]).all()


def test_queries_fail_like_every_device_call_without_a_gpu(rt3):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(rt3.Fatal, match="no CPU fallback"):
        rt3.initialize_renderer(0)
    L = rt3.lib()
    rays = rt3.make_rays([[0, 0, 0]], [[0, 0, -1]])
    hits = np.zeros(1, rt3.HIT)
    occ = np.zeros(1, np.uint32)
    # no context can exist: every entry point refuses a NULL one with RT3_E_ARG, as the other device calls do
    assert L.rt3_intersect(None, rays.ctypes.data_as(C.c_void_p), 1, np.float32(0.001), hits.ctypes.data_as(C.c_void_p)) == -1
    assert L.rt3_occluded(None, rays.ctypes.data_as(C.c_void_p), 1, np.float32(0.001), occ.ctypes.data_as(C.c_void_p)) == -1
    assert L.rt3_intersect_device(None, None, 1, np.float32(0.001), None, None) == -1
    assert L.rt3_occluded_device(None, None, 1, np.float32(0.001), None, None) == -1
