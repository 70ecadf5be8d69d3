"""The counter-hash table k_trace_mfma32's render form keeps in LDS (rt3_kernel_common.hpp): row d, word k is hash_u32(1 + 8 (d + 1) + k),
the inner hash of rnd(base, ctr + k) for a path of depth d.  rt3_debug_ctr_table computes it on the host with the function the kernel's prologue
fills the table with; here it is compared with the oracle's hash and with a numpy statement of random_v1.glsl's hash, for every depth below the cap."""
import numpy as np


def hash_u32(x):
    x = np.asarray(x, np.uint32).copy()
    x += x << np.uint32(10); x ^= x >> np.uint32(6); x += x << np.uint32(3); x ^= x >> np.uint32(11); x += x << np.uint32(15)
    return x


def test_every_row_holds_the_hashes_of_its_depths_counters(rt3, oracle):
    tab = rt3.debug_ctr_table()
    cap = rt3.lib().rt3_debug_ctr_table(None, 0)
    assert tab.dtype == np.uint32 and tab.shape == (cap, 4) and cap >= 50           # (the bench frame's max_depth is 50)
    d, k = np.meshgrid(np.arange(cap, dtype=np.uint32), np.arange(4, dtype=np.uint32), indexing="ij")
    ctr = np.uint32(1) + np.uint32(8) * (d + np.uint32(1)) + k
    assert np.array_equal(tab, hash_u32(ctr))
    H = oracle.lib().oracle_hash_u32
    assert all(int(tab[i, j]) == H(int(ctr[i, j])) for i in range(cap) for j in range(4))
    assert all(int(tab[i, j]) == rt3.lib().rt3_hash_u32(int(ctr[i, j])) for i in range(cap) for j in range(4))


def test_a_short_buffer_gets_only_its_rows(rt3):
    out = np.full((5, 4), 0xDEADBEEF, np.uint32)
    cap = rt3.lib().rt3_debug_ctr_table(out.ctypes.data, 3)
    assert cap == len(rt3.debug_ctr_table())
    assert np.array_equal(out[:3], rt3.debug_ctr_table()[:3]) and (out[3:] == 0xDEADBEEF).all()
