"""The bf16 precision of in-sim policy inference without a GPU (DESIGN.md §2
definition 17): the host's bf16 B-operand packing against the lane map stated
in numpy, and the numpy restatement of the definition against the f32
restatement of definition 15."""
import ctypes as C

import numpy as np
import pytest

import mpenv_testlib as T
import policy_bf16_testlib as B
import policy_testlib as P

CKPT_SEED = 21


def u32_as_f32(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


# round-to-nearest-even cases: a tie under an even and under an odd bf16, one ulp(f32) to either side of
# a tie, both zeros, the largest finite f32 (rounds to inf), a NaN
EDGES = u32_as_f32(0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f808001, 0x3f807fff, 0x3f818001, 0x3f817fff,
                   0x00000000, 0x80000000, 0x7f7fffff, 0xff7fffff, 0x7fc00000)


def test_bf16_round_is_round_to_nearest_even():
    got = B.bf16_round(EDGES).view(np.uint32)
    want = np.array([0x3f800000, 0x3f820000, 0xbf800000, 0xbf820000, 0x3f810000, 0x3f800000, 0x3f820000, 0x3f810000,
                     0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000], np.uint32)
    assert (got == want).all(), [hex(x) for x in got]


@pytest.mark.parametrize("K,N", [(16, 32), (100, 37), (384, 512), (512, 64)])
def test_pack_bf16_puts_every_element_at_its_lane(K, N):
    """mpenv_debug_policy_pack_bf16: every element at the place the lane map
    names, each bf16_round(w) bit for bit, the padding +0."""
    lib = B.bind(T.lib_mpenv())
    rng = np.random.default_rng(K * 1000 + N)
    w = rng.standard_normal((K, N)).astype(np.float32)
    flat = w.reshape(-1)
    flat[rng.choice(flat.size, len(EDGES), replace=False)] = EDGES
    want = B.pack_ref(w)
    count = C.c_int64(-1)
    assert lib.mpenv_debug_policy_pack_bf16(w.ctypes.data, K, N, None, C.byref(count)) == 0
    assert count.value == want.size == ((N + 31) // 32) * ((K + 15) // 16) * 512
    got = np.full(count.value + 8, 0xabcd, np.uint16)
    count.value = -1
    assert lib.mpenv_debug_policy_pack_bf16(w.ctypes.data, K, N, got.ctypes.data, C.byref(count)) == 0
    assert count.value == want.size and (got[want.size:] == 0xabcd).all()  # nothing past the count
    got = got[:want.size]
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    # the map, once more from the other side: where each w[k][n] went, and that the rest is +0
    steps = (K + 15) // 16
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    t, r, s, h, j = n // 32, n % 32, k // 16, (k % 16) // 8, k % 8
    at = (((t * steps + s) * 64 + 32 * h + r) * 8 + j).reshape(-1)
    assert len(np.unique(at)) == K * N
    assert (got[at] == B.bf16_bits(w).reshape(-1)).all()
    rest = np.ones(got.size, bool)
    rest[at] = False
    assert (got[rest] == 0).all()


def test_pack_bf16_refuses_bad_arguments():
    lib = B.bind(T.lib_mpenv())
    w = np.zeros((4, 4), np.float32)
    count = C.c_int64(0)
    assert lib.mpenv_debug_policy_pack_bf16(None, 4, 4, None, C.byref(count)) == -1
    assert lib.mpenv_debug_policy_pack_bf16(w.ctypes.data, 4, 4, None, None) == -1
    assert lib.mpenv_debug_policy_pack_bf16(w.ctypes.data, 0, 4, None, C.byref(count)) == -1
    assert lib.mpenv_policy_set_precision(None, B.BF16) == -1
    assert lib.mpenv_policy_precision(None, None) == -1


def random_obs(n, seed):
    """observations of the shapes Ref.forward takes: unit normals, masks 0 / 1"""
    rng = np.random.default_rng(seed)
    dims = {"self": P.SELF_OBS, "coefs": P.COEFS, "pos": 3, "fwd": P.FWD_IN, "rear": P.REAR_IN, "tm": 5 * P.OTHER,
            "opp": 6 * P.OTHER, "lk": 6 * P.OTHER}
    obs = {k: rng.standard_normal((n, d)).astype(np.float32) for k, d in dims.items()}
    obs["masks"] = rng.integers(0, 2, (n, 6)).astype(np.float32)
    return obs


def test_contract_stays_close_to_f32_and_differs_from_it():
    """The numpy restatement of definition 17 on random trunk inputs against
    definition 15: bf16 moves every logit a little and none by much (the
    logits' standard deviation is about 2)."""
    tensors = P.checkpoint_tensors(CKPT_SEED)
    a, tin = P.Ref(tensors).forward(random_obs(48, 5), trunk_in=True)
    b = B.Contract(tensors).forward(tin)
    delta = np.abs(b.astype(np.float64) - a)
    print(f"mean |dlogit| {delta.mean():.4g}, max {delta.max():.4g}, logit sd {a.std():.3g}")
    assert 0 < delta.mean() and delta.max() < 0.25
