"""Test infrastructure for the bf16 precision of in-sim policy inference
(DESIGN.md §2 definition 17, include/mpenv_policy_precision.h).

* bind: the ctypes signatures of the header's functions.
* bf16_round: f32 -> bf16 -> f32, round to nearest even, as integer
  arithmetic on the bit patterns.
* pack_ref: the B-operand lane map of v_mfma_f32_32x32x16_bf16, stated in
  numpy.
* Contract: the definition restated in numpy from the f32 trunk inputs that
  policy_testlib.Ref.forward(trunk_in=True) returns: one k-ascending f32 chain
  per dense output (any order is allowed; this is one) and the LayerNorm
  statistics in float64.

Nothing here is imported by the product.
"""
import ctypes as C

import numpy as np

import policy_testlib as P

F32, BF16 = 0, 1  # MPENV_POLICY_F32, MPENV_POLICY_BF16

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
SIGNATURES = {
    "mpenv_policy_set_precision": (i32, [vp, i32]),
    "mpenv_policy_precision": (i32, [vp, C.POINTER(i32)]),
    "mpenv_debug_policy_dense_bf16": (i32, [vp, vp, i32, i32, vp, i32, vp, vp]),
    "mpenv_debug_policy_pack_bf16": (i32, [vp, i32, i32, vp, C.POINTER(i64)]),
}


def bind(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def bf16_bits(a):
    """uint16 bf16 patterns of a float32 array, round to nearest even (a NaN
    whose payload survives the shift stays that NaN)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(a):
    """float32 array -> the float32 values of its bf16 roundings"""
    a = np.ascontiguousarray(a, np.float32)
    return (bf16_bits(a).astype(np.uint32) << 16).view(np.float32).reshape(a.shape)


def pack_ref(w):
    """[K][N] float32 -> uint16 [tiles][steps][64 lanes][8]: lane l with
    r = l & 31, h = l >> 5 of k step s and column tile t holds
    w[16 s + 8 h + j][32 t + r]; K padded to 16 and N to 32 with +0"""
    K, N = w.shape
    steps, tiles = (K + 15) // 16, (N + 31) // 32
    padded = np.zeros((steps * 16, tiles * 32), np.uint16)
    padded[:K, :N] = bf16_bits(w).reshape(K, N)
    out = np.zeros((tiles, steps, 64, 8), np.uint16)
    for t in range(tiles):
        for s in range(steps):
            for l in range(64):
                r, h = l & 31, l >> 5
                out[t, s, l] = padded[16 * s + 8 * h:16 * s + 8 * h + 8, 32 * t + r]
    return out.reshape(-1)


def chain_dense(x, w):
    """[n][K] . [K][N] over the bf16 roundings: exact f32 products, one f32
    addition per k, ascending"""
    xh, wh = bf16_round(x), bf16_round(w)
    y = np.zeros((x.shape[0], w.shape[1]), np.float32)
    for k in range(x.shape[1]):
        y = y + xh[:, k, None] * wh[None, k, :]
    return y


class Contract:
    """Definition 17 over one checkpoint's tensors."""

    def __init__(self, tensors):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
        self.w = [f32(tensors[f"{P.TRUNK}Dense_{i}_kernel"]) for i in range(3)]
        self.scale = [f32(tensors[f"{P.TRUNK}LayerNorm_{i}_impl_scale"]) for i in range(3)]
        self.bias = [f32(tensors[f"{P.TRUNK}LayerNorm_{i}_impl_bias"]) for i in range(3)]
        self.head_w = np.concatenate(
            [f32(tensors[f"params_actor_DenseLayerDiscreteActor_{h}_impl_kernel"]) for h in range(2)], axis=1)
        self.head_b = np.concatenate(
            [f32(tensors[f"params_actor_DenseLayerDiscreteActor_{h}_impl_bias"]) for h in range(2)])

    def forward(self, trunk_in, dense=chain_dense):
        """[n][384] f32 trunk inputs -> [n][37] f32 logits; dense: the
        summation order (any is allowed)"""
        x = np.ascontiguousarray(trunk_in, np.float32)
        for i in range(3):
            y = dense(x, self.w[i])
            y64 = y.astype(np.float64)
            mean = y64.mean(axis=1)
            var = ((y64 - mean[:, None]) ** 2).mean(axis=1)
            mean32 = mean.astype(np.float32)
            sigma = np.sqrt(var + 1e-6).astype(np.float32)
            q = self.scale[i][None, :] / sigma[:, None]            # f32 division
            d = y - mean32[:, None]                                # f32 subtraction
            o = (q.astype(np.float64) * d.astype(np.float64) + self.bias[i][None, :].astype(np.float64))
            o = o.astype(np.float32)                               # the fma's one rounding
            x = np.where(o >= 0, o, np.float32(0) * o)
        return dense(x, self.head_w) + self.head_b[None, :]
