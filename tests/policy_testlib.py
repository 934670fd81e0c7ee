"""Test infrastructure for in-sim policy inference (DESIGN.md §2 definition 15).

* write_checkpoint: a full converted checkpoint in the reference's directory
  format (dnn.cpp:1066-1090: i32 ndim, i32 shape[ndim], f32 data; kernels
  [in][out]) drawn from numpy.random.default_rng(seed); nothing is committed.
* Ref: tests/policy_ref.cpp, the independent CPU restatement, built into a
  temporary directory and loaded with ctypes.

Nothing here is imported by the product.
"""
import atexit
import ctypes as C
import functools
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import mpenv_testlib as T

SELF_OBS, COEFS, OTHER = 43, 9, 32
SELF_IN, FWD_IN, REAR_IN = 100, 256, 64
EMBED, TRUNK_IN, HIDDEN = 64, 384, 512
BUCKETS = (3, 8, 3, 3, 13, 7)  # moveAmount, moveAngle, fire, stand, yaw, pitch
LOGITS = 37

# (file stem, length): obs_preprocess_state_<stem>_{mu,inv_sigma}, in the restatement's order
NORMS = [("self", SELF_OBS), ("reward_coefs", COEFS), ("fwd_lidar", 4), ("rear_lidar", 4),
         ("teammates", OTHER), ("opponents", OTHER), ("opponents_last_known", OTHER)]
# (file stem, LayerNorm index, inputs), in the restatement's order
EMBEDS = [("self", 2, SELF_IN), ("fwd_lidar", 0, FWD_IN), ("rear_lidar", 1, REAR_IN),
          ("teammates", 3, OTHER), ("opponents", 4, OTHER), ("opponents_last_known", 5, OTHER)]
TRUNK = "params_backbone_actor_encoder_net_MaxPoolNet_0_MLP_0_"
HEADS = [17, 20]


def checkpoint_tensors(seed):
    """{file name: float32 array}: dense N(0, 1/sqrt(K)), head kernels x 3,
    LayerNorm scale 1 + 0.1 N, biases 0.1 N, means 0.1 N, inverse sigmas in
    [0.5, 2]."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    t = {}

    def dense(K, N, gain=1.0):
        return (gain * rng.standard_normal((K, N)) / np.sqrt(K)).astype(f32)

    def layer_norm(base, n):
        t[base + "_scale"] = (1 + 0.1 * rng.standard_normal(n)).astype(f32)
        t[base + "_bias"] = (0.1 * rng.standard_normal(n)).astype(f32)

    for stem, n in NORMS:
        t[f"obs_preprocess_state_{stem}_mu"] = (0.1 * rng.standard_normal(n)).astype(f32)
        t[f"obs_preprocess_state_{stem}_inv_sigma"] = rng.uniform(0.5, 2.0, n).astype(f32)
    for stem, ln, K in EMBEDS:
        t[f"params_backbone_prefix_{stem}_embed_kernel"] = dense(K, EMBED)
        layer_norm(f"params_backbone_prefix_LayerNorm_{ln}_impl", EMBED)
    for i in range(3):
        t[f"{TRUNK}Dense_{i}_kernel"] = dense(TRUNK_IN if i == 0 else HIDDEN, HIDDEN)
        layer_norm(f"{TRUNK}LayerNorm_{i}_impl", HIDDEN)
    for h, n in enumerate(HEADS):
        t[f"params_actor_DenseLayerDiscreteActor_{h}_impl_kernel"] = dense(HIDDEN, n, 3.0)
        t[f"params_actor_DenseLayerDiscreteActor_{h}_impl_bias"] = (0.1 * rng.standard_normal(n)).astype(f32)
    return t


def write_tensor(path, arr):
    arr = np.ascontiguousarray(arr, np.float32)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", arr.ndim))
        f.write(struct.pack(f"<{arr.ndim}i", *arr.shape))
        f.write(arr.tobytes())


def write_checkpoint(dirname, seed):
    """Writes the checkpoint under dirname; returns its tensors."""
    os.makedirs(dirname, exist_ok=True)
    t = checkpoint_tensors(seed)
    for name, arr in t.items():
        write_tensor(os.path.join(dirname, name), arr)
    return t


class _Weights(C.Structure):
    _fields_ = [("normMean", C.c_void_p * 7), ("normInv", C.c_void_p * 7),
                ("embedW", C.c_void_p * 6), ("embedScale", C.c_void_p * 6), ("embedBias", C.c_void_p * 6),
                ("trunkW", C.c_void_p * 3), ("trunkScale", C.c_void_p * 3), ("trunkBias", C.c_void_p * 3),
                ("headW", C.c_void_p * 2), ("headBias", C.c_void_p * 2)]


@functools.lru_cache(maxsize=None)
def _ref_lib():
    d = tempfile.mkdtemp(prefix="policy_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libpolicy_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall",
                    "-I", os.path.join(T.PKG, "csrc"), os.path.join(T.ROOT, "tests", "policy_ref.cpp"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.policy_ref_dense.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.policy_ref_pos_embed.argtypes = [C.c_void_p, C.c_void_p]
    lib.policy_ref_gumbel.argtypes = [C.c_float]
    lib.policy_ref_gumbel.restype = C.c_float
    lib.policy_ref_sample_head.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
    lib.policy_ref_sample_head.restype = C.c_int32
    lib.policy_ref_forward.argtypes = [C.c_int] + [C.c_void_p] * 9 + [C.POINTER(_Weights), C.c_void_p, C.c_void_p]
    lib.policy_ref_sample.argtypes = [C.c_int] + [C.c_void_p] * 6
    lib.policy_ref_gumbels.argtypes = [C.c_int] + [C.c_void_p] * 4
    return lib


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


class Ref:
    """The CPU restatement over one checkpoint's tensors."""

    def __init__(self, tensors):
        self.lib = _ref_lib()
        self.t = {k: _f32(v) for k, v in tensors.items()}  # keeps the arrays alive
        w = _Weights()
        for i, (stem, _n) in enumerate(NORMS):
            w.normMean[i] = self.t[f"obs_preprocess_state_{stem}_mu"].ctypes.data
            w.normInv[i] = self.t[f"obs_preprocess_state_{stem}_inv_sigma"].ctypes.data
        for i, (stem, ln, _K) in enumerate(EMBEDS):
            w.embedW[i] = self.t[f"params_backbone_prefix_{stem}_embed_kernel"].ctypes.data
            w.embedScale[i] = self.t[f"params_backbone_prefix_LayerNorm_{ln}_impl_scale"].ctypes.data
            w.embedBias[i] = self.t[f"params_backbone_prefix_LayerNorm_{ln}_impl_bias"].ctypes.data
        for i in range(3):
            w.trunkW[i] = self.t[f"{TRUNK}Dense_{i}_kernel"].ctypes.data
            w.trunkScale[i] = self.t[f"{TRUNK}LayerNorm_{i}_impl_scale"].ctypes.data
            w.trunkBias[i] = self.t[f"{TRUNK}LayerNorm_{i}_impl_bias"].ctypes.data
        for h in range(2):
            w.headW[h] = self.t[f"params_actor_DenseLayerDiscreteActor_{h}_impl_kernel"].ctypes.data
            w.headBias[h] = self.t[f"params_actor_DenseLayerDiscreteActor_{h}_impl_bias"].ctypes.data
        self.w = w

    def forward(self, obs, trunk_in=False):
        """obs: {self, coefs, pos, fwd, rear, tm, opp, masks, lk} arrays with
        the agent in front.  Returns logits [n, 37] (and the trunk input)."""
        n = len(obs["self"])
        a = {k: _f32(v).reshape(n, -1) for k, v in obs.items()}
        assert [a[k].shape[1] for k in ("self", "coefs", "pos", "fwd", "rear", "tm", "opp", "masks", "lk")] == \
            [SELF_OBS, COEFS, 3, FWD_IN, REAR_IN, 5 * OTHER, 6 * OTHER, 6, 6 * OTHER]
        logits = np.zeros((n, LOGITS), np.float32)
        tin = np.zeros((n, TRUNK_IN), np.float32) if trunk_in else None
        self.lib.policy_ref_forward(n, *(a[k].ctypes.data for k in ("self", "coefs", "pos", "fwd", "rear", "tm",
                                                                   "opp", "masks", "lk")),
                                    C.byref(self.w), logits.ctypes.data, tin.ctypes.data if trunk_in else None)
        return (logits, tin) if trunk_in else logits

    def sample(self, logits, rng_a, rng_b, rng_ctr):
        """actions [n, 6] and the advanced counters."""
        n = len(logits)
        lg = _f32(logits)
        ra, rb, rc = (np.ascontiguousarray(x, np.int32) for x in (rng_a, rng_b, rng_ctr))
        acts = np.zeros((n, 6), np.int32)
        ctr = np.zeros(n, np.int32)
        self.lib.policy_ref_sample(n, lg.ctypes.data, ra.ctypes.data, rb.ctypes.data, rc.ctypes.data,
                                   acts.ctypes.data, ctr.ctypes.data)
        return acts, ctr


def ref_gumbels(rng_a, rng_b, rng_ctr):
    """[n, 37] the noise Ref.sample adds to each logit."""
    ra, rb, rc = (np.ascontiguousarray(x, np.int32) for x in (rng_a, rng_b, rng_ctr))
    g = np.zeros((len(ra), LOGITS), np.float32)
    _ref_lib().policy_ref_gumbels(len(ra), ra.ctypes.data, rb.ctypes.data, rc.ctypes.data, g.ctypes.data)
    return g


def ref_dense(x, w):
    x, w = _f32(x), _f32(w)
    y = np.zeros((x.shape[0], w.shape[1]), np.float32)
    _ref_lib().policy_ref_dense(x.ctypes.data, x.shape[0], x.shape[1], w.ctypes.data, w.shape[1], y.ctypes.data)
    return y


def ref_pos_embed(pos3):
    p = _f32(pos3)
    out = np.zeros(48, np.float32)
    _ref_lib().policy_ref_pos_embed(p.ctypes.data, out.ctypes.data)
    return out


def ref_gumbel(u):
    return np.float32(_ref_lib().policy_ref_gumbel(np.float32(u)))


def ref_sample_head(logits, key_a, key_b):
    lg = _f32(logits)
    return int(_ref_lib().policy_ref_sample_head(lg.ctypes.data, len(lg), key_a, key_b))


# the engine exports the network reads, under the restatement's names
ENGINE_INPUTS = {"self": "SELF_OBSERVATION", "coefs": "REWARD_HYPER_PARAMS", "pos": "SELF_POSITION",
                 "fwd": "FWD_LIDAR", "rear": "REAR_LIDAR", "tm": "TEAMMATE_OBSERVATIONS",
                 "opp": "OPPONENT_OBSERVATIONS", "masks": "OPPONENT_MASKS",
                 "lk": "OPPONENT_LAST_KNOWN_OBSERVATIONS"}


def engine_obs(engine):
    return {k: engine.get(name) for k, name in ENGINE_INPUTS.items()}


def policy_check(dirname):
    """(return code, message) of mpenv_policy_check."""
    lib = T.lib_mpenv()
    rc = lib.mpenv_policy_check(os.fsencode(str(dirname)))
    return rc, (lib.mpenv_last_error().decode() if rc else "")
