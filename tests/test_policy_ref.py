"""tests/policy_ref.cpp is the right network, not just self-consistent: an
independent torch model written here (matmul, two-pass LayerNorm) in float64
is the yardstick, and the same model in float32 gives the size of an f32
evaluation's error.  No GPU."""
import math

import numpy as np
import pytest
import torch

import policy_testlib as P

N = 2000
SEED = 5


def torch_model(t, obs, dtype):
    """logits [n, 37] of the architecture of DESIGN.md §2 definition 15."""
    w = {k: torch.from_numpy(v).to(dtype) for k, v in t.items()}
    o = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dtype) for k, v in obs.items()}
    n = o["self"].shape[0]

    def norm(x, stem):
        return w[f"obs_preprocess_state_{stem}_inv_sigma"] * (x - w[f"obs_preprocess_state_{stem}_mu"])

    def block(x, kernel, ln, slope):
        y = x @ w[kernel]
        mean = y.mean(-1, keepdim=True)
        var = ((y - mean) ** 2).mean(-1, keepdim=True)
        y = (y - mean) / torch.sqrt(var + 1e-6) * w[ln + "_scale"] + w[ln + "_bias"]
        return torch.where(y >= 0, y, slope * y)

    def embed(x, stem, ln):
        return block(x, f"params_backbone_prefix_{stem}_embed_kernel", f"params_backbone_prefix_LayerNorm_{ln}_impl",
                     0.01)

    pos = o["pos"].reshape(n, 3)
    rows = []
    for i in range(8):
        scaled = pos * float(1 << i) * torch.tensor(math.pi, dtype=dtype)
        rows += [torch.sin(scaled), torch.cos(scaled)]
    self_in = torch.cat([norm(o["self"].reshape(n, 43), "self"), norm(o["coefs"].reshape(n, 9), "reward_coefs")]
                        + rows, dim=1)
    parts = [embed(self_in, "self", 2),
             embed(norm(o["fwd"].reshape(n, 64, 4), "fwd_lidar").reshape(n, 256), "fwd_lidar", 0),
             embed(norm(o["rear"].reshape(n, 16, 4), "rear_lidar").reshape(n, 64), "rear_lidar", 1),
             embed(norm(o["tm"].reshape(n, 5, 32), "teammates"), "teammates", 3).max(dim=1).values,
             (embed(norm(o["opp"].reshape(n, 6, 32), "opponents"), "opponents", 4)
              * o["masks"].reshape(n, 6, 1)).max(dim=1).values,
             embed(norm(o["lk"].reshape(n, 6, 32), "opponents_last_known"), "opponents_last_known", 5).max(dim=1).values]
    h = torch.cat(parts, dim=1)
    for i in range(3):
        h = block(h, f"{P.TRUNK}Dense_{i}_kernel", f"{P.TRUNK}LayerNorm_{i}_impl", 0.0)
    heads = [h @ w[f"params_actor_DenseLayerDiscreteActor_{k}_impl_kernel"]
             + w[f"params_actor_DenseLayerDiscreteActor_{k}_impl_bias"] for k in range(2)]
    return torch.cat(heads, dim=1).numpy()


def random_obs(n, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return {"self": f(n, 43), "coefs": rng.uniform(0, 1, (n, 9)).astype(np.float32),
            "pos": rng.uniform(-1, 1, (n, 3)).astype(np.float32), "fwd": f(n, 256), "rear": f(n, 64),
            "tm": f(n, 160), "opp": f(n, 192), "masks": (rng.uniform(0, 1, (n, 6)) < 0.5).astype(np.float32),
            "lk": f(n, 192)}


@pytest.fixture(scope="module")
def case():
    t = P.checkpoint_tensors(SEED)
    obs = random_obs(N, SEED + 1)
    ref = P.Ref(t)
    logits, trunk_in = ref.forward(obs, trunk_in=True)
    torch.manual_seed(0)
    f64 = torch_model(t, obs, torch.float64)
    f32 = torch_model(t, obs, torch.float32)
    return dict(ref=ref, logits=logits, trunk_in=trunk_in, f64=f64, e32=float(np.abs(f32 - f64).max()))


def test_logits_match_the_float64_model_within_an_f32_evaluations_error(case):
    err = float(np.abs(case["logits"].astype(np.float64) - case["f64"]).max())
    print(f"e32 = {case['e32']:.3e}, restatement error = {err:.3e}, logit std = {case['f64'].std():.3f}")
    assert np.isfinite(case["logits"]).all() and np.isfinite(case["trunk_in"]).all()
    assert 0 < case["e32"] < 1e-4  # the f32 model itself is sane
    assert err <= 4 * case["e32"]


def test_sampled_actions_match_those_of_the_float64_logits(case):
    rng = np.random.default_rng(SEED + 2)
    ra, rb = (rng.integers(-2**31, 2**31, N).astype(np.int32) for _ in range(2))
    rc = rng.integers(0, 1000, N).astype(np.int32)
    acts, ctr = case["ref"].sample(case["logits"], ra, rb, rc)
    assert np.array_equal(ctr, rc + 6)
    score = case["f64"] + P.ref_gumbels(ra, rb, rc).astype(np.float64)
    at, excluded, heads = 0, 0, 0
    for h, nb in enumerate(P.BUCKETS):
        s = score[:, at:at + nb]
        top = np.sort(s, axis=1)
        close = (top[:, -1] - top[:, -2]) < 8 * case["e32"]
        want = np.argmax(s, axis=1)
        assert np.array_equal(acts[~close, h], want[~close]), h
        assert (acts[:, h] >= 0).all() and (acts[:, h] < nb).all()
        excluded += int(close.sum())
        heads += N
        at += nb
    print(f"{excluded} of {heads} heads inside the gap")
    assert excluded <= heads // 100


def test_position_embedding_puts_sin_rows_before_cos_rows():
    e = P.ref_pos_embed([0.5, 0.25, 0.0])
    r = math.sqrt(0.5)
    # frequency 0: sin(x pi), sin(y pi), sin(z pi), then the cosines
    assert np.allclose(e[0:6], [1, r, 0, 0, r, 1], atol=1e-6) and e[2] == 0 and e[5] == 1
    # frequency 1: sin(2 x pi) = 0, sin(2 y pi) = 1; cos(2 x pi) = -1, cos(2 y pi) = 0
    assert np.allclose(e[6:12], [0, 1, 0, -1, 0, 1], atol=1e-6)
    # frequency 7 of x = 1/256: sin(pi / 2) = 1
    assert abs(P.ref_pos_embed([1 / 256, 0, 0])[42] - 1) < 1e-6


def test_zero_uniform_gives_minus_infinity_and_bucket_zero_wins_by_default():
    assert P.ref_gumbel(0.0) == -np.inf  # logf_(0) = -inf, so g = -(logf_(+inf)) = -inf
    assert np.isfinite(P.ref_gumbel(0.5)) and abs(float(P.ref_gumbel(0.5)) + math.log(math.log(2))) < 1e-6
    none = np.full(8, -np.inf, np.float32)
    assert P.ref_sample_head(none, 1, 2) == 0  # nothing beats -inf
    one = none.copy()
    one[5] = 0.0
    assert P.ref_sample_head(one, 1, 2) == 5


def test_dense_is_the_k_ascending_fma_chain():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 7)).astype(np.float32)
    w = rng.standard_normal((7, 5)).astype(np.float32)
    want = np.zeros((3, 5), np.float32)
    for m in range(3):
        for n in range(5):
            y = np.float64(0)
            for k in range(7):  # one rounding per step: the f64 sum of an f32 product and an f32 is exact enough
                y = np.float64(np.float32(np.float64(w[k, n]) * np.float64(x[m, k]) + y))
            want[m, n] = y
    assert np.array_equal(P.ref_dense(x, w), want)
