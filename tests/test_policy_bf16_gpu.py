"""The bf16 precision of in-sim policy inference on the GPU (csrc/policy.hip
k_pol_trunk_bf16, include/mpenv_policy_precision.h) against DESIGN.md §2
definition 17: the dense code exactly where the definition makes it exact and
within the derived bound elsewhere, the logits against the numpy restatement,
and sampling, the step, the slots and the surface as in f32.

Shapes as in test_policy_gpu.py: 6 agents (a partial tile), 42, 130 (more than
two tiles) and 6v6 in three world groups."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mpenv_testlib as T
import policy_bf16_testlib as B
import policy_slots_abi
import policy_testlib as P

pytestmark = pytest.mark.gpu

SEED = 1234
CKPT_SEED = 21
SHAPES = [(1, 3, 1), (3, 7, 1), (5, 13, 1), (6, 7, 3)]
NAMES = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS
ERR_INVALID = -1


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """{seed: (directory, P.Ref, B.Contract)} for the checkpoints of seeds 21 and 22"""
    root = tmp_path_factory.mktemp("policy_bf16")
    out = {}
    for seed in (CKPT_SEED, CKPT_SEED + 1):
        d = root / f"ckpt{seed}"
        tensors = P.write_checkpoint(d, seed)
        out[seed] = (str(d), P.Ref(tensors), B.Contract(tensors))
    return out


def engine(ts, W, groups=1, **kw):
    e = T.Engine(W, ts, **kw)
    B.bind(e.lib)
    policy_slots_abi.bind(e.lib)
    if groups > 1:
        e.set_world_groups(groups)
    e.put_ctrl([0, 1, 1])
    e.init()
    return e


def ok(e, rc):
    assert rc == 0, e.lib.mpenv_last_error().decode()


def set_precision(e, p):
    ok(e, e.lib.mpenv_policy_set_precision(e.h, p))


def precision(e):
    p = C.c_int32(-1)
    ok(e, e.lib.mpenv_policy_precision(e.h, C.byref(p)))
    return p.value


def outputs(e):
    return {n: e.get(n) for n in NAMES}


def compare_all(got, want, where):
    for n in NAMES:
        T.compare(got[n], want[n], f"{n} @ {where}")


def rng_of(e):
    ai = e.get("DEBUG_AGENT_I32")
    return ai[:, 3].copy(), ai[:, 4].copy(), ai[:, 5].copy()


def actions_of(e):
    return np.concatenate([e.get("PVP_DISCRETE_ACTION"), e.get("PVP_DISCRETE_AIM_ACTION")], axis=1)


def mixed_ids(A):
    """policy ids per agent: >= 0 (evaluated), -1 (A* bot), -2 (left alone); period 7, so every world differs"""
    return np.resize(np.array([0, -1, -2, 3, 1, 0, -2], np.int32), A)


def forward(e, slot=0):
    """(logits [A][37], actions [A][6]) of mpenv_policy_forward_slot at the manager's precision"""
    A = e.W * e.N
    lg_d = e.mem.upload(np.full((A, P.LOGITS), np.nan, np.float32))
    ac_d = e.mem.upload(np.full((A, 6), -7, np.int32))
    ok(e, e.lib.mpenv_policy_forward_slot(e.h, slot, lg_d, ac_d, None))
    e.mem.hip.hipDeviceSynchronize()
    logits, acts = np.empty((A, P.LOGITS), np.float32), np.empty((A, 6), np.int32)
    e.mem.d2h(lg_d, logits.nbytes, logits)
    e.mem.d2h(ac_d, acts.nbytes, acts)
    e.mem.free(lg_d)
    e.mem.free(ac_d)
    return logits, acts


# ---------------------------------------------------------------- dense

@functools.lru_cache(maxsize=None)
def dense_engine():
    return engine(1, 1)


def dense_bf16(x, w):
    e = dense_engine()
    x, w = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32)
    (M, K), N = x.shape, w.shape[1]
    xd = e.mem.upload(x)
    yd = e.mem.upload(np.full((M, N), np.nan, np.float32))
    ok(e, e.lib.mpenv_debug_policy_dense_bf16(e.h, xd, M, K, w.ctypes.data, N, yd, None))
    got = np.empty((M, N), np.float32)
    e.mem.d2h(yd, got.nbytes, got)
    e.mem.free(xd)
    e.mem.free(yd)
    return got


@pytest.mark.parametrize("K", [1, 15, 16, 17, 100, 384, 512])
def test_dense_of_small_integers_is_exact(K):
    """Integers in [-8, 8] are bf16 values and every partial sum is an integer
    below 2^24 in any order: the result is the integer product bit for bit,
    whatever order the hardware adds in (a wrong lane, a missed k range or a
    padding that is not zero shows)."""
    rng = np.random.default_rng(K)
    for N in (17, 64, 512):
        w = rng.integers(-8, 9, (K, N)).astype(np.float32)
        for M in (1, 63, 65, 130):
            x = rng.integers(-8, 9, (M, K)).astype(np.float32)
            want = (x.astype(np.int64) @ w.astype(np.int64)).astype(np.float32)
            T.compare(dense_bf16(x, w), want, f"integer dense M={M} K={K} N={N}")


def test_dense_rounds_its_input_to_nearest_even():
    """One 1.0 per column of w: the output is the rounded input itself.  x
    lies exactly on bf16 ties (under even and under odd neighbours), one f32
    ulp to either side of them, and on and next to bf16 values."""
    rng = np.random.default_rng(7)
    M, K = 130, 96
    hi = (rng.integers(0x3e80, 0x4100, (M, K)).astype(np.uint32) | (rng.integers(0, 2, (M, K)).astype(np.uint32) << 15))
    lo = rng.choice(np.array([0x8000, 0x8001, 0x7fff, 0x0000, 0x0001, 0xffff], np.uint32), (M, K))
    x = ((hi << 16) | lo).view(np.float32)
    ties = lo == 0x8000
    assert (ties & (hi & 1 == 0)).any() and (ties & (hi & 1 == 1)).any()
    w = np.zeros((K, K), np.float32)
    w[rng.permutation(K), np.arange(K)] = 1.0
    want = B.bf16_round(x) @ w  # a permutation of the columns, exact
    T.compare(dense_bf16(x, w), want, "rounded inputs")
    # the weights are rounded the same way: x = 1 picks a row of w
    T.compare(dense_bf16(w.T.copy(), x[:K].copy()), w.T @ B.bf16_round(x[:K]), "rounded weights")


@pytest.mark.parametrize("K", [17, 384, 512])
def test_dense_is_within_the_f32_accumulation_bound(K):
    """Random operands (with +0 and -0): against the float64 product e of the
    rounded operands, |got - e| <= 1.01 K 2^-23 sum_k |x^ w^| per element --
    at most K - 1 f32 additions, each off by at most 2^-23 relative (round to
    nearest or truncation) of a partial sum no larger than the sum of the
    terms' magnitudes; the products themselves are exact."""
    rng = np.random.default_rng(100 + K)

    def draw(shape):
        a = rng.standard_normal(shape).astype(np.float32)
        kind = rng.integers(0, 12, shape)
        a[kind == 0] = 0.0
        a[kind == 1] = -0.0
        small = (a != 0) & (np.abs(a) < 1e-30)  # nothing whose bf16 is subnormal
        a[small] = 1.0
        return a

    M, N = 130, 96
    x, w = draw((M, K)), draw((K, N))
    xh, wh = B.bf16_round(x).astype(np.float64), B.bf16_round(w).astype(np.float64)
    e = xh @ wh
    bound = 1.01 * K * 2.0 ** -23 * (np.abs(xh) @ np.abs(wh))
    got = dense_bf16(x, w).astype(np.float64)
    err = np.abs(got - e)
    print(f"K={K}: max |got - e| / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all(), (err - bound).max()


# ---------------------------------------------------------------- forward

@functools.lru_cache(maxsize=None)
def forward_case(d, ts, W, groups):
    """After 40 seek-and-fight steps: the exports, the RNG, the bf16 and the
    f32 forward of the GPU and the exports after them.  Computed once per
    shape and left unchanged."""
    e = engine(ts, W, groups)
    A = e.W * e.N
    tape = e.mem.upload(np.zeros((A, 6), np.int32))
    for s in range(40):
        e.mem.h2d(tape, T.mpenv_tape.tape_actions(SEED, s, 0, A))
        e.combat_actions(tape, None, 1)
        e.step()
    e.mem.free(tape)
    ok(e, e.lib.mpenv_policy_load(e.h, d.encode()))
    case = {"before": outputs(e), "obs": P.engine_obs(e), "rng": rng_of(e)}
    set_precision(e, B.BF16)
    case["bf16"] = forward(e)
    case["after_bf16"] = outputs(e)
    set_precision(e, B.F32)
    case["f32"] = forward(e)
    e.close()
    return case


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_forward_follows_the_contract(ckpts, ts, W, groups):
    """g: the GPU's bf16 logits, b: the numpy restatement of definition 17 on
    the same trunk inputs, a: definition 15.  g lies much nearer to b than b
    to a (another accumulation order only flips single bf16 roundings: on the
    CPU, other orders moved the mean by 0.003-0.007 of mean|b - a| and the
    maximum by 0.19-0.28 of max|b - a|; a dropped or misplaced rounding point
    moves the mean by the order of mean|b - a|), bf16 is not a no-op, and back
    at F32 the logits are definition 15's bit for bit."""
    d, ref, contract = ckpts[CKPT_SEED]
    case = forward_case(d, ts, W, groups)
    a, tin = ref.forward(case["obs"], trunk_in=True)
    b = contract.forward(tin).astype(np.float64)
    g = case["bf16"][0].astype(np.float64)
    gb, ba, ga = np.abs(g - b), np.abs(b - a), np.abs(g - a)
    print(f"{ts}v{ts} x {W}: mean|g-b| / mean|b-a| = {gb.mean() / ba.mean():.4g}, "
          f"max|g-b| / max|b-a| = {gb.max() / ba.max():.4g}, mean|b-a| = {ba.mean():.4g}, max|b-a| = {ba.max():.4g}")
    assert np.isfinite(g).all()
    assert gb.mean() <= ba.mean() / 20
    assert gb.max() <= ba.max()
    assert ga.mean() > 0
    T.compare(case["f32"][0], a, "logits back at F32")


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_sampling_is_exact_given_the_logits_and_forward_writes_no_state(ckpts, ts, W, groups):
    d, ref, _ = ckpts[CKPT_SEED]
    case = forward_case(d, ts, W, groups)
    logits, acts = case["bf16"]
    want, _ = ref.sample(logits, *case["rng"])
    T.compare(acts, want, "actions sampled from the bf16 logits")
    compare_all(case["after_bf16"], case["before"], "after the bf16 policy_forward")


# ---------------------------------------------------------------- step

@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_step_plays_forwards_actions_and_twin_trajectory_matches(ckpts, ts, W, groups):
    """Manager A steps in bf16 with mixed policy ids; its policy agents play
    the actions mpenv_policy_forward sampled just before, agents with id -2
    keep the tape's, and a twin without a policy, fed the played actions and
    with the policy agents' rngCtr raised by 6, equals it byte for byte.  The
    precision goes back to F32 at step 6 (from there on the played actions are
    definition 15's) and the step graph is not captured again."""
    import torch

    import mpenv_state

    d, ref, _ = ckpts[CKPT_SEED]
    a, b = engine(ts, W, groups), engine(ts, W, groups)
    A = a.W * a.N
    ids = mixed_ids(A)
    pol, alone = ids >= 0, ids == -2
    for e in (a, b):
        e.put("AGENT_POLICY", ids)
    set_precision(a, B.BF16)
    ok(a, a.lib.mpenv_policy_load(a.h, d.encode()))
    blob = torch.empty(b.state_bytes(), dtype=torch.uint8, device="cuda")
    pol_t = torch.from_numpy(np.flatnonzero(pol)).cuda()
    caps = []
    for s in range(12):
        if s == 6:
            set_precision(a, B.F32)
        given = T.mpenv_tape.tape_actions(SEED, s, 0, A)
        a.set_actions(given)
        _, want = forward(a)
        if s >= 6:
            obs = {k: v[pol] for k, v in P.engine_obs(a).items()}
            exact, _ = ref.sample(ref.forward(obs), *(r[pol] for r in rng_of(a)))
            T.compare(want[pol], exact, f"F32 forward @ {s}")
        a.step()
        caps.append(a.graph_captures())
        played = actions_of(a)
        T.compare(played[pol], want[pol], f"policy agents' actions @ {s}")
        T.compare(played[alone], given[alone], f"actions of agents with policy -2 @ {s}")
        b.state_save(blob.data_ptr())
        mpenv_state.view(blob, "rngCtr")[pol_t] += 6
        b.state_load(blob.data_ptr())
        b.set_actions(played)
        b.step()
        compare_all(outputs(a), outputs(b), f"step {s}")
    assert caps[0] >= 1 and caps[-1] == caps[0], caps
    a.close()
    b.close()


# ---------------------------------------------------------------- slots

def test_each_agent_plays_its_own_slots_bf16_forward(ckpts):
    """Checkpoints 21 and 22 in slots 0 and 3, bf16: ids 0 and 1 (an empty
    slot: the fallback) play slot 0's forward, id 3 plays slot 3's, and the
    two differ."""
    ts, W = 5, 13
    e = engine(ts, W)
    A = e.W * e.N
    ids = mixed_ids(A)
    e.put("AGENT_POLICY", ids)
    set_precision(e, B.BF16)
    for slot, seed in ((0, CKPT_SEED), (3, CKPT_SEED + 1)):
        ok(e, e.lib.mpenv_policy_load_slot(e.h, slot, ckpts[seed][0].encode()))
    serve = np.where(ids == 3, 3, np.where(ids >= 0, 0, -1))
    differ = False
    for s in range(4):
        given = T.mpenv_tape.tape_actions(SEED, s, 0, A)
        e.set_actions(given)
        by_slot = {slot: forward(e, slot) for slot in (0, 3)}
        differ |= bool((by_slot[0][1] != by_slot[3][1]).any())
        e.step()
        played = actions_of(e)
        for slot in (0, 3):
            sel = serve == slot
            assert sel.any()
            T.compare(played[sel], by_slot[slot][1][sel], f"actions of slot {slot}'s agents @ {s}")
        T.compare(played[ids == -2], given[ids == -2], f"actions of agents with policy -2 @ {s}")
    assert differ
    e.close()


# ---------------------------------------------------------------- surface

def test_precision_switch_surface(ckpts):
    d, ref, _ = ckpts[CKPT_SEED]
    e = engine(3, 5)
    assert precision(e) == B.F32  # the default
    for bad in (2, -1, 16):
        assert e.lib.mpenv_policy_set_precision(e.h, bad) == ERR_INVALID
        msg = e.lib.mpenv_last_error().decode()
        assert "MPENV_POLICY_F32" in msg and "MPENV_POLICY_BF16" in msg and str(bad) in msg
        assert precision(e) == B.F32
    # set with nothing loaded: the first load is served in bf16
    set_precision(e, B.BF16)
    assert precision(e) == B.BF16
    ok(e, e.lib.mpenv_policy_load(e.h, d.encode()))
    assert precision(e) == B.BF16
    exact = ref.forward(P.engine_obs(e))
    g, _ = forward(e)
    assert np.isfinite(g).all() and 0 < np.abs(g - exact).mean() < 0.25
    set_precision(e, B.F32)
    T.compare(forward(e)[0], exact, "logits at F32")
    # an unload keeps the switch
    set_precision(e, B.BF16)
    ok(e, e.lib.mpenv_policy_unload(e.h))
    assert precision(e) == B.BF16
    assert e.lib.mpenv_debug_policy_dense_bf16(e.h, None, 1, 1, None, 1, None, None) == ERR_INVALID
    x = e.mem.upload(np.zeros((1, 513), np.float32))
    w = np.zeros((513, 1), np.float32)
    assert e.lib.mpenv_debug_policy_dense_bf16(e.h, x, 1, 513, w.ctypes.data, 1, x, None) == ERR_INVALID
    assert "K <= 512" in e.lib.mpenv_last_error().decode()
    e.mem.free(x)
    e.close()


def test_python_surface(ckpts):
    import torch

    import madrona_mp_env as m

    d, ref, _ = ckpts[CKPT_SEED]
    kw = dict(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=3, rand_seed=5, auto_reset=True,
              sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone, team_size=2, num_pbt_policies=0,
              policy_history_size=0, scene_path=T.SCENE)
    sim = m.SimManager(**kw, policy_weights_path=d, policy_precision="bf16")
    assert sim.policy_loaded() and sim.policy_precision() == "bf16"
    sim.init()
    A = 3 * 4
    obs = {"self": sim.self_observation_tensor(), "coefs": sim.reward_coefs(), "pos": sim.self_pos(),
           "fwd": sim.fwd_lidar(), "rear": sim.rear_lidar(), "tm": sim.teammates(), "opp": sim.opponents(),
           "masks": sim.opponent_masks(), "lk": sim.opponents_last_known()}
    exact = ref.forward({k: t.to_torch().cpu().numpy() for k, t in obs.items()})

    def logits_now():
        lg = torch.full((A, P.LOGITS), float("nan"), device="cuda")
        sim.policy_forward(lg.data_ptr())
        torch.cuda.synchronize()
        return lg.cpu().numpy()

    g = logits_now()
    assert np.isfinite(g).all() and 0 < np.abs(g - exact).mean() < 0.25
    sim.set_policy_precision("f32")
    assert sim.policy_precision() == "f32"
    T.compare(logits_now(), exact, "logits at f32 through the Python module")
    sim.set_policy_precision("bf16")
    T.compare(logits_now(), g, "logits at bf16 again")
    with pytest.raises(Exception, match="f32.*bf16"):
        sim.set_policy_precision("fp8")
    assert sim.policy_precision() == "bf16"
    with pytest.raises(Exception, match="f32.*bf16"):
        m.SimManager(**kw, policy_precision="half")
    assert m.SimManager(**kw).policy_precision() == "f32"


def test_cpp_caller_switches_precision(ckpts, tmp_path):
    """tests/policy_bf16_hpp_caller.cpp: setPolicyPrecision / policyPrecision
    of include/mpenv_manager.hpp, compiled with -Wall -Werror."""
    d = ckpts[CKPT_SEED][0]
    exe = str(tmp_path / "policy_bf16_caller")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "policy_bf16_hpp_caller.cpp"), "-o", exe, "-L", T.PKG, "-lmpenv",
                    f"-Wl,-rpath,{T.PKG}"], check=True)
    r = subprocess.run([exe, T.SCENE, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "policy bf16 caller ok" in r.stdout
