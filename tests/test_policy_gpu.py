"""In-sim policy inference on the GPU (csrc/policy.hip, include/mpenv.h
mpenv_policy_*) against tests/policy_ref.cpp, bit for bit.

Shapes: the smallest that cross every boundary of the kernels -- 6 agents (one
partial wave of the embed kernel, one partial trunk tile), 42, 130 (past the
64- and 128-row tiles, a partial last tile) and 6v6 in three world groups."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mpenv_testlib as T
import policy_testlib as P

pytestmark = pytest.mark.gpu

SEED = 1234
CKPT_SEED = 21
# (team size, worlds, world groups)
SHAPES = [(1, 3, 1), (3, 7, 1), (5, 13, 1), (6, 7, 3)]
NAMES = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS
ERR_INVALID = -1
FULL_TEAM_POLICY = 1 << 9


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("policy") / "ckpt"
    tensors = P.write_checkpoint(d, CKPT_SEED)
    return str(d), P.Ref(tensors)


def engine(ts, W, groups=1, **kw):
    e = T.Engine(W, ts, **kw)
    if groups > 1:
        e.set_world_groups(groups)
    e.put_ctrl([0, 1, 1])
    e.init()
    return e


def load(e, d):
    assert e.lib.mpenv_policy_load(e.h, d.encode()) == 0, e.lib.mpenv_last_error().decode()


def loaded(e):
    on = C.c_int32(-1)
    assert e.lib.mpenv_policy_loaded(e.h, C.byref(on)) == 0
    return on.value


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


# ---------------------------------------------------------------- dense

@functools.lru_cache(maxsize=None)
def dense_engine():
    return engine(1, 1)


def special_values(rng, shape):
    """normals with subnormals, +0 and -0 mixed in"""
    x = rng.standard_normal(shape).astype(np.float32)
    kind = rng.integers(0, 12, shape)
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    sub = (rng.integers(1, 1 << 22, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 31))
    x[kind == 2] = sub.view(np.float32)[kind == 2]
    return x


@pytest.mark.parametrize("K", [2, 32, 100, 384, 512])
def test_dense_equals_the_cpu_chain_bit_for_bit(K):
    """mpenv_debug_policy_dense (the trunk's MFMA dense) against the
    k-ascending fmaf chain, for every N and M; subnormal, +0 and -0 inputs,
    and one row and one column of subnormals only (subnormal results)."""
    e = dense_engine()
    rng = np.random.default_rng(K)
    for N in (17, 20, 64, 512):
        w = special_values(rng, (K, N))
        w[:, 0] = np.float32(1e-30) * rng.standard_normal(K).astype(np.float32)
        for M in (1, 63, 65, 130):
            x = special_values(rng, (M, K))
            x[M - 1] = np.float32(1e-12) * rng.standard_normal(K).astype(np.float32)
            want = P.ref_dense(x, w)
            xd = e.mem.upload(x)
            yd = e.mem.upload(np.full((M, N), np.nan, np.float32))
            rc = e.lib.mpenv_debug_policy_dense(e.h, xd, M, K, w.ctypes.data, N, yd, None)
            assert rc == 0, e.lib.mpenv_last_error().decode()
            got = np.empty((M, N), np.float32)
            e.mem.d2h(yd, got.nbytes, got)
            e.mem.free(xd)
            e.mem.free(yd)
            T.compare(got, want, f"dense M={M} K={K} N={N}")
            assert (np.abs(want[M - 1, 0]) < np.float32(1.2e-38)).all()  # the subnormal corner is exercised


# ---------------------------------------------------------------- forward

@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_forward_equals_the_restatement_and_writes_no_state(ckpt, ts, W, groups):
    """40 steps of the seek-and-fight action source (masks, last-known rows,
    deaths and respawns live), then mpenv_policy_forward: logits and sampled
    actions equal the restatement fed the engine's exports, and no export or
    debug column changed, rngCtr included."""
    d, ref = ckpt
    e = engine(ts, W, groups)
    A = e.W * e.N
    tape = e.mem.upload(np.zeros((A, 6), np.int32))
    for s in range(40):
        e.mem.h2d(tape, T.mpenv_tape.tape_actions(SEED, s, 0, A))
        e.combat_actions(tape, None, 1)
        e.step()
    e.mem.free(tape)
    load(e, d)
    before = outputs(e)
    assert (before["OPPONENT_MASKS"] > 0).any() or ts == 1
    lg_d = e.mem.upload(np.full((A, P.LOGITS), np.nan, np.float32))
    ac_d = e.mem.upload(np.full((A, 6), -7, np.int32))
    assert e.lib.mpenv_policy_forward(e.h, lg_d, ac_d, None) == 0, e.lib.mpenv_last_error().decode()
    e.mem.hip.hipDeviceSynchronize()
    logits, acts = np.empty((A, P.LOGITS), np.float32), np.empty((A, 6), np.int32)
    e.mem.d2h(lg_d, logits.nbytes, logits)
    e.mem.d2h(ac_d, acts.nbytes, acts)
    compare_all(outputs(e), before, "after policy_forward")
    want = ref.forward(P.engine_obs(e))
    T.compare(logits, want, "logits")
    want_acts, _ = ref.sample(want, *rng_of(e))
    T.compare(acts, want_acts, "actions")
    # logits only: the actions buffer stays as it was
    e.mem.h2d(ac_d, np.full((A, 6), -7, np.int32))
    assert e.lib.mpenv_policy_forward(e.h, lg_d, None, None) == 0
    e.mem.hip.hipDeviceSynchronize()
    e.mem.d2h(ac_d, acts.nbytes, acts)
    assert (acts == -7).all()
    e.mem.free(lg_d)
    e.mem.free(ac_d)
    e.close()


# ---------------------------------------------------------------- step and twin trajectory

@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_step_writes_policy_agents_actions_and_twin_trajectory_matches(ckpt, ts, W, groups):
    """Manager A steps with the policy loaded and mixed policy ids; manager B
    has none and is fed A's played actions, its policy agents' rngCtr raised
    by 6 through a state snapshot before each step.  A's policy agents'
    actions equal the restatement's sample from the pre-step RNG, agents with
    id -2 keep the tape's, and B equals A byte for byte at every step (so
    rngCtr rose by exactly 6 beyond the step's own draws, for nobody else)."""
    import torch

    import mpenv_state

    d, ref = ckpt
    a, b = engine(ts, W, groups), engine(ts, W, groups)
    A = a.W * a.N
    ids = mixed_ids(A)
    pol, alone = ids >= 0, ids == -2
    for e in (a, b):
        e.put("AGENT_POLICY", ids)
    load(a, d)
    assert loaded(a) == 1 and loaded(b) == 0
    blob = torch.empty(b.state_bytes(), dtype=torch.uint8, device="cuda")
    pol_t = torch.from_numpy(np.flatnonzero(pol)).cuda()
    caps = []
    for s in range(30):
        given = T.mpenv_tape.tape_actions(SEED, s, 0, A)
        a.set_actions(given)
        check = s < 3 or s % 6 == 0
        if check:
            obs = {k: v[pol] for k, v in P.engine_obs(a).items()}
            want, _ = ref.sample(ref.forward(obs), *(r[pol] for r in rng_of(a)))
        a.step()
        caps.append(a.graph_captures())
        played = actions_of(a)
        if check:
            T.compare(played[pol], want, f"policy agents' actions @ {s}")
        T.compare(played[alone], given[alone], f"actions of agents with policy -2 @ {s}")
        # B: the same step without a policy
        b.state_save(blob.data_ptr())
        mpenv_state.view(blob, "rngCtr")[pol_t] += 6
        b.state_load(blob.data_ptr())
        b.set_actions(played)
        b.step()
        compare_all(outputs(a), outputs(b), f"step {s}")
    assert caps[0] >= 1 and caps[-1] == caps[0], caps  # the step graph is captured once
    a.close()
    b.close()


# ---------------------------------------------------------------- stream path, unload

def test_gpu_stream_step_plays_the_same_actions_as_step(ckpt):
    import torch

    d, _ = ckpt
    ts, W = 3, 7
    a = engine(ts, W)
    b = T.Engine(W, ts)
    A = a.W * a.N
    ids = mixed_ids(A)
    sb = T.StreamBuffers(b, n_sets=1)
    bufs, arr = sb.sets[0], sb.arrs[0]
    sb.put(0, "pbt.policy_assignments", ids)
    a.put("AGENT_POLICY", ids)
    b.put_ctrl([0, 1, 1])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    b.gpu_stream_init(stream.cuda_stream, arr)
    stream.synchronize()
    load(a, d)
    load(b, d)
    for s in range(8):
        given = T.mpenv_tape.tape_actions(SEED, s, 0, A)
        a.set_actions(given)
        a.step()
        sb.set_actions(0, given)
        torch.cuda.synchronize()
        b.gpu_stream_step(stream.cuda_stream, arr)
        stream.synchronize()
        T.compare(actions_of(b), actions_of(a), f"played actions @ {s}")
        for (io, nm, ename, _, _), t in zip(sb.ti, bufs):
            if io == 1 and "agent_map" not in nm:
                T.compare(t.cpu().numpy(), a.get(ename), f"{nm} @ {s}")
    compare_all(outputs(b), outputs(a), "after the stream steps")
    a.close()
    b.close()


def test_unloaded_manager_equals_one_that_never_loaded(ckpt):
    d, _ = ckpt
    ts, W = 3, 7
    a, b = engine(ts, W), engine(ts, W)
    A = a.W * a.N
    load(a, d)
    for e in (a, b):  # nobody on the policy: a loaded policy then changes nothing
        e.put("AGENT_POLICY", np.full(A, -2, np.int32))
    for s in range(6):
        if s == 3:
            assert loaded(a) == 1
            assert a.lib.mpenv_policy_unload(a.h) == 0
            assert loaded(a) == 0
            for e in (a, b):  # everybody on it: nothing is loaded to evaluate
                e.put("AGENT_POLICY", np.zeros(A, np.int32))
        acts = T.mpenv_tape.tape_actions(SEED, s, 0, A)
        for e in (a, b):
            e.set_actions(acts)
            e.step()
        compare_all(outputs(a), outputs(b), f"step {s}")
    lg = a.mem.upload(np.zeros((A, P.LOGITS), np.float32))
    assert a.lib.mpenv_policy_forward(a.h, lg, None, None) == ERR_INVALID
    assert "no policy loaded" in a.lib.mpenv_last_error().decode()
    a.mem.free(lg)
    a.close()
    b.close()


# ---------------------------------------------------------------- surface

def test_refusals_name_their_reason(ckpt, tmp_path):
    d, _ = ckpt
    rec = T.Engine(2, 1, record=str(tmp_path / "rec.bin"))
    assert rec.lib.mpenv_policy_load(rec.h, d.encode()) == ERR_INVALID
    assert "record_log_path" in rec.lib.mpenv_last_error().decode()
    rec.put_ctrl([0, 1, 1])
    rec.init()
    rec.step()
    rec.close()
    rep = T.Engine(2, 1, replay=str(tmp_path / "rec.bin"))
    assert rep.lib.mpenv_policy_load(rep.h, d.encode()) == ERR_INVALID
    assert "replay_log_path" in rep.lib.mpenv_last_error().decode()
    rep.close()
    (tmp_path / "events").mkdir()
    ev = T.Engine(2, 1, events=str(tmp_path / "events"))
    assert ev.lib.mpenv_policy_load(ev.h, d.encode()) == ERR_INVALID
    assert "event_log_path" in ev.lib.mpenv_last_error().decode()
    ev.close()
    ft = T.Engine(2, 1, sim_flags=FULL_TEAM_POLICY)
    assert ft.lib.mpenv_policy_load(ft.h, d.encode()) == ERR_INVALID
    assert "FullTeamPolicy" in ft.lib.mpenv_last_error().decode()
    ft.close()
    e = T.Engine(2, 1)
    broken = tmp_path / "broken"
    P.write_checkpoint(broken, 1)
    os.remove(broken / "params_backbone_prefix_self_embed_kernel")
    assert e.lib.mpenv_policy_load(e.h, str(broken).encode()) == -2
    assert "params_backbone_prefix_self_embed_kernel" in e.lib.mpenv_last_error().decode()
    assert loaded(e) == 0
    e.close()


def test_load_is_refused_after_a_direct_stream_step_until_a_plain_step(ckpt):
    """A direct mpenv_gpu_stream_step leaves the engine's own observation rows,
    the network's inputs, a step behind: no load until a plain step."""
    import torch

    d, _ = ckpt
    ts, W = 3, 5
    A = W * 2 * ts
    e = T.Engine(W, ts)
    sb = T.StreamBuffers(e, n_sets=1)
    e.put_ctrl([0, 1, 1])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    e.gpu_stream_init(stream.cuda_stream, sb.arrs[0])
    sb.set_actions(0, T.mpenv_tape.tape_actions(SEED, 0, 0, A))
    torch.cuda.synchronize()
    e.gpu_stream_step(stream.cuda_stream, sb.arrs[0])
    stream.synchronize()
    assert e.lib.mpenv_policy_load(e.h, d.encode()) == ERR_INVALID
    assert "mpenv_gpu_stream_step" in e.lib.mpenv_last_error().decode()
    assert loaded(e) == 0
    e.set_actions(T.mpenv_tape.tape_actions(SEED, 1, 0, A))
    e.step()
    load(e, d)
    assert loaded(e) == 1
    e.close()


def test_python_surface(ckpt, tmp_path):
    import torch

    import madrona_mp_env as m

    d, ref = ckpt
    kw = dict(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=3, rand_seed=5, auto_reset=True,
              sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone, team_size=2, num_pbt_policies=0,
              policy_history_size=0, scene_path=T.SCENE)
    m.policy_check(d)
    sim = m.SimManager(**kw, policy_weights_path=d)
    assert sim.policy_loaded()
    sim.init()
    A = 3 * 4
    logits = torch.full((A, P.LOGITS), float("nan"), device="cuda")
    actions = torch.full((A, 6), -1, dtype=torch.int32, device="cuda")
    sim.policy_forward(logits.data_ptr(), actions.data_ptr())
    torch.cuda.synchronize()
    obs = {"self": sim.self_observation_tensor(), "coefs": sim.reward_coefs(), "pos": sim.self_pos(),
           "fwd": sim.fwd_lidar(), "rear": sim.rear_lidar(), "tm": sim.teammates(), "opp": sim.opponents(),
           "masks": sim.opponent_masks(), "lk": sim.opponents_last_known()}
    want = ref.forward({k: t.to_torch().cpu().numpy() for k, t in obs.items()})
    T.compare(logits.cpu().numpy(), want, "logits through the Python module")
    sim.step()  # the default policy id is 0: the step plays the sampled actions
    played = torch.cat([sim.pvp_action_tensor().to_torch().view(A, 4), sim.aim_action_tensor().to_torch().view(A, 2)], 1)
    assert torch.equal(played.cpu(), actions.cpu())
    sim.unload_policy()
    assert not sim.policy_loaded()
    sim.load_policy(d)
    assert sim.policy_loaded()
    with pytest.raises(Exception, match="cannot open"):
        m.SimManager(**kw, policy_weights_path=str(tmp_path / "nowhere"))
    with pytest.raises(Exception, match="cannot open"):
        m.policy_check(str(tmp_path / "nowhere"))


def test_cpp_caller_with_policy_weights_path(ckpt, tmp_path):
    """tests/policy_hpp_caller.cpp sets Manager::Config::policyWeightsPath
    (mgr.hpp:49): it is honoured, and a directory that does not load throws."""
    d, _ = ckpt
    exe = str(tmp_path / "policy_caller")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "policy_hpp_caller.cpp"), "-o", exe, "-L", T.PKG, "-lmpenv",
                    f"-Wl,-rpath,{T.PKG}"], check=True)
    r = subprocess.run([exe, T.SCENE, d, str(tmp_path / "nowhere")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "policy caller ok" in r.stdout
