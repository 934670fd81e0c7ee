"""League play on the GPU: one frozen checkpoint per policy id inside the step
(include/mpenv_policy_slots.h, csrc/policy.hip selection kernels) against
tests/policy_ref.cpp over the checkpoint that serves each agent, bit for bit.

Shapes: 6v6 x 12 worlds (144 agents) holds the per-slot counts 65 / 64 / 1 --
a segment one past a tile, one exactly a tile, one of a single agent -- with
agents on -1 and -2 besides; the second and third id layouts give a segment
one short of a tile and a loaded slot with no agent between two used ones."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mpenv_testlib as T
import policy_slots_abi
import policy_testlib as P

pytestmark = pytest.mark.gpu

SEED = 1234
NAMES = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS
ERR_INVALID, ERR_IO = -1, -2
FULL_TEAM_POLICY = 1 << 9
SLOTS = policy_slots_abi.POLICY_SLOTS
# checkpoint seeds: the slots of the league, the unused slot 7, and the one swapped in
CKPT_SEEDS = {"s0": 31, "s2": 32, "s5": 33, "s7": 34, "swap": 35}


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """{name: (directory, P.Ref)}: distinct checkpoints, written once"""
    root = tmp_path_factory.mktemp("league")
    out = {}
    for name, seed in CKPT_SEEDS.items():
        d = root / name
        out[name] = (str(d), P.Ref(P.write_checkpoint(d, seed)))
    return out


def engine(ts, W, groups=1, **kw):
    e = T.Engine(W, ts, **kw)
    policy_slots_abi.bind(e.lib)
    if groups > 1:
        e.set_world_groups(groups)
    e.put_ctrl([0, 1, 1])
    e.init()
    return e


def load_slot(e, slot, d):
    assert e.lib.mpenv_policy_load_slot(e.h, slot, d.encode()) == 0, e.lib.mpenv_last_error().decode()


def unload_slot(e, slot):
    assert e.lib.mpenv_policy_unload_slot(e.h, slot) == 0, e.lib.mpenv_last_error().decode()


def slot_mask(e):
    m = C.c_uint32(0xdead)
    assert e.lib.mpenv_policy_slots(e.h, C.byref(m)) == 0
    return m.value


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


def serving_slot(ids, occupied):
    """The rule of mpenv_policy_slots.h, restated: per agent the slot that
    evaluates it, -1 for nobody.  occupied: the slots that hold a checkpoint."""
    ids = np.asarray(ids)
    own = np.isin(ids, list(occupied)) & (ids >= 0) & (ids < SLOTS)
    return np.where(ids < 0, -1, np.where(own, ids, 0 if 0 in occupied else -1)).astype(np.int32)


def dealt(A, counts, seed):
    """[A] policy ids: counts = {id: how many}, the rest -1 and -2 in turn, shuffled over the worlds"""
    ids = [p for p, n in counts.items() for _ in range(n)]
    ids += [-1 - (k & 1) for k in range(A - len(ids))]
    assert len(ids) == A
    return np.random.default_rng(seed).permutation(np.array(ids, np.int32))


# 144 agents; slot 0 serves ids 0, 1 and 40 (1: an empty slot, 40: past the last slot)
LAYOUTS = {
    "65-64-1": {0: 40, 1: 15, 40: 10, 2: 64, 5: 1},
    "63-1-0": {0: 40, 1: 13, 40: 10, 2: 1},
    "63-0-1": {0: 40, 1: 13, 40: 10, 5: 1},
}
LAYOUT_COUNTS = {"65-64-1": (65, 64, 1), "63-1-0": (63, 1, 0), "63-0-1": (63, 0, 1)}


def wanted_actions(e, refs, serve):
    """[A][6] from the engine's current exports and RNG: each agent through
    the restatement of the checkpoint that serves it (rows of agents nobody
    serves are not meaningful); refs: {slot: P.Ref}"""
    obs, rng = P.engine_obs(e), rng_of(e)
    want = np.zeros((len(serve), 6), np.int32)
    for slot, ref in refs.items():
        sel = serve == slot
        if sel.any():
            o = {k: v[sel] for k, v in obs.items()}
            want[sel], _ = ref.sample(ref.forward(o), *(r[sel] for r in rng))
    return want


def policy_step(a, refs, ids, s, twin=None, blob=None):
    """One step of `a` (slots refs loaded) on the tape's actions: the served
    agents play their checkpoint's restatement, agents with -2 and agents with
    an id >= 0 that nobody serves keep the tape's.  twin: a manager without a
    policy that is fed the played actions, the served agents' rngCtr raised by
    6 through a snapshot; it must equal `a` byte for byte after the step."""
    import torch

    import mpenv_state

    A = len(ids)
    serve = serving_slot(ids, set(refs))
    served = serve >= 0
    given = T.mpenv_tape.tape_actions(SEED, s, 0, A)
    a.set_actions(given)
    want = wanted_actions(a, refs, serve)
    a.step()
    played = actions_of(a)
    for slot in refs:
        sel = serve == slot
        T.compare(played[sel], want[sel], f"actions of slot {slot}'s agents @ {s}")
    kept = (ids == -2) | ((ids >= 0) & ~served)
    T.compare(played[kept], given[kept], f"actions of agents nobody evaluates @ {s}")
    if twin is not None:
        twin.state_save(blob.data_ptr())
        mpenv_state.view(blob, "rngCtr")[torch.from_numpy(np.flatnonzero(served)).cuda()] += 6
        twin.state_load(blob.data_ptr())
        twin.set_actions(played)
        twin.step()
        compare_all(outputs(a), outputs(twin), f"step {s}")
    return played, serve


# ---------------------------------------------------------------- 1: each id its own checkpoint

@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_each_policy_id_is_served_by_its_own_checkpoint(ckpts, layout, groups):
    """Slots 0, 2 and 5 serve their ids (1 and 40 fall back to slot 0), slot 7
    is loaded and serves nobody; 12 steps, every served agent's played actions
    against the restatement of its own checkpoint.  The restatements of every
    two checkpoints differ on some compared agent, so one checkpoint serving
    everybody does not pass."""
    ts, W = 6, 12
    e = engine(ts, W, groups)
    A = e.W * e.N
    ids = dealt(A, LAYOUTS[layout], 3)
    e.put("AGENT_POLICY", ids)
    refs = {}
    for slot, name in ((0, "s0"), (2, "s2"), (5, "s5"), (7, "s7")):
        load_slot(e, slot, ckpts[name][0])
        refs[slot] = ckpts[name][1]
    assert slot_mask(e) == 0b10100101 and loaded(e) == 1
    serve = serving_slot(ids, set(refs))
    assert tuple(int((serve == s).sum()) for s in (0, 2, 5)) == LAYOUT_COUNTS[layout]
    assert (serve == 7).sum() == 0 and (ids == -1).any() and (ids == -2).any()
    used = [s for s in (0, 2, 5) if (serve == s).any()]
    differ = {(i, j): False for i in used for j in used if i < j}
    for s in range(12):
        # the first two steps: both checkpoints over the agents of either, before the step moves the RNG
        for (i, j) in (differ if s < 2 else ()):
            both = (serve == i) | (serve == j)
            wi = wanted_actions(e, {i: refs[i]}, np.where(both, i, -1))
            wj = wanted_actions(e, {j: refs[j]}, np.where(both, j, -1))
            differ[(i, j)] |= bool((wi[both] != wj[both]).any())
        policy_step(e, refs, ids, s)
    assert all(differ.values()), differ
    e.close()


# ---------------------------------------------------------------- 2: twin trajectory

def test_twin_without_a_policy_fed_the_played_actions_matches(ckpts):
    """20 steps in three world groups: the twin equals the league manager on
    every export and debug column, so rngCtr rose by exactly 6 beyond the
    step's own draws for the served agents and for nobody else; the step graph
    is captured once."""
    import torch

    ts, W = 6, 12
    a, b = engine(ts, W, 3), engine(ts, W, 3)
    A = a.W * a.N
    ids = dealt(A, LAYOUTS["65-64-1"], 4)
    for e in (a, b):
        e.put("AGENT_POLICY", ids)
    refs = {}
    for slot, name in ((0, "s0"), (2, "s2"), (5, "s5")):
        load_slot(a, slot, ckpts[name][0])
        refs[slot] = ckpts[name][1]
    blob = torch.empty(b.state_bytes(), dtype=torch.uint8, device="cuda")
    caps = []
    for s in range(20):
        policy_step(a, refs, ids, s, b, blob)
        caps.append(a.graph_captures())
    assert caps[0] >= 1 and caps[-1] == caps[0], caps
    a.close()
    b.close()


# ---------------------------------------------------------------- 3: list order

def test_result_does_not_depend_on_the_order_inside_a_segment(ckpts):
    """The scatter's atomics order a segment differently from run to run: the
    same step from the same snapshot gives the same bytes every time."""
    import torch

    ts, W = 6, 12
    e = engine(ts, W, 3)
    A = e.W * e.N
    ids = dealt(A, LAYOUTS["65-64-1"], 5)
    e.put("AGENT_POLICY", ids)
    for slot, name in ((0, "s0"), (2, "s2"), (5, "s5")):
        load_slot(e, slot, ckpts[name][0])
    for s in range(2):
        e.set_actions(T.mpenv_tape.tape_actions(SEED, s, 0, A))
        e.step()
    blob = torch.empty(e.state_bytes(), dtype=torch.uint8, device="cuda")
    e.state_save(blob.data_ptr())
    given = T.mpenv_tape.tape_actions(SEED, 2, 0, A)
    first = None
    for k in range(4):  # the first run and three repeats
        if k:
            e.state_load(blob.data_ptr())
        e.set_actions(given)
        e.step()
        got = outputs(e)
        if first is None:
            first = got
        else:
            compare_all(got, first, f"repeat {k}")
    e.close()


# ---------------------------------------------------------------- 4: hot swap, unload, fallback

def test_hot_swap_unload_fallback_and_failed_load(ckpts, tmp_path):
    import torch

    ts, W = 3, 7
    a, b = engine(ts, W), engine(ts, W)
    A = a.W * a.N
    ids = np.resize(np.array([0, 2, 5, -2, 1, 40, 2, -1, 5, 0, 2], np.int32), A)
    for e in (a, b):
        e.put("AGENT_POLICY", ids)
    refs = {}
    for slot, name in ((0, "s0"), (2, "s2"), (5, "s5")):
        load_slot(a, slot, ckpts[name][0])
        refs[slot] = ckpts[name][1]
    blob = torch.empty(b.state_bytes(), dtype=torch.uint8, device="cuda")
    caps = a.graph_captures
    step = iter(range(100))

    def run(n):
        for _ in range(n):
            policy_step(a, refs, ids, next(step), b, blob)

    run(2)
    caps0 = caps()
    # hot swap: id 2 follows the new checkpoint from the next step on, the others their own
    load_slot(a, 2, ckpts["swap"][0])
    refs[2] = ckpts["swap"][1]
    assert slot_mask(a) == 0b100101
    run(2)
    # a load that fails leaves the slot as it was
    broken = tmp_path / "broken"
    P.write_checkpoint(broken, 1)
    os.remove(broken / "params_backbone_prefix_self_embed_kernel")
    assert a.lib.mpenv_policy_load_slot(a.h, 2, str(broken).encode()) == ERR_IO
    assert "params_backbone_prefix_self_embed_kernel" in a.lib.mpenv_last_error().decode()
    assert slot_mask(a) == 0b100101
    run(2)
    # id 2 falls back to slot 0
    unload_slot(a, 2)
    del refs[2]
    assert slot_mask(a) == 0b100001
    assert (serving_slot(ids, set(refs))[ids == 2] == 0).all()
    run(2)
    # slot 0 empty, slot 5 still loaded: ids 0, 1, 2 and 40 are not evaluated (the
    # twin raises nobody's rngCtr but id 5's), id 5 still is
    unload_slot(a, 0)
    del refs[0]
    assert slot_mask(a) == 0b100000 and loaded(a) == 1
    serve = serving_slot(ids, set(refs))
    assert (serve[np.isin(ids, [0, 1, 2, 40])] == -1).all() and (serve[ids == 5] == 5).all()
    run(2)
    # the last unload: a manager that never loaded
    unload_slot(a, 5)
    del refs[5]
    assert slot_mask(a) == 0 and loaded(a) == 0
    unload_slot(a, 5)  # emptying an empty slot is no error
    run(3)
    # and loading again after everything was freed
    load_slot(a, 5, ckpts["s5"][0])
    refs[5] = ckpts["s5"][1]
    run(1)
    assert caps() == caps0  # no load or unload re-captures the step graph
    for bad in (-1, SLOTS):
        assert a.lib.mpenv_policy_load_slot(a.h, bad, ckpts["s0"][0].encode()) == ERR_INVALID
        assert f"[0, {SLOTS})" in a.lib.mpenv_last_error().decode()
        assert a.lib.mpenv_policy_unload_slot(a.h, bad) == ERR_INVALID
        assert f"[0, {SLOTS})" in a.lib.mpenv_last_error().decode()
    a.close()
    b.close()


# ---------------------------------------------------------------- 5: forward_slot

def test_forward_slot_evaluates_every_agent_through_that_slot(ckpts):
    ts, W = 3, 7
    e = engine(ts, W)
    A = e.W * e.N
    for s in range(4):
        e.set_actions(T.mpenv_tape.tape_actions(SEED, s, 0, A))
        e.step()
    load_slot(e, 0, ckpts["s0"][0])
    load_slot(e, 5, ckpts["s5"][0])
    before = outputs(e)
    lg_d = e.mem.upload(np.full((A, P.LOGITS), np.nan, np.float32))
    ac_d = e.mem.upload(np.full((A, 6), -7, np.int32))

    def fetch():
        e.mem.hip.hipDeviceSynchronize()
        logits, acts = np.empty((A, P.LOGITS), np.float32), np.empty((A, 6), np.int32)
        e.mem.d2h(lg_d, logits.nbytes, logits)
        e.mem.d2h(ac_d, acts.nbytes, acts)
        return logits, acts

    assert e.lib.mpenv_policy_forward_slot(e.h, 5, lg_d, ac_d, None) == 0, e.lib.mpenv_last_error().decode()
    logits5, acts5 = fetch()
    compare_all(outputs(e), before, "after forward_slot")
    obs = P.engine_obs(e)
    want5 = ckpts["s5"][1].forward(obs)
    T.compare(logits5, want5, "logits through slot 5")
    T.compare(acts5, ckpts["s5"][1].sample(want5, *rng_of(e))[0], "actions through slot 5")
    assert e.lib.mpenv_policy_forward_slot(e.h, 0, lg_d, ac_d, None) == 0
    logits0, acts0 = fetch()
    T.compare(logits0, ckpts["s0"][1].forward(obs), "logits through slot 0")
    assert (logits0 != logits5).any()
    assert e.lib.mpenv_policy_forward(e.h, lg_d, ac_d, None) == 0
    logits, acts = fetch()
    T.compare(logits, logits0, "mpenv_policy_forward against forward_slot(0): logits")
    T.compare(acts, acts0, "mpenv_policy_forward against forward_slot(0): actions")
    assert e.lib.mpenv_policy_forward_slot(e.h, 9, lg_d, ac_d, None) == ERR_INVALID
    assert "slot 9 is empty" in e.lib.mpenv_last_error().decode()
    assert e.lib.mpenv_policy_forward_slot(e.h, SLOTS, lg_d, ac_d, None) == ERR_INVALID
    assert f"[0, {SLOTS})" in e.lib.mpenv_last_error().decode()
    unload_slot(e, 0)  # slot 5 alone: the one-checkpoint call keeps its message
    assert e.lib.mpenv_policy_forward(e.h, lg_d, ac_d, None) == ERR_INVALID
    assert "no policy loaded" in e.lib.mpenv_last_error().decode()
    compare_all(outputs(e), before, "after the refused calls")
    e.mem.free(lg_d)
    e.mem.free(ac_d)
    e.close()


# ---------------------------------------------------------------- 6: gpuStreamStep

def test_gpu_stream_step_plays_the_same_actions_as_step(ckpts):
    import torch

    ts, W = 3, 7
    a = engine(ts, W)
    b = T.Engine(W, ts)
    policy_slots_abi.bind(b.lib)
    A = a.W * a.N
    ids = np.resize(np.array([0, -1, -2, 3, 1, 0, -2], np.int32), A)
    sb = T.StreamBuffers(b, n_sets=1)
    bufs, arr = sb.sets[0], sb.arrs[0]
    sb.put(0, "pbt.policy_assignments", ids)
    a.put("AGENT_POLICY", ids)
    b.put_ctrl([0, 1, 1])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    b.gpu_stream_init(stream.cuda_stream, arr)
    stream.synchronize()
    refs = {0: ckpts["s0"][1], 3: ckpts["s2"][1]}
    for e in (a, b):
        load_slot(e, 0, ckpts["s0"][0])
        load_slot(e, 3, ckpts["s2"][0])
    for s in range(6):
        given = T.mpenv_tape.tape_actions(SEED, s, 0, A)
        sb.set_actions(0, given)
        torch.cuda.synchronize()
        b.gpu_stream_step(stream.cuda_stream, arr)
        stream.synchronize()
        policy_step(a, refs, ids, s)
        T.compare(actions_of(b), actions_of(a), f"played actions @ {s}")
        for (io, nm, ename, _, _), t in zip(sb.ti, bufs):
            if io == 1 and "agent_map" not in nm:
                T.compare(t.cpu().numpy(), a.get(ename), f"{nm} @ {s}")
    compare_all(outputs(b), outputs(a), "after the stream steps")
    a.close()
    b.close()


# ---------------------------------------------------------------- 7: refusals per slot

def test_every_slot_refuses_what_slot_0_refuses_in_the_same_words(ckpts, tmp_path):
    import torch

    d = ckpts["s0"][0].encode()

    def refused_alike(e, needle):
        msgs = []
        for call in (lambda: e.lib.mpenv_policy_load(e.h, d), lambda: e.lib.mpenv_policy_load_slot(e.h, 3, d)):
            assert call() == ERR_INVALID
            msgs.append(e.lib.mpenv_last_error().decode())
        assert needle in msgs[0] and msgs[1] == msgs[0], msgs
        assert slot_mask(e) == 0 and loaded(e) == 0

    rec = T.Engine(2, 1, record=str(tmp_path / "rec.bin"))
    policy_slots_abi.bind(rec.lib)
    refused_alike(rec, "record_log_path")
    rec.put_ctrl([0, 1, 1])
    rec.init()
    rec.step()
    rec.close()
    rep = T.Engine(2, 1, replay=str(tmp_path / "rec.bin"))
    refused_alike(rep, "replay_log_path")
    rep.close()
    (tmp_path / "events").mkdir()
    ev = T.Engine(2, 1, events=str(tmp_path / "events"))
    refused_alike(ev, "event_log_path")
    ev.close()
    ft = T.Engine(2, 1, sim_flags=FULL_TEAM_POLICY)
    refused_alike(ft, "FullTeamPolicy")
    ft.close()
    # after a direct stream step, until a plain step
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
    refused_alike(e, "mpenv_gpu_stream_step")
    e.set_actions(T.mpenv_tape.tape_actions(SEED, 1, 0, A))
    e.step()
    load_slot(e, 3, ckpts["s0"][0])
    assert slot_mask(e) == 1 << 3 and loaded(e) == 1
    e.close()


# ---------------------------------------------------------------- 8: Python and C++ surfaces

def test_python_surface(ckpts):
    import torch

    import madrona_mp_env as m

    (d0, ref0), (d3, ref3), (d5, _) = ckpts["s0"], ckpts["s2"], ckpts["s5"]
    kw = dict(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=3, rand_seed=5, auto_reset=True,
              sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone, team_size=2, num_pbt_policies=0,
              policy_history_size=0, scene_path=T.SCENE)
    sim = m.SimManager(**kw, policy_weights_path={0: d0, 3: d3})
    assert sim.policy_slots() == [0, 3] and sim.policy_loaded()
    sim.init()
    A = 3 * 4
    pol = sim.policy_assignment_tensor().to_torch()
    ids = np.resize(np.array([3, 0, -2, 3, 7], np.int32), A)
    pol.copy_(torch.from_numpy(ids).view_as(pol))
    obs = {"self": sim.self_observation_tensor(), "coefs": sim.reward_coefs(), "pos": sim.self_pos(),
           "fwd": sim.fwd_lidar(), "rear": sim.rear_lidar(), "tm": sim.teammates(), "opp": sim.opponents(),
           "masks": sim.opponent_masks(), "lk": sim.opponents_last_known()}
    obs = {k: t.to_torch().cpu().numpy() for k, t in obs.items()}
    logits = torch.full((A, P.LOGITS), float("nan"), device="cuda")
    acts = {}
    for pid, ref in ((0, ref0), (3, ref3)):
        actions = torch.full((A, 6), -1, dtype=torch.int32, device="cuda")
        sim.policy_forward(logits.data_ptr(), actions.data_ptr(), 0, policy_id=pid)
        torch.cuda.synchronize()
        T.compare(logits.cpu().numpy(), ref.forward(obs), f"logits of policy id {pid} through the Python module")
        acts[pid] = actions.cpu()
    sim.policy_forward(logits.data_ptr())  # positional, as before: policy id 0
    torch.cuda.synchronize()
    T.compare(logits.cpu().numpy(), ref0.forward(obs), "logits of the positional call")
    given = torch.from_numpy(T.mpenv_tape.tape_actions(SEED, 0, 0, A))
    sim.pvp_action_tensor().to_torch().copy_(given[:, :4].reshape(sim.pvp_action_tensor().to_torch().shape))
    sim.aim_action_tensor().to_torch().copy_(given[:, 4:6].reshape(sim.aim_action_tensor().to_torch().shape))
    sim.step()
    played = torch.cat([sim.pvp_action_tensor().to_torch().view(A, 4), sim.aim_action_tensor().to_torch().view(A, 2)],
                       1).cpu()
    want = torch.where(torch.from_numpy(ids == 3)[:, None], acts[3], acts[0])  # id 7 falls back to id 0's
    want = torch.where(torch.from_numpy(ids == -2)[:, None], given, want)
    assert torch.equal(played, want)
    sim.load_policy(d5, policy_id=5)
    sim.load_policy(d5, 6)
    assert sim.policy_slots() == [0, 3, 5, 6]
    sim.unload_policy(3)
    sim.unload_policy(policy_id=6)
    assert sim.policy_slots() == [0, 5] and sim.policy_loaded()
    sim.unload_policy()
    assert sim.policy_slots() == [] and not sim.policy_loaded()
    sim.load_policy(d0)
    assert sim.policy_slots() == [0]
    with pytest.raises(Exception, match=r"\[0, 32\)"):
        sim.load_policy(d0, policy_id=32)
    with pytest.raises(Exception, match="cannot open"):
        m.SimManager(**kw, policy_weights_path={0: d0, 4: d0 + "_nowhere"})
    assert m.SimManager(**kw, policy_weights_path=d0).policy_slots() == [0]  # a string, as before


def test_cpp_caller_with_policy_ids(ckpts, tmp_path):
    """tests/policy_slots_hpp_caller.cpp: loadPolicy(dir, id), unloadPolicy(id),
    policySlots and policyForward(..., id) of include/mpenv_manager.hpp."""
    exe = str(tmp_path / "policy_slots_caller")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "policy_slots_hpp_caller.cpp"), "-o", exe, "-L", T.PKG, "-lmpenv",
                    f"-Wl,-rpath,{T.PKG}"], check=True)
    r = subprocess.run([exe, T.SCENE, ckpts["s0"][0], ckpts["s2"][0]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "policy slots caller ok" in r.stdout
