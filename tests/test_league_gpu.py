"""k_league on the device (csrc/league.hip, include/mpenv_league.h; DESIGN.md §2
definition 20) against the numpy restatement in league_testlib, exactly.

W = 70 (two waves of worlds, the second a ragged tail of six), team size 2,
P = 3, five steps each.  Episode ends are posed through a snapshot
(league_testlib.pose_ends): curStep = 2998 - w % 3 ends 24, 23 and 23 worlds
in steps 2, 3 and 4 of the five, with all three outcomes among them.  The
restatement is fed the engine's own DONE / MATCH_RESULT exports of each step
and the AGENT_POLICY column as it stood in front of the step."""
import numpy as np
import pytest

import league_testlib as L
import maps_testlib as M
import mpenv_testlib as T
import policy_slots_abi
import policy_testlib as P

pytestmark = pytest.mark.gpu

SEED = 9
# non-uniform, with a zero row (1: a home team of id 1 keeps its opponent) and clamped entries
WEIGHTS = np.array([[5, 0, 1], [0, 0, 0], [1, 70000, -3], [2, 1, 4]], np.int32)


def plain(W=L.W, **kw):
    return T.Engine(W, L.TEAM, **kw)


def two_maps(**kw):
    return M.MapEngine([(T.SCENE, 40), (T.SCENE, 30)], L.TEAM, **kw)


def start(make, mode, weights=None, offset=0, seed=SEED):
    """An engine with the league on, initialised: (engine, restatement), the init's draws checked."""
    e = make(world_id_offset=offset) if offset else make()
    e.put_ctrl([0, 1, 1])
    assert L.enable(e, L.config(L.P, mode, seed)) == 0, L.err()
    ref = L.Ref(L.P, mode, seed, e.W, L.TEAM, offset)
    L.check(e, ref, "enable")
    if weights is not None:
        assert L.set_weights(e, weights) == 0, L.err()
        ref.weights = np.array(weights, np.int32)
    before = e.get("AGENT_POLICY")
    e.init()
    L.check(e, ref, "init", policy=ref.visit(None, None, before, init=True))
    return e, ref


def run_steps(e, ref, steps=L.STEPS, first_world=0, step=None):
    """`steps` tape steps, the league checked after each: [worlds ended per step]"""
    ended = []
    for k in range(steps):
        before = e.get("AGENT_POLICY")
        (step or L.tape_step)(e, k, first_world)
        done, mr = e.get("DONE"), e.get("MATCH_RESULT")
        fin = done.reshape(e.W, e.N)[:, 0] == 1
        assert (done.reshape(e.W, e.N) == fin[:, None]).all()  # every agent of a world shares done
        want = ref.visit(done, mr, before)
        L.check(e, ref, f"step {k + 1}", policy=want)
        # worlds that did not end are untouched
        T.compare(want.reshape(e.W, -1)[~fin], before.reshape(e.W, -1)[~fin], f"ids of running worlds @ step {k + 1}")
        ended.append(int(fin.sum()))
    return ended


def standings(make):
    e, ref = start(make, L.NONE)
    ids = L.standings_ids()
    L.pose_ends(e, ids)
    cells = {(L.ref_bucket(L.ref_team_id(p[0]), L.P), L.ref_bucket(L.ref_team_id(p[1]), L.P))
             for p in ids.reshape(L.W, 2, L.TEAM)[64:]}
    assert len(cells) >= 5 and len({tuple(p.reshape(-1)) for p in ids.reshape(L.W, 2, L.TEAM)[:64]}) == 1
    ended = run_steps(e, ref)
    assert ended == [0, 24, 23, 23, 0], ended
    table = L.read(e, L.TABLE)
    assert table[..., 0].sum() == 70 and (table[..., 1:4].sum(axis=(0, 1)) > 0).all()  # every outcome occurred
    assert table[1, 2, 0] == 64 and not L.read(e, L.DRAWS).any()
    assert L.clear(e) == 0
    assert not L.read(e, L.TABLE).any()
    e.close()


def draws(make, mode):
    e, ref = start(make, mode, WEIGHTS)
    assert (ref.draws == 1).all()
    # homes over every row: 0, 1 (the zero row), 2, external (-1), mixed, out of range
    home = np.array([[0, 0], [1, 1], [2, 2], [-1, -1], [0, 2], [7, 7]], np.int32)
    ids = np.zeros((L.W, 2, L.TEAM), np.int32)
    ids[:, 0] = home[np.arange(L.W) % len(home)]
    ids[:, 1] = (np.arange(L.W) % 3)[:, None]
    L.pose_ends(e, ids.reshape(-1))
    first = e.get("AGENT_POLICY").reshape(L.W, 2, L.TEAM)
    assert sum(run_steps(e, ref)) == 70 and (ref.draws == 2).all()
    last = e.get("AGENT_POLICY").reshape(L.W, 2, L.TEAM)
    if mode == L.TEAM1:
        T.compare(last[:, 0], first[:, 0], "team 0 under DRAW_TEAM1")
        zero_row = np.arange(L.W) % len(home) == 1
        T.compare(last[zero_row, 1], first[zero_row, 1], "team 1 against a home team whose row is all zero")
        assert (last[~zero_row, 1] != first[~zero_row, 1]).any()
    else:
        assert (last[:, 0] == last[:, 0, :1]).all() and ((last[:, 0] >= 0) & (last[:, 0] < L.P)).all()
    e.close()


# ---------------------------------------------------------------- 1, 2, 3
def test_standings_match_the_accumulation():
    standings(plain)


def test_one_cell_takes_every_world_in_one_step():
    e, ref = start(plain, L.NONE)
    L.pose_ends(e, np.tile(np.array([2, 2, 0, 0], np.int32), L.W), cur_step=2998)
    assert run_steps(e, ref, steps=3) == [0, 70, 0]
    table = L.read(e, L.TABLE)
    assert table[2, 0, 0] == 70 and table[..., 0].sum() == 70
    e.close()


@pytest.mark.parametrize("mode", [L.TEAM1, L.BOTH])
def test_draws_match_the_restatement(mode):
    draws(plain, mode)


# ---------------------------------------------------------------- 4
def test_the_step_is_untouched():
    names = T.DEBUG_OUTPUTS + list(T.TRAIN_OUTPUTS.values()) + ["AGENT_POLICY"]
    on, off = plain(), plain()
    for e in (on, off):
        e.put_ctrl([0, 1, 1])
    assert L.enable(on, L.config(L.P, L.NONE, SEED)) == 0
    for e in (on, off):
        e.init()
        L.pose_ends(e, L.standings_ids())
    for k in range(L.STEPS):
        for e in (on, off):
            L.tape_step(e, k)
        for n in names:
            T.compare(on.get(n), off.get(n), f"{n} @ step {k + 1}: league on against off")
        if k == 2:
            assert L.read(on, L.TABLE)[..., 0].sum() == 47
            assert L.disable(on) == 0 and L.enabled(on)[0] == 0
    assert on.graph_captures() == off.graph_captures() >= 1
    # enabling again never re-captures
    c0 = on.graph_captures()
    assert L.enable(on, L.config(L.P, L.TEAM1, SEED)) == 0
    L.tape_step(on, L.STEPS)
    assert on.graph_captures() == c0
    on.close()
    off.close()


# ---------------------------------------------------------------- 5
def test_two_shards_draw_and_record_what_the_whole_run_does():
    ids = np.zeros((L.W, 2, L.TEAM), np.int32)
    ids[:, 0] = (np.arange(L.W) % 4 - 1)[:, None]
    ids[:, 1] = (np.arange(L.W) % 3)[:, None]
    whole, ref = start(plain, L.TEAM1, WEIGHTS)
    L.pose_ends(whole, ids.reshape(-1))
    run_steps(whole, ref)
    pol, table = [], np.zeros_like(ref.table)
    for off in (0, 35):
        e, r = start(lambda **kw: plain(35, **kw), L.TEAM1, WEIGHTS, offset=off)
        L.pose_ends(e, ids[off:off + 35].reshape(-1), first_world=off)
        run_steps(e, r, first_world=off)
        pol.append(e.get("AGENT_POLICY"))
        table += L.read(e, L.TABLE)
        e.close()
    T.compare(np.concatenate(pol), whole.get("AGENT_POLICY"), "AGENT_POLICY: two shards against the whole run")
    T.compare(table, L.read(whole, L.TABLE), "the shards' tables summed against the whole run's")
    assert table[..., 0].sum() == 70
    whole.close()


# ---------------------------------------------------------------- 6
def test_redrawn_agents_play_their_new_checkpoint(tmp_path):
    e, ref = start(plain, L.BOTH, np.array([[1, 2, 3], [3, 2, 1], [1, 1, 1], [2, 1, 2]], np.int32))
    policy_slots_abi.bind(e.lib)
    for slot in range(3):
        d = tmp_path / f"ckpt{slot}"
        P.write_checkpoint(d, 50 + slot)
        assert e.lib.mpenv_policy_load_slot(e.h, slot, str(d).encode()) == 0, L.err()
    A = e.W * e.N
    L.pose_ends(e, (np.arange(L.W) % 3).repeat(2 * L.TEAM))
    ac_d = e.mem.upload(np.zeros((A, 6), np.int32))
    lg_d = e.mem.upload(np.zeros((A, P.LOGITS), np.float32))
    checked, redrawn = 0, np.zeros(A, bool)
    for k in range(L.STEPS):
        before = e.get("AGENT_POLICY")
        assert ((before >= 0) & (before < 3)).all()
        # what each agent's current id plays: every slot's actions for every agent, picked by id
        want = np.zeros((A, 6), np.int32)
        for slot in range(3):
            assert e.lib.mpenv_policy_forward_slot(e.h, slot, lg_d, ac_d, None) == 0, L.err()
            e.mem.hip.hipDeviceSynchronize()
            acts = np.empty((A, 6), np.int32)
            e.mem.d2h(ac_d, acts.nbytes, acts)
            sel = before.reshape(-1) == slot
            want[sel] = acts[sel]
        L.tape_step(e, k)
        played = np.concatenate([e.get("PVP_DISCRETE_ACTION"), e.get("PVP_DISCRETE_AIM_ACTION")], axis=1)
        # the agents re-drawn behind the previous step played their new checkpoint's actions
        T.compare(played[redrawn], want[redrawn], f"actions of the agents re-drawn in step {k}")
        checked += int(redrawn.sum())
        now = ref.visit(e.get("DONE"), e.get("MATCH_RESULT"), before)
        T.compare(e.get("AGENT_POLICY"), now, f"AGENT_POLICY @ step {k + 1}")
        redrawn = np.repeat(e.get("DONE").reshape(e.W, e.N)[:, 0] == 1, e.N)
    assert checked == 70 * e.N
    assert (e.get("AGENT_POLICY") != (np.arange(L.W) % 3).repeat(2 * L.TEAM).reshape(-1, 1)).any()
    e.mem.free(ac_d)
    e.mem.free(lg_d)
    e.close()


# ---------------------------------------------------------------- 7
def test_a_map_set_is_one_launch_over_the_batch():
    standings(two_maps)
    draws(two_maps, L.TEAM1)


# ---------------------------------------------------------------- 8
def test_direct_gpu_stream_step_records():
    import torch

    e, ref = start(plain, L.NONE)
    ids = L.standings_ids()
    stream = torch.cuda.Stream()
    sb = T.StreamBuffers(e, n_sets=1)
    sb.put(0, "pbt.policy_assignments", ids.reshape(-1, 1))
    torch.cuda.synchronize()
    e.gpu_stream_init(stream.cuda_stream, sb.arrs[0])
    stream.synchronize()
    L.check(e, ref, "gpuStreamInit")
    L.pose_ends(e, ids)

    def step(e, k, first_world):
        sb.set_actions(0, T.mpenv_tape.tape_actions(L.TAPE_SEED, k, 0, e.W * e.N))
        torch.cuda.synchronize()
        e.gpu_stream_step(stream.cuda_stream, sb.arrs[0])
        stream.synchronize()

    assert run_steps(e, ref, steps=2, step=step) == [0, 24]
    assert L.read(e, L.TABLE)[..., 0].sum() == 24
    e.close()


# ---------------------------------------------------------------- 9
def test_refusals_leave_the_manager_as_it_was():
    e = plain(3)
    e.put_ctrl([0, 1, 1])
    e.init()
    for cfg, needle in ((L.config(0), "num_policies"), (L.config(33), "num_policies"), (L.config(3, 3), "draw"),
                        (L.config(3, -1), "draw")):
        assert L.enable(e, cfg) == L.ERR_INVALID and needle in L.err()
        assert L.enabled(e)[0] == 0
    for call in (lambda: L.tensor(e, L.TABLE)[0], lambda: L.clear(e), lambda: L.set_weights(e, np.ones((4, 3)))):
        assert call() == L.ERR_INVALID and "disabled" in L.err()
    assert L.enable(e, L.config(3, L.BOTH, 5)) == 0
    table, draws_ = L.read(e, L.TABLE), L.read(e, L.DRAWS)
    ptr = L.tensor(e, L.TABLE)[1]
    # a refused re-enable leaves the league it had
    assert L.enable(e, L.config(40, L.BOTH, 5)) == L.ERR_INVALID
    on, cfg = L.enabled(e)
    assert (on, cfg.num_policies, cfg.draw, cfg.seed) == (1, 3, L.BOTH, 5) and L.tensor(e, L.TABLE)[1] == ptr
    T.compare(L.read(e, L.TABLE), table, "table after a refused enable")
    T.compare(L.read(e, L.DRAWS), draws_, "draws after a refused enable")
    assert L.tensor(e, 3)[0] == L.ERR_INVALID
    for which, dt, shape in ((L.TABLE, L.DTYPE_I64, (4, 4, 8)), (L.WEIGHTS, L.DTYPE_I32, (4, 3)), (L.DRAWS, L.DTYPE_U32, (3,))):
        assert L.tensor(e, which)[2:] == (dt, shape)
    e.close()
    # no auto_reset: refused whatever the mode
    e = plain(3, auto_reset=False)
    assert L.enable(e, L.config(3, L.NONE)) == L.ERR_INVALID and "auto_reset" in L.err()
    assert L.enabled(e)[0] == 0
    e.close()
    # sub-zones: standings only
    e = plain(3, sim_flags=L.SIMFLAG_SUB_ZONES)
    for mode in (L.TEAM1, L.BOTH):
        assert L.enable(e, L.config(3, mode)) == L.ERR_INVALID and "SUB_ZONES" in L.err()
        assert L.enabled(e)[0] == 0
    assert L.enable(e, L.config(3, L.NONE)) == 0
    e.close()


def test_python_surface():
    import torch

    import madrona_mp_env as m

    sim = m.SimManager(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=5, rand_seed=5, auto_reset=True,
                       sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone, team_size=2,
                       num_pbt_policies=0, policy_history_size=0, scene_path=T.SCENE)
    ctrl = sim.sim_control_tensor().to_torch()
    ctrl.copy_(torch.tensor([0, 1, 1], dtype=torch.int32, device=ctrl.device).view_as(ctrl))
    assert sim.league_config() is None
    with pytest.raises(RuntimeError, match="disabled"):
        sim.league_table()
    with pytest.raises(RuntimeError, match="num_policies"):
        sim.enable_league(33)
    sim.enable_league(3, draw="both", seed=4)
    assert sim.league_config() == (3, "both", 4)
    table, weights = sim.league_table().to_torch(), sim.league_weights().to_torch()
    assert table.dtype == torch.int64 and tuple(table.shape) == (4, 4, 8) and sim.league_table().dtype == "int64"
    assert weights.dtype == torch.int32 and tuple(weights.shape) == (4, 3) and bool((weights == 1).all())
    assert tuple(sim.league_draws().shape) == (5,)
    weights[3] = torch.tensor([0, 0, 9], dtype=torch.int32)  # zero-copy: team 0 always draws 2
    weights[2] = torch.tensor([0, 7, 0], dtype=torch.int32)  # and team 1, against 2, always 1
    torch.cuda.synchronize()
    sim.init()
    pol = sim.policy_assignment_tensor().to_torch().cpu().numpy().reshape(5, 2, 2)
    assert (pol[:, 0] == 2).all() and (pol[:, 1] == 1).all()
    for w in range(5):
        got = m.league_draw(3, "both", 4, w, 0, np.zeros((2, 2), np.int32), weights.cpu().numpy())
        assert (np.asarray(got) == pol[w]).all()
    assert int(table.sum()) == 0
    table += 1
    sim.clear_league()
    torch.cuda.synchronize()
    assert int(table.sum()) == 0
    sim.set_league_weights(np.ones((4, 3), np.int32))
    assert bool((weights == 1).all())
    sim.disable_league()
    assert sim.league_config() is None
