"""World checkpoints (csrc/state.hip, include/mpenv.h mpenv_state_*) against
the oracle, bit for bit: rewind and replay, selective restore, forks across
world groups, the refusals (device-side and host-side) and the Python surface.

The oracle cannot rewind; it runs each shape once, forward, and its outputs
after init and after every step are recorded and shared by the tests.  The
shapes are the smallest at which the copies can go wrong: 8-B spans and a
2-byte visMask span (1v1), 24-B spans (3v3), 48-B spans and wide rows over
the mapped load's 512-B threshold (6v6), and world groups whose boundaries
the restored spans cross (6v6, W = 7, three groups)."""
import functools

import numpy as np
import pytest

import mpenv_testlib as T

pytestmark = pytest.mark.gpu

SEED = 1234
STEPS = 16
RESET_AT, RESET_WORLD = 3, 1
ERR_HEADER, ERR_MAP = 1, 2
# (team size, worlds, world groups)
SHAPES = [(1, 3, 1), (3, 5, 1), (6, 3, 1), (6, 7, 3)]
NAMES = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS + ["EXPLORE"]


def row_kinds(e):
    """{output name: rows per world}, from the snapshot's own section table
    (not guessed from shape[0]: with N = 2, A == 2 W)."""
    w, t, l = T.state_dims(e)
    per = {0: 2 * t, 1: 1, 2: 2}
    out = {}
    k = 0
    while True:
        sec = T.state_section(k, w, t, l)
        if sec is None:
            break
        out[sec["name"]] = per[sec["kind"]]
        k += 1
    # the debug exports are gathered from per-agent / per-world columns
    for n in ("DEBUG_AGENT_F32", "DEBUG_AGENT_I32", "EXPLORE"):
        out[n] = per[0]
    for n in ("DEBUG_WORLD_I32", "DEBUG_WORLD_F32", "DEBUG_CRUMBS"):
        out[n] = per[1]
    return out


def outputs(sim):
    out = {n: sim.get(n) for n in T.STEP_OUTPUTS + T.DEBUG_OUTPUTS}
    out["EXPLORE"] = T.explore_visited(sim)
    return out


def world_rows(arr, per_world, w):
    return arr[w * per_world:(w + 1) * per_world]


def compare_all(got, want, where):
    for n in NAMES:
        T.compare(got[n], want[n], f"{n} @ {where}")


def compare_worlds(got, want, kinds, pairs, where):
    """world d of `got` against world s of `want`, for (d, s) in pairs"""
    for n in NAMES:
        for d, s in pairs:
            T.compare(world_rows(got[n], kinds[n], d), world_rows(want[n], kinds[n], s),
                      f"{n} world {d} (oracle world {s}) @ {where}")


def tape(step, A):
    return T.mpenv_tape.tape_actions(SEED, step, 0, A)


@functools.lru_cache(maxsize=None)
def oracle_run(ts, W):
    """The oracle's outputs after init ("init") and after steps 0..STEPS-1,
    computed once per shape and never modified."""
    o = T.Oracle(W, ts)
    o.put_ctrl([0, 1, 1])
    o.init()
    rec = {"init": outputs(o)}
    for s in range(STEPS):
        if s == RESET_AT:
            o.view("RESET")[RESET_WORLD] = 1
        o.set_actions(tape(s, W * 2 * ts))
        o.step()
        rec[s] = outputs(o)
    o.close()
    for d in rec.values():
        for a in d.values():
            a.setflags(write=False)
    return rec


def engine_at(ts, W, groups, last_step, rec=None):
    """An engine that has run init and steps 0..last_step like oracle_run
    (compared at every step when rec is given)."""
    e = T.Engine(W, ts)
    if groups > 1:
        e.set_world_groups(groups)
    e.put_ctrl([0, 1, 1])
    e.init()
    for s in range(last_step + 1):
        if s == RESET_AT:
            e.trigger_reset(RESET_WORLD)
        e.set_actions(tape(s, W * 2 * ts))
        e.step()
        if rec is not None:
            compare_all(outputs(e), rec[s], f"step {s}")
    return e


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_rewind_and_replay_against_the_oracle(ts, W, groups):
    rec = oracle_run(ts, W)
    A = W * 2 * ts
    e = engine_at(ts, W, groups, 7, rec)
    before = (e.graph_captures(), e.graph_status()[0])
    blob = e.new_state_blob()
    e.state_save(blob)
    for s in range(8, STEPS):
        e.set_actions(tape(s, A))
        e.step()
        compare_all(outputs(e), rec[s], f"step {s}")
    e.state_load(blob)
    # no step in between: every export is what it was after step 7
    compare_all(outputs(e), rec[7], "directly after the load")
    for s in range(8, STEPS):
        e.set_actions(tape(s, A))
        e.step()
        compare_all(outputs(e), rec[s], f"replayed step {s}")
    assert e.state_error() == 0
    assert (e.graph_captures(), e.graph_status()[0]) == before and before[1] == 1 and before[0] >= 1
    e.mem.free(blob)
    e.close()


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_selective_restore_rewinds_some_worlds_and_keeps_the_rest(ts, W, groups):
    rec = oracle_run(ts, W)
    N = 2 * ts
    A = W * N
    e = engine_at(ts, W, groups, 5)
    kinds = row_kinds(e)
    blob = e.new_state_blob()
    e.state_save(blob)
    for s in range(6, 12):
        e.set_actions(tape(s, A))
        e.step()
    rewound = [w for w in range(W) if w % 2 == 0]
    kept = [w for w in range(W) if w % 2 == 1]
    wmap = np.full(W, -1, np.int32)
    wmap[rewound] = rewound
    dmap = e.mem.upload(wmap)
    e.state_load(blob, dmap)
    got = outputs(e)
    compare_worlds(got, rec[5], kinds, [(w, w) for w in rewound], "after the load, rewound")
    compare_worlds(got, rec[11], kinds, [(w, w) for w in kept], "after the load, kept")
    acts = tape(12, A)
    a6 = tape(6, A)
    for w in rewound:
        acts[w * N:(w + 1) * N] = a6[w * N:(w + 1) * N]
    e.set_actions(acts)
    e.step()
    got = outputs(e)
    compare_worlds(got, rec[6], kinds, [(w, w) for w in rewound], "one step on, rewound")
    compare_worlds(got, rec[12], kinds, [(w, w) for w in kept], "one step on, kept")
    assert e.state_error() == 0
    e.mem.free(dmap)
    e.mem.free(blob)
    e.close()


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_fork_continues_as_the_source_world_did(ts, W, groups):
    rec = oracle_run(ts, W)
    N = 2 * ts
    A = W * N
    first, last = 6, 11  # the six steps right after the save
    # forks: the last world from world 0 (different world groups when the
    # batch is split), and world 0 from world 2
    forks = [(W - 1, 0), (0, 2)]
    # precondition, from the oracle's record: no fork source ends an episode in the window
    ep_col = 11  # MPENV_DBG_WI_EPISODE_COUNTER
    for _, s in forks:
        for step in range(first, last + 1):
            assert not world_rows(rec[step]["DONE"], N, s).any(), (s, step)
            assert rec[step]["DEBUG_WORLD_I32"][s, ep_col] == rec[first - 1]["DEBUG_WORLD_I32"][s, ep_col], (s, step)
    e = engine_at(ts, W, groups, first - 1)
    kinds = row_kinds(e)
    blob = e.new_state_blob()
    e.state_save(blob)
    wmap = np.full(W, -1, np.int32)
    for d, s in forks:
        wmap[d] = s
    dmap = e.mem.upload(wmap)
    e.state_load(blob, dmap)
    source = {d: s for d, s in forks}
    pairs = [(d, source.get(d, d)) for d in range(W)]
    compare_worlds(outputs(e), rec[first - 1], kinds, pairs, "directly after the fork")
    for step in range(first, last + 1):
        t = tape(step, A)
        acts = t.copy()
        for d, s in forks:
            acts[d * N:(d + 1) * N] = t[s * N:(s + 1) * N]
        e.set_actions(acts)
        e.step()
        compare_worlds(outputs(e), rec[step], kinds, pairs, f"forked step {step}")
    assert e.state_error() == 0
    e.mem.free(dmap)
    e.mem.free(blob)
    e.close()


# World groups that start off a 4-agent boundary (tests/test_ragged_groups_gpu.py):
# group starts at agents 6 and 18 (3v3 x 5 in three groups) and 10 (5v5 x 3 in
# two), so a group's spans are 8 B off the 16-B alignment the whole batch has,
# and the forks cross such a boundary.
RAGGED = [(3, 5, 3), (5, 3, 2)]


@pytest.mark.parametrize("ts,W,groups", RAGGED)
@pytest.mark.parametrize("what", ["rewind", "fork"])
def test_checkpoints_under_misaligned_world_groups(what, ts, W, groups):
    starts = [W * i // groups * 2 * ts for i in range(1, groups)]
    assert any(g0 % 4 for g0 in starts), starts
    if what == "rewind":
        test_rewind_and_replay_against_the_oracle(ts, W, groups)
    else:
        test_fork_continues_as_the_source_world_did(ts, W, groups)


def test_refused_loads_write_nothing():
    ts, W = 3, 5
    e = engine_at(ts, W, 1, 3)
    blob = e.new_state_blob()
    e.state_save(blob)
    nbytes = e.state_bytes()
    for s in range(4, 7):
        e.set_actions(tape(s, W * 2 * ts))
        e.step()
    before = {n: e.get(n) for n in T.DEBUG_OUTPUTS}

    def refused(src, world_map, bit, what):
        e.state_load(src, world_map)  # the call itself succeeds: the check runs on the device
        assert e.state_error() == bit, what
        assert e.state_error() == 0, what
        for n in T.DEBUG_OUTPUTS:
            assert np.array_equal(e.get(n).view(np.uint8), before[n].view(np.uint8)), (what, n)

    host = np.empty(nbytes, np.uint8)
    e.mem.d2h(blob, nbytes, host)
    assert host[:4].tobytes() == b"MPS1"
    for byte in (0, 9, 33, 255):  # magic, W, total bytes, a reserved byte
        bad = host.copy()
        bad[byte] ^= 0x10
        dbad = e.mem.upload(bad)
        refused(dbad, None, ERR_HEADER, f"header byte {byte} flipped")
        e.mem.free(dbad)
    for other_ts, other_W, what in ((ts, 3, "another W"), (1, W, "another team size")):
        o = engine_at(other_ts, other_W, 1, 0)
        oblob = o.new_state_blob()
        o.state_save(oblob)
        o.mem.hip.hipDeviceSynchronize()
        refused(oblob, None, ERR_HEADER, what)
        ident = e.mem.upload(np.arange(W, dtype=np.int32))
        refused(oblob, ident, ERR_HEADER, what + ", mapped")
        e.mem.free(ident)
        o.mem.free(oblob)
        o.close()
    for entry, what in ((W, "map entry W"), (-2, "map entry -2")):
        wmap = np.arange(W, dtype=np.int32)
        wmap[W - 2] = entry
        dmap = e.mem.upload(wmap)
        refused(blob, dmap, ERR_MAP, what)
        e.mem.free(dmap)
    # the snapshot itself is still good
    e.state_load(blob)
    assert e.state_error() == 0
    T.compare(e.get("DEBUG_AGENT_F32"), oracle_run(ts, W)[3]["DEBUG_AGENT_F32"], "good load after the refusals")
    e.mem.free(blob)
    e.close()


def test_host_side_rejections_name_their_reason(tmp_path):
    lib = T.lib_mpenv()
    e = T.Engine(3, 1)
    e.init()
    blob = e.new_state_blob()

    def invalid(rc, word):
        assert rc == -1  # MPENV_ERR_INVALID
        assert word in lib.mpenv_last_error().decode(), lib.mpenv_last_error()

    invalid(lib.mpenv_state_save(None, blob, None), "null")
    invalid(lib.mpenv_state_save(e.h, None, None), "null")
    invalid(lib.mpenv_state_load(e.h, None, None, None), "null")
    invalid(lib.mpenv_state_bytes(e.h, None), "null")
    invalid(lib.mpenv_state_error(e.h, None), "null")
    invalid(lib.mpenv_state_save(e.h, blob + 4, None), "aligned")
    invalid(lib.mpenv_state_load(e.h, blob + 8, None, None), "aligned")
    invalid(lib.mpenv_state_load(e.h, blob, blob + 4, None), "aligned")
    # a buffer inside the manager's own allocations would alias live state
    invalid(lib.mpenv_state_load(e.h, e.desc("SELF_OBSERVATION")[0], None, None), "own allocations")
    assert e.state_error() == 0
    logged = T.Engine(3, 1, events=str(tmp_path))
    logged.init()
    invalid(lib.mpenv_state_save(logged.h, blob, None), "event_log_path")
    invalid(lib.mpenv_state_load(logged.h, blob, None, None), "event_log_path")
    logged.close()
    e.mem.free(blob)
    e.close()


def test_python_surface_round_trips_on_a_side_stream():
    import torch

    import madrona_mp_env as m
    import mpenv_state

    ts, W = 3, 5
    A = W * 2 * ts
    sim = m.SimManager(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=W, rand_seed=5,
                       auto_reset=True, sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone,
                       team_size=ts, num_pbt_policies=0, policy_history_size=0, scene_path=T.SCENE)
    ctrl = sim.sim_control_tensor().to_torch()
    ctrl.copy_(torch.tensor([0, 1, 1], dtype=torch.int32, device=ctrl.device).view_as(ctrl))
    torch.cuda.synchronize()
    sim.init()
    side = torch.cuda.Stream()
    ring = torch.from_numpy(T.mpenv_tape.tape_ring(SEED, 0, A, 8)).cuda()
    blob = torch.empty(sim.state_bytes(), dtype=torch.uint8, device="cuda")
    wmap = torch.tensor([0, -1, 2, -1, 1], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pos = sim.self_pos().to_torch()
    hp = sim.hp().to_torch()
    with torch.cuda.stream(side):
        for s in range(4):
            sim.copy_actions(ring[s].data_ptr(), side.cuda_stream)
            sim.step_async(side.cuda_stream)
        sim.save_state(blob.data_ptr(), side.cuda_stream)
        saved_pos, saved_hp = pos.clone(), hp.clone()
        for s in range(4, 8):
            sim.copy_actions(ring[s].data_ptr(), side.cuda_stream)
            sim.step_async(side.cuda_stream)
        moved = pos.clone()
        sim.load_state(blob.data_ptr(), stream=side.cuda_stream)
        restored = pos.clone()
        sim.load_state(blob.data_ptr(), wmap.data_ptr(), side.cuda_stream)
        forked = pos.clone()
    side.synchronize()
    assert sim.state_error() == 0
    assert not torch.equal(moved, saved_pos)
    assert torch.equal(restored, saved_pos)
    N = 2 * ts
    assert torch.equal(forked[4 * N:5 * N], saved_pos[1 * N:2 * N]) and torch.equal(forked[:N], saved_pos[:N])
    assert torch.equal(mpenv_state.view(blob, "SELF_POSITION"), saved_pos)
    assert torch.equal(mpenv_state.view(blob, "HP"), saved_hp)
    assert tuple(sim.state_dims())[:2] == (W, ts)
    assert mpenv_state.header(blob)["bytes"] == sim.state_bytes() == mpenv_state.total_bytes(sim)
    assert list(mpenv_state.sections(sim)) == list(mpenv_state.sections(tuple(sim.state_dims())))
