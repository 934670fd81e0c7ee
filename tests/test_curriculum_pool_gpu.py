"""The live curriculum pool on the device (csrc/curriculum.hip k_harvest,
csrc/curriculum.cpp, include/mpenv_curriculum.h; DESIGN.md §2 definition 21).

W = 16 with team sizes 6 and 3, and a ragged case W = 3 with capacity 5.  What
episode starts read is pinned to the oracle opened with a curriculum file
(consumption) and to single-map managers (map set); what k_harvest writes is
pinned to the event log's PACKED_STEP_SNAPSHOT bytes and to the numpy
restatement of tests/curriculum_testlib.py fed the engine's own exports."""
import ctypes as C

import numpy as np
import pytest

import curriculum_testlib as CT
import maps_testlib as M
import mpenv_testlib as T
import policy_testlib as P
import posed_testlib as PT

pytestmark = pytest.mark.gpu

TAPE = 1234
EXPORTS = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS


def fresh(W=16, ts=6, ctrl=(0, 1, 1), **kw):
    e = T.Engine(W, ts, sim_flags=1, **kw)
    e.put_ctrl(list(ctrl))
    e.init()
    return e


def tape_step(e, k, first_world=0):
    e.set_actions(T.mpenv_tape.tape_actions(TAPE, k, first_world * e.N, e.W * e.N))
    e.step()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a.reshape(-1) != b.reshape(-1)))
        raise AssertionError(f"{what}: {len(bad)} of {a.size} differ, first at {bad[:8]}")


def harvest_checked(e, cfg, ranges, t, pool, ticks, offset=0):
    """After a step: the pool and ticks equal the restated harvest of tick t from (pool, ticks) and the
    engine's exports.  -> (pool, ticks, refreshed, candidates, state)"""
    st = CT.State(e)
    want_pool, want_ticks, refreshed, cands = CT.model_harvest(pool, ticks, st, cfg, t, ranges, offset)
    got_pool, got_ticks = CT.read(e)
    same(got_ticks, want_ticks, f"ticks @ tick {t}")
    same(got_pool, want_pool, f"pool @ tick {t}")
    assert CT.tick(e) == t
    return got_pool, got_ticks, refreshed, cands, st


def trigger(sims, s, W, first_world=0):
    """The reset schedule of test_curriculum_data_matches_oracle at step s, by global world"""
    if s % 10 == 0:
        for w in range(W):
            if (s // 10 + first_world + w) % 4 == 0:
                for sim in sims:
                    if isinstance(sim, T.Oracle):
                        sim.view("RESET")[w] = 1
                    else:
                        sim.trigger_reset(w)


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("ts", [6, 3])
def test_episode_starts_read_the_pool_as_the_oracle_reads_its_file(tmp_path, ts):
    """The pool holds the file's 48 snapshots (pool_set, period 0): every export equals the oracle opened
    with that file over 200 steps of triggered resets.  Then both sides get another 48 snapshots -- the
    engine only in its pool, its creation file unchanged -- and stay equal: the resets read the pool."""
    W = 16
    path = T.make_curriculum_file(str(tmp_path / "curriculum.bin"), n=48)
    other = T.make_curriculum_file(str(tmp_path / "other.bin"), n=48, seed=8)
    snaps, snaps2 = CT.MC.from_file(path), CT.MC.from_file(other)
    assert snaps.tobytes() != snaps2.tobytes()
    e = T.Engine(W, ts, sim_flags=1, curriculum=path)  # the init's starts come from the file on both sides
    o = T.Oracle(W, ts, sim_flags=1, curriculum=path)
    for sim in (e, o):
        sim.put_ctrl([0, 1, 1])
        sim.init()
    assert CT.enable(e, CT.config(48, period=0)) == 0, CT.err()
    assert CT.pool_set(e, snaps) == 0, CT.err()
    got, ticks = CT.read(e)
    same(got[0], snaps, "pool after pool_set")
    assert (ticks == 0).all()
    M.compare_all(e, o, f"ts {ts} init")
    starts = 0
    keep = None
    for s in range(240):
        if s == 200:  # the second set: the oracle's table and the engine's pool, not its file
            keep = np.fromfile(other, np.uint8)
            o.lib.oracle_set_curriculum(o.h, keep.ctypes.data, 48)
            assert CT.pool_set(e, snaps2) == 0, CT.err()
        trigger((e, o), s, W)
        reset_now = [w for w in range(W) if s % 10 == 0 and (s // 10 + w) % 4 == 0]
        acts = T.combat_actions(o, s)
        e.set_actions(acts)
        o.set_actions(acts)
        e.step()
        o.step()
        if s % 5 == 0:
            M.compare_all(e, o, f"ts {ts} step {s}")
        else:
            for n in ("SELF_OBSERVATION", "REWARD", "HP", "DEBUG_WORLD_I32"):
                T.compare(e.get(n), o.get(n), f"{n} @ ts {ts} step {s}")
        if reset_now:  # on the oracle: worlds that started from a snapshot of the set in use
            st = CT.State(o)
            table = snaps if s < 200 else snaps2
            for w in reset_now:
                starts += any(CT.started_from(st.wi[w], st.af[w], st.hp[w], sn, 2 * ts) for sn in table)
    assert starts >= 1
    same(CT.read(e)[0][0], snaps2, "pool at the end (period 0: nothing harvested)")
    assert CT.tick(e) == 240
    e.close()
    o.close()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("W,ts,cap", [(16, 6, 64), (16, 3, 64), (3, 6, 5)])
def test_harvest_equals_the_event_log_bytes(tmp_path, W, ts, cap):
    e = fresh(W, ts, ctrl=(0, 0, 1), events=str(tmp_path))
    cfg = CT.config(cap, period=2, seed=3)
    # on the host model first: some slot refreshes and some does not
    model = [CT.ref_select(cfg.seed, 0, np.arange(cap), t, 2, 0, W)[0] for t in range(1, 21)]
    assert any(m.any() for m in model) and any((~m).any() for m in model)
    assert CT.enable(e, cfg) == 0, CT.err()
    pool, ticks = CT.read(e)
    written_slots = 0
    for k in range(20):
        t = k + 1
        before = pool.copy()
        tape_step(e, k)
        pool, ticks, refreshed, cands, st = harvest_checked(e, cfg, [(0, W)], t, pool, ticks)
        log = e.get("PACKED_STEP_SNAPSHOT").view(np.uint8).reshape(W, 192)
        logged = e.get("SNAPSHOT_WRITTEN").ravel()
        raw = pool.view(np.uint8).reshape(cap, 176)
        for s in range(cap):
            if ticks[0, s] == t:
                rc, ref, w = CT.select(cfg.seed, 0, 0, s, t, 2, 0, W)
                assert rc == 0 and ref == 1 and logged[w] == 1
                assert raw[s].tobytes() == log[w, 16:].tobytes(), (t, s, w)
                written_slots += 1
            else:
                assert pool[0, s].tobytes() == before[0, s].tobytes(), (t, s)
        # open window, no need: ticks is select alone
        same(ticks[0] == t, refreshed[0], f"ticks against select @ {t}")
    assert written_slots >= cap
    e.close()


# ---------------------------------------------------------------- 3
def test_filters_keep_the_pool_and_a_posed_capture_passes():
    W, ts, cap = 16, 3, 64
    e = fresh(W, ts, ctrl=(0, 0, 1))
    cfg = CT.config(cap, period=1, step_range=(500, 2999), seed=2)  # step_lo above every world's step
    assert CT.enable(e, cfg) == 0, CT.err()
    pool0, ticks0 = CT.read(e)
    for k in range(3):
        tape_step(e, k)
    assert CT.State(e).wi[:, CT.WI_CUR_STEP].max() < 500
    pool, ticks = CT.read(e)
    same(pool, pool0, "pool under a closed window")
    assert (ticks == 0).all() and CT.tick(e) == 3
    cfg = CT.config(cap, period=1, need=CT.NEED_CAPTURED, seed=2)
    assert CT.configure(e, cfg) == 0, CT.err()
    tape_step(e, 3)
    assert (CT.State(e).wi[:, CT.WI_CAPTURED] == 0).all()  # a fresh batch: nothing captured
    pool, ticks = CT.read(e)
    same(pool, pool0, "pool under NEED_CAPTURED on a fresh batch")
    assert (ticks == 0).all()
    # world 5: team 1 holds a zone nobody stands in, captured, its first agent alone at the zone's centre
    boxes = PT.nav()[2]
    xy = CT.State(e).af[5, :, 0:2]
    empty = [z for z in range(3) if not ((xy >= boxes[z, 0:2]) & (xy <= boxes[z, 3:5])).all(1).any()]
    zone = empty[0]
    x, y = PT.zone_point(zone, 0.5, 0.5, np.zeros(3, np.float32))
    row = [5 * e.N + ts]
    PT._pose_engine(e, {"captured": ([5], 1), "controlling": ([5], 1), "curZone": ([5], zone),
                        "px": (row, np.float32(x)), "py": (row, np.float32(y)),
                        "vx": (row, np.float32(0)), "vy": (row, np.float32(0))})
    tape_step(e, 4)
    st = CT.State(e)
    assert [w for w in range(W) if st.wi[w, CT.WI_CAPTURED]] == [5]
    pool, ticks, refreshed, cands, _ = harvest_checked(e, cfg, [(0, W)], 5, pool0, ticks0)
    hit = cands[0] == 5
    assert hit.any() and not hit.all()
    same(ticks[0] == 5, hit, "exactly the slots whose candidate is the captured world")
    assert (pool[0][hit]["controller"] == 1).all()
    same(pool[0][~hit], pool0[0][~hit], "the other slots")
    e.close()


# ---------------------------------------------------------------- 4
def closed_loop(seed, W=16, ts=6):
    e = fresh(W, ts)
    cfg = CT.config(8, period=1, seed=seed)
    assert CT.enable(e, cfg) == 0, CT.err()
    pool, ticks = CT.read(e)
    from_pool = 0
    for s in range(100):
        reset_now = [w for w in range(W) if s % 10 == 0 and (s // 10 + w) % 4 == 0]
        trigger((e,), s, W)
        before, tbefore = pool, ticks
        tape_step(e, s)
        pool, ticks = CT.read(e)
        if reset_now:
            st = CT.State(e)
            live = before[0][tbefore[0] > 0]
            for w in reset_now:
                from_pool += any(CT.started_from(st.wi[w], st.af[w], st.hp[w], sn, 2 * ts) for sn in live)
    out = {n: e.get(n) for n in EXPORTS}
    e.close()
    return pool, ticks, out, from_pool


def test_closed_loop_starts_from_harvested_states_and_is_reproducible():
    pool_a, ticks_a, out_a, from_pool = closed_loop(4)
    assert from_pool >= 1
    assert ticks_a.max() == 100
    pool_b, ticks_b, out_b, _ = closed_loop(4)
    same(pool_a, pool_b, "pool of two runs with one seed")
    same(ticks_a, ticks_b, "ticks of two runs with one seed")
    for n in EXPORTS:
        T.compare(out_a[n], out_b[n], f"{n} of two runs with one seed")
    pool_c, _, _, _ = closed_loop(5)
    assert pool_a.tobytes() != pool_c.tobytes()


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("W,ts,cap", [(16, 6, 20), (16, 3, 20), (3, 6, 5)])
def test_initial_fill_is_the_pack_of_world_s_mod_w(W, ts, cap):
    e = fresh(W, ts, ctrl=(0, 0, 1))
    for k in range(3):
        tape_step(e, k)
    st = CT.State(e)
    assert CT.enable(e, CT.config(cap, period=0)) == 0, CT.err()
    pool, ticks = CT.read(e)
    assert pool.shape == (1, cap) and (ticks == 0).all() and CT.tick(e) == 0
    for s in range(cap):
        rc, want = CT.pack(st.rows(s % W), ts)  # the host entry point, and its restatement
        assert rc == 0
        assert pool[0, s].tobytes() == want.tobytes() == st.pack(s % W).tobytes(), s
    assert (pool[0]["step"] == 2).all()  # curStep 3 is logged as step 2
    e.close()


def test_lifecycle_graph_captures_and_disable_restores_the_run():
    W, ts = 16, 3
    a, b = fresh(W, ts), fresh(W, ts)
    for k in range(2):
        for e in (a, b):
            tape_step(e, k)
    blob = a.new_state_blob()
    a.state_save(blob)
    a.mem.hip.hipDeviceSynchronize()
    c0 = a.graph_captures()
    assert c0 >= 1 and a.graph_status() == (1, "")
    assert CT.enable(a, CT.config(8, period=1, seed=1)) == 0, CT.err()
    assert CT.enabled(a)[0] == 1 and CT.enabled(a)[1].capacity == 8
    tape_step(a, 2)
    assert a.graph_captures() == c0 + 1
    for k in range(3, 13):
        tape_step(a, k)
    assert a.graph_captures() == c0 + 1 and a.graph_status() == (1, "")
    assert CT.read(a)[1].max() == 11
    assert CT.disable(a) == 0, CT.err()
    assert CT.enabled(a)[0] == 0 and CT.tensor(a, CT.POOL)[0] == CT.ERR_INVALID and "disabled" in CT.err()
    tape_step(a, 13)
    assert a.graph_captures() == c0 + 2 and a.graph_status() == (1, "")
    # both from the one saved state: a, which had a pool, and b, which never did
    for e in (a, b):
        e.state_load(blob)
        assert e.state_error() == 0
    for s in range(30):
        trigger((a, b), s, W)
        for e in (a, b):
            tape_step(e, 20 + s)
        for n in EXPORTS:
            T.compare(a.get(n), b.get(n), f"{n} after disable @ {s}")
    a.mem.free(blob)
    a.close()
    b.close()


def test_refusals_name_their_reason(tmp_path):
    e = T.Engine(3, 3, sim_flags=1)
    e.put_ctrl([0, 1, 1])
    assert CT.enable(e, CT.config(4)) == CT.ERR_INVALID and "mpenv_init" in CT.err()  # before an init
    e.init()
    for cfg, word in ((CT.config(0), "capacity"), (CT.config(4, step_range=(9, 8)), "step_lo"),
                      (CT.config(4, need=16), "need"), (CT.config(4, period=-2), "period")):
        assert CT.enable(e, cfg) == CT.ERR_INVALID and word in CT.err(), CT.err()
        assert CT.enabled(e)[0] == 0
    for call in (lambda: CT.tensor(e, CT.TICKS)[0], lambda: CT.configure(e, CT.config(4)),
                 lambda: CT.pool_set(e, np.zeros(1, CT.SNAPSHOT)),
                 lambda: CT.lib().mpenv_curriculum_pool_tick(e.h, C.byref(C.c_uint32()))):
        assert call() == CT.ERR_INVALID and "disabled" in CT.err()
    assert CT.enable(e, CT.config(5, period=1)) == 0, CT.err()
    ptr = CT.tensor(e, CT.POOL)[1]
    assert CT.enable(e, CT.config(-1)) == CT.ERR_INVALID  # a refused re-enable leaves the pool it had
    assert CT.enabled(e)[0] == 1 and CT.tensor(e, CT.POOL)[1] == ptr
    assert CT.configure(e, CT.config(6)) == CT.ERR_INVALID and "capacity" in CT.err()
    assert CT.tensor(e, 2)[0] == CT.ERR_INVALID
    bad = np.zeros(2, CT.SNAPSHOT)
    bad[1]["cur_zone"] = 200
    assert CT.pool_set(e, bad) == CT.ERR_INVALID and "zone" in CT.err()
    bad[1]["cur_zone"], bad[1]["controller"] = 0, 2
    assert CT.pool_set(e, bad) == CT.ERR_INVALID and "controller" in CT.err()
    assert CT.pool_set(e, np.zeros(2, CT.SNAPSHOT), first_slot=4) == CT.ERR_INVALID and "slots" in CT.err()
    assert CT.pool_set(e, np.zeros(1, CT.SNAPSHOT), map_range=1) == CT.ERR_INVALID and "range" in CT.err()
    # pool_set writes its slots and zeroes their ticks
    tape_step(e, 0)
    assert (CT.read(e)[1] == 1).all()
    one = np.zeros(2, CT.SNAPSHOT)
    one["step"] = 77
    assert CT.pool_set(e, one, first_slot=3) == 0, CT.err()
    pool, ticks = CT.read(e)
    assert list(ticks[0]) == [1, 1, 1, 0, 0] and list(pool[0]["step"][3:]) == [77, 77]
    e.close()
    # a replay manager
    rec = str(tmp_path / "rec.bin")
    r = T.Engine(3, 3, sim_flags=1, record=rec)
    r.put_ctrl([0, 1, 1])
    r.init()
    tape_step(r, 0)
    assert CT.enable(r, CT.config(4)) == 0, CT.err()  # allowed with record_log_path
    r.close()
    p = T.Engine(3, 3, sim_flags=1, replay=rec)
    p.put_ctrl([0, 1, 1])
    p.init()
    assert CT.enable(p, CT.config(4)) == CT.ERR_INVALID and "replay_log_path" in CT.err()
    p.close()


# ---------------------------------------------------------------- 6
def test_direct_gpu_stream_step_harvests_as_a_plain_step():
    import torch

    W, ts = 16, 3
    cfg = CT.config(12, period=1, seed=6)
    a = fresh(W, ts)
    b = T.Engine(W, ts, sim_flags=1)
    b.put_ctrl([0, 1, 1])
    stream = torch.cuda.Stream()
    sb = T.StreamBuffers(b, n_sets=1)
    torch.cuda.synchronize()
    b.gpu_stream_init(stream.cuda_stream, sb.arrs[0])
    stream.synchronize()
    for e in (a, b):
        assert CT.enable(e, cfg) == 0, CT.err()
    pool, ticks = CT.read(a)
    same(CT.read(b)[0], pool, "initial fill behind gpuStreamInit")
    for k in range(6):
        acts = T.mpenv_tape.tape_actions(TAPE, k, 0, W * a.N)
        a.set_actions(acts)
        a.step()
        sb.set_actions(0, acts)
        torch.cuda.synchronize()
        b.gpu_stream_step(stream.cuda_stream, sb.arrs[0])
        stream.synchronize()
        pool, ticks, _, _, _ = harvest_checked(a, cfg, [(0, W)], k + 1, pool, ticks)
        got_pool, got_ticks = CT.read(b)
        same(got_pool, pool, f"pool behind a direct gpuStreamStep @ {k}")
        same(got_ticks, ticks, f"ticks behind a direct gpuStreamStep @ {k}")
    a.close()
    b.close()


def test_with_a_policy_loaded_the_pool_refreshes(tmp_path):
    W, ts = 16, 6
    e = fresh(W, ts)
    d = tmp_path / "ckpt"
    P.write_checkpoint(d, 50)
    assert e.lib.mpenv_policy_load_slot(e.h, 0, str(d).encode()) == 0, CT.err()
    cfg = CT.config(16, period=2, seed=8)
    assert CT.enable(e, cfg) == 0, CT.err()
    pool, ticks = CT.read(e)
    for k in range(6):
        tape_step(e, k)
        pool, ticks, _, _, _ = harvest_checked(e, cfg, [(0, W)], k + 1, pool, ticks)
    assert (ticks > 0).any()
    e.close()


def test_world_groups_change_nothing():
    W, ts = 16, 3
    cfg = CT.config(8, period=1, seed=7)
    sims = [fresh(W, ts) for _ in range(3)]
    sims[1].set_world_groups(3)  # before the pool
    for e in sims:
        assert CT.enable(e, cfg) == 0, CT.err()
    sims[2].set_world_groups(3)  # behind it: the new groups read the pool too
    for s in range(40):
        trigger(sims, s, W)
        for e in sims:
            tape_step(e, s)
        if s % 10 in (0, 5):
            for e in sims[1:]:
                for n in EXPORTS:
                    T.compare(e.get(n), sims[0].get(n), f"{n} with world groups @ {s}")
                same(CT.read(e)[0], CT.read(sims[0])[0], f"pool with world groups @ {s}")
                same(CT.read(e)[1], CT.read(sims[0])[1], f"ticks with world groups @ {s}")
    for e in sims:
        e.close()


# ---------------------------------------------------------------- 7
def test_a_map_set_keeps_a_pool_per_range():
    ts, n = 3, 8
    dirs = [M.scene("A"), M.scene("C")]  # C: simple_map with its two spawn lists swapped
    cfg = CT.config(8, period=1, seed=12)
    ms = M.MapEngine([(dirs[0], n), (dirs[1], n)], ts, sim_flags=1)
    singles = [T.Engine(n, ts, sim_flags=1, scene=dirs[r], world_id_offset=r * n) for r in range(2)]
    for e in [ms] + singles:
        e.put_ctrl([0, 1, 1])
        e.init()
        assert CT.enable(e, cfg) == 0, CT.err()
    ranges = [(0, n), (n, n)]
    pool, ticks = CT.read(ms)
    assert pool.shape == (2, 8)
    starts = [0, 0]
    for s in range(40):
        trigger((ms,), s, 2 * n)
        for r in range(2):
            trigger((singles[r],), s, n, first_world=r * n)
        reset_now = [w for w in range(2 * n) if s % 10 == 0 and (s // 10 + w) % 4 == 0]
        before, tbefore = pool, ticks
        tape_step(ms, s)
        for r in range(2):
            tape_step(singles[r], s, first_world=r * n)
        # each range's slots hold only its own worlds: the restatement draws range r from [r * n, (r + 1) * n)
        pool, ticks, _, cands, st = harvest_checked(ms, cfg, ranges, s + 1, before, tbefore)
        assert ((cands[0] >= 0) & (cands[0] < n)).all() and ((cands[1] >= n) & (cands[1] < 2 * n)).all()
        for r in range(2):
            sp, stk = CT.read(singles[r])
            same(pool[r], sp[0], f"range {r}'s pool against the single-map manager @ {s}")
            same(ticks[r], stk[0], f"range {r}'s ticks against the single-map manager @ {s}")
            if s % 5 == 0:
                for name in EXPORTS:
                    full = ms.get(name)
                    rows = full.shape[0] // (2 * n) * n
                    T.compare(full[r * rows:(r + 1) * rows], singles[r].get(name), f"{name} of range {r} @ {s}")
        for w in reset_now:  # a start from a snapshot is one of the world's own range's row
            r = w // n
            own = any(CT.started_from(st.wi[w], st.af[w], st.hp[w], sn, 2 * ts) for sn in before[r])
            starts[r] += own
    assert starts[0] >= 1 and starts[1] >= 1
    assert pool[0].tobytes() != pool[1].tobytes()
    for e in [ms] + singles:
        e.close()


# ---------------------------------------------------------------- the Python surface
def test_python_surface(tmp_path):
    import torch

    import madrona_mp_env as m

    sim = m.SimManager(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=5, rand_seed=5, auto_reset=True,
                       sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone, team_size=2,
                       num_pbt_policies=0, policy_history_size=0, scene_path=T.SCENE)
    ctrl = sim.sim_control_tensor().to_torch()
    ctrl.copy_(torch.tensor([0, 1, 1], dtype=torch.int32, device=ctrl.device).view_as(ctrl))
    assert sim.curriculum_pool_config() is None
    with pytest.raises(RuntimeError, match="mpenv_init"):
        sim.enable_curriculum_pool(7)
    sim.init()
    with pytest.raises(RuntimeError, match="disabled"):
        sim.curriculum_pool()
    with pytest.raises(RuntimeError, match="capacity"):
        sim.enable_curriculum_pool(0)
    sim.enable_curriculum_pool(7, period=1, need=m.CURRICULUM_NEED_BOTH_ALIVE, seed=3)
    assert sim.curriculum_pool_config() == dict(capacity=7, period=1, step_range=(0, 2999), need=4, seed=3)
    pool, ticks = sim.curriculum_pool().to_torch(), sim.curriculum_pool_ticks().to_torch()
    assert pool.dtype == torch.uint8 and tuple(pool.shape) == (1, 7, 176)
    assert tuple(ticks.shape) == (1, 7) and sim.curriculum_pool_ticks().dtype == "uint32"
    sim.step()
    torch.cuda.synchronize()
    assert sim.curriculum_pool_tick() == 1 and int(ticks.cpu().numpy().astype(np.int64).max()) == 1  # zero-copy
    sim.configure_curriculum_pool(period=0, step_range=(10, 20))
    assert sim.curriculum_pool_config() == dict(capacity=7, period=0, step_range=(10, 20), need=4, seed=3)
    path = str(tmp_path / "pool.bin")
    assert CT.MC.to_file(pool.cpu().numpy(), path) == 7
    snaps = CT.MC.from_file(path)
    assert len(snaps) == 7 and CT.MC.describe(snaps, team_size=2)["living"][4] == 7
    steps = [int(v) for v in snaps["step"]]
    snaps["step"] = 9
    sim.curriculum_pool_set(snaps[:2], first_slot=5)
    torch.cuda.synchronize()
    got = pool.cpu().numpy().view(CT.SNAPSHOT).reshape(7)
    assert list(got["step"]) == steps[:5] + [9, 9]
    sim.disable_curriculum_pool()
    assert sim.curriculum_pool_config() is None
