"""Map sets on the GPU (include/mpenv_maps.h; DESIGN.md §2 definition 19): a
manager from mpenv_create_maps against one oracle per range, bit for bit.

Every world of range r must compute what an oracle on that range's directory
computes with n_r worlds and world_id_offset advanced by the range's first
world.  Shapes: the smallest that put a range's first agent off
the 4-agent lidar unit and its first world on an odd id, with every kind of
scene difference (geometry B, spawns C, zones D, navmesh E), mixed residency,
a scene shared by two non-adjacent ranges, and an aligned control.

Each parity shape first asserts its own precondition from oracles alone: for
every range and every other scene of its set, oracles on the range's scene and
on the other one, over the range's own worlds and offset, differ in a compared
output by step 5 -- otherwise a range given the wrong scene would pass.  The
seed of a shape is the first from 5 up at which that holds (5 is the test
libraries' default): with SpawnInMiddle (sim_flags 1) a world draws per episode,
with probability 1/2, whether everyone spawns from the middle cells, which are
computed from the collision mesh and so are the same on A and C; at seed 5
worlds 4 and 5, the 3v3 shape's range on A, both draw them and never touch the
exchanged lists in 60 steps, and world 0 of the 5v5 shape does not tell E from A."""
import ctypes as C
import functools

import numpy as np
import pytest

import camera_testlib as Cam
import maps_testlib as M
import mpenv_testlib as T
import policy_testlib as P
import scene_residency_testlib as R

pytestmark = pytest.mark.gpu

STEPS = 60
SIM_FLAGS = 1
# name -> (team size, [(map, worlds)], manager world_id_offset, team 1 as A* bots, rand_seed)
SHAPES = {
    "3v3": (3, [("A", 2), ("B", 3), ("C", 1), ("D", 2)], 4, False, 10),
    "1v1": (1, [("B", 1), ("A", 1), ("B", 1)], 0, False, 5),
    "5v5": (5, [("A", 1), ("E", 2), ("B", 2)], 0, True, 6),
    "6v6": (6, [("A", 2), ("B", 1)], 0, False, 5),
}


def bot_policy(W, ts):
    pol = np.zeros((W, 2 * ts), np.int32)
    pol[:, ts:] = -1
    return pol.reshape(-1, 1)


def outputs(sim):
    out = {n: sim.get(n) for n in M.COMPARED}
    out["EXPLORE"] = sim.explore() if isinstance(sim, M.RangeOracles) else T.explore_visited(sim)
    return out


def compare_all(got, want, where):
    for n in want:
        T.compare(got[n], want[n], f"{n} @ {where}")


@functools.lru_cache(maxsize=None)
def record(shape, steps=STEPS):
    """The range oracles' outputs after init ("init") and after steps
    0..steps-1 and the actions they played, once per shape, never modified."""
    ts, spec, off, bots, seed = SHAPES[shape]
    o = M.RangeOracles(M.ranges_of(spec), ts, world_id_offset=off, sim_flags=SIM_FLAGS, rand_seed=seed)
    o.put_ctrl([0, 1, 1])
    if bots:
        o.set_policy(bot_policy(o.W, ts))
    o.init()
    rec, acts = {"init": outputs(o)}, []
    for s in range(steps):
        acts.append(o.seek_actions(s))
        o.step()
        rec[s] = outputs(o)
    o.close()
    for d in rec.values():
        for a in d.values():
            a.setflags(write=False)
    return rec, acts


@functools.lru_cache(maxsize=None)
def precondition(shape):
    """Every range tells its scene from every other scene of the shape: oracles
    on the two, over the range's own worlds and offset, differ in a compared
    output by step 5."""
    ts, spec, off, bots, seed = SHAPES[shape]
    kinds = sorted({k for k, _ in spec})
    w0 = 0
    for k, n in spec:
        for other in kinds:
            if other != k:
                by = M.scenes_differ_by(M.scene(other), M.scene(k), ts, n, off + w0, bots=bots, sim_flags=SIM_FLAGS,
                                        rand_seed=seed)
                assert by is not None, f"{shape}: worlds [{w0}, {w0 + n}) compute the same on {k} and {other} for 5 steps"
        w0 += n
    return True


def engine(shape):
    ts, spec, off, bots, seed = SHAPES[shape]
    e = M.MapEngine(M.ranges_of(spec), ts, world_id_offset=off, sim_flags=SIM_FLAGS, rand_seed=seed)
    e.put_ctrl([0, 1, 1])
    if bots:
        e.put("AGENT_POLICY", bot_policy(e.W, ts))
    return e


def engine_at(shape, last_step, rec=None):
    """An engine after init and steps 0..last_step on the record's actions."""
    _, acts = record(shape)
    e = engine(shape)
    e.init()
    if rec is not None:
        compare_all(outputs(e), rec["init"], "init")
    for s in range(last_step + 1):
        e.set_actions(acts[s])
        e.step()
        if rec is not None:
            compare_all(outputs(e), rec[s], f"step {s}")
    return e


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "direct"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_range_equals_its_own_oracle(shape, graph, monkeypatch):
    assert precondition(shape)
    if not graph:
        monkeypatch.setenv("MPENV_STEP_GRAPH", "0")
    rec, _ = record(shape)
    ts, spec, off, _, _ = SHAPES[shape]
    e = engine_at(shape, STEPS - 1, rec)
    assert e.graph_captures() == (1 if graph else 0)
    assert e.graph_status()[0] == (1 if graph else 0)
    # the ranges as the engine holds them
    assert e.num_maps() == len(spec)
    w0, scenes = 0, {}
    for r, (k, n) in enumerate(spec):
        info = e.map_info(r)
        assert (info["path"], info["first_world"], info["num_worlds"]) == (M.scene(k), w0, n)
        assert info["scene"] == scenes.setdefault(k, len(scenes))
        assert (e.map_of_world()[w0:w0 + n] == r).all()
        w0 += n
    e.close()


def test_two_ranges_on_one_map_equal_a_single_map_manager():
    ts, W = 3, 5
    a = M.MapEngine([(T.SCENE, 2), (T.SCENE, 3)], ts, sim_flags=SIM_FLAGS)
    b = T.Engine(W, ts, sim_flags=SIM_FLAGS)
    # a single-map manager: one range over the batch, a table of zeros made on first use
    n, d, path, tab = C.c_int32(-1), M.MapDesc(), C.c_char_p(), C.c_void_p()
    assert b.lib.mpenv_num_maps(b.h, C.byref(n)) == 0 and n.value == 1
    assert b.lib.mpenv_map_info(b.h, 0, C.byref(d), C.byref(path)) == 0
    assert (d.first_world, d.num_worlds, d.scene, d.residency, path.value.decode()) == (0, W, 0, M.LDS, T.SCENE)
    assert b.lib.mpenv_map_info(b.h, 1, C.byref(d), None) == M.ERR_INVALID
    for _ in range(2):
        assert b.lib.mpenv_map_of_world(b.h, C.byref(tab)) == 0
        zeros = np.full(W, -1, np.int32)
        b.mem.d2h(tab.value, zeros.nbytes, zeros)
        assert not zeros.any()
    assert (a.map_of_world() == [0, 0, 1, 1, 1]).all()
    for e in (a, b):
        e.put_ctrl([0, 1, 1])
        e.init()
    compare_all(outputs(a), outputs(b), "init")
    for s in range(30):
        acts = T.seek_combat_actions(b, s)
        for e in (a, b):
            e.set_actions(acts)
            e.step()
        compare_all(outputs(a), outputs(b), f"step {s}")
    assert a.state_bytes() == b.state_bytes()
    a.close()
    b.close()


def test_residency_is_per_map_and_switches_for_all():
    rec, acts = record("3v3")
    e = engine_at("3v3", 9, rec)
    B = M.scene("B")

    def in_use():
        return [e.map_info(r)["residency"] for r in range(e.num_maps())]

    assert in_use() == [M.LDS, M.GLOBAL, M.LDS, M.LDS]
    assert e.graph_captures() == 1
    assert R.set_residency(e, R.GLOBAL) == 0
    assert in_use() == [M.GLOBAL] * 4
    for s in range(10, 20):
        e.set_actions(acts[s])
        e.step()
        compare_all(outputs(e), rec[s], f"global-resident step {s}")
    assert e.graph_captures() == 2
    assert R.set_residency(e, R.LDS) == M.ERR_INVALID
    msg = e.lib.mpenv_last_error().decode()
    assert "map range 1" in msg and B in msg and "k_lidar" in msg, msg
    assert in_use() == [M.GLOBAL] * 4  # nothing changed
    mode = C.c_int32(-7)
    assert R.lib().mpenv_scene_residency(e.h, C.byref(mode)) == M.ERR_INVALID and mode.value == -7
    assert "mpenv_map_info" in e.lib.mpenv_last_error().decode()
    assert R.set_residency(e, R.AUTO) == 0
    assert in_use() == [M.LDS, M.GLOBAL, M.LDS, M.LDS]
    for s in range(20, 25):
        e.set_actions(acts[s])
        e.step()
        compare_all(outputs(e), rec[s], f"step {s} back on auto")
    assert e.graph_captures() == 3
    e.close()


def test_gpu_stream_step_over_a_map_set():
    import torch

    rec, acts = record("3v3")
    e = engine("3v3")
    sb = T.StreamBuffers(e)
    stream = torch.cuda.Stream()
    e.gpu_stream_init(stream.cuda_stream, sb.arrs[0])
    stream.synchronize()

    def check(bufs, want, where):
        for (io, nm, ename, _, _), b in zip(sb.ti, bufs):
            if io == 1 and ename in want:
                T.compare(b.cpu().numpy(), want[ename], f"{nm} @ {where}")

    check(sb.sets[0], rec["init"], "init")
    caps = []
    for s in range(20):
        sb.set_actions(s % 2, acts[s])
        torch.cuda.synchronize()
        e.gpu_stream_step(stream.cuda_stream, sb.arrs[s % 2])
        stream.synchronize()
        check(sb.sets[s % 2], rec[s], f"step {s}")
        caps.append(e.graph_captures())
    assert caps[0] == 1 and caps[-1] == 1, caps
    # a plain step afterwards writes the engine's own exports again
    e.set_actions(acts[20])
    e.step()
    compare_all(outputs(e), rec[20], "plain step after the stream steps")
    e.close()


# ------------------------------------------------------------------ checkpoints
def world_rows(arr, W, N, w):
    per = {W * N: N, W: 1, 2 * W: 2}[arr.shape[0]]
    return arr[w * per:(w + 1) * per]


def test_rewind_and_replay_over_a_map_set():
    rec, acts = record("3v3")
    e = engine_at("3v3", 9)
    blob = e.new_state_blob()
    e.state_save(blob)
    for s in range(10, 20):
        e.set_actions(acts[s])
        e.step()
    compare_all(outputs(e), rec[19], "step 19")
    e.state_load(blob)
    compare_all(outputs(e), rec[9], "directly after the load")
    for s in range(10, 20):
        e.set_actions(acts[s])
        e.step()
        compare_all(outputs(e), rec[s], f"replayed step {s}")
    assert e.state_error() == 0 and e.graph_captures() == 1
    e.mem.free(blob)
    e.close()


def test_fork_inside_a_scene_and_refusal_across_scenes():
    rec, acts = record("3v3")
    ts, spec, _, _, _ = SHAPES["3v3"]
    N, W = 2 * ts, sum(n for _, n in spec)
    src, dst = 2, 3  # both in B's range [2, 5)
    first = 10
    # the window: until the source world ends an episode (its reset), from the record
    ep_col = 11  # MPENV_DBG_WI_EPISODE_COUNTER
    last = first
    while (last + 1 < STEPS and not world_rows(rec[last]["DONE"], W, N, src).any()
           and rec[last]["DEBUG_WORLD_I32"][src, ep_col] == rec[first - 1]["DEBUG_WORLD_I32"][src, ep_col]):
        last += 1
    assert last - first >= 5, "the source world resets too early for the fork to show anything"
    e = engine_at("3v3", first - 1)
    blob = e.new_state_blob()
    e.state_save(blob)
    wmap = np.full(W, -1, np.int32)
    wmap[dst] = src
    dmap = e.mem.upload(wmap)
    e.state_load(blob, dmap)
    assert e.state_error() == 0
    pairs = [(w, src if w == dst else w) for w in range(W)]

    def compare_worlds(got, want, where):
        for n in want:
            for d, s in pairs:
                T.compare(world_rows(got[n], W, N, d), world_rows(want[n], W, N, s), f"{n} world {d} <- {s} @ {where}")

    compare_worlds(outputs(e), rec[first - 1], "directly after the fork")
    for s in range(first, last):
        a = acts[s].copy()
        a[dst * N:(dst + 1) * N] = acts[s][src * N:(src + 1) * N]
        e.set_actions(a)
        e.step()
        compare_worlds(outputs(e), rec[s], f"forked step {s}")
    # world 0 (map A) from snapshot world 2 (map B): refused, nothing written
    before = {n: e.get(n) for n in T.DEBUG_OUTPUTS + ["SELF_OBSERVATION", "FWD_LIDAR"]}
    wmap[:] = -1
    wmap[0] = 2
    e.mem.h2d(dmap, wmap)
    e.state_load(blob, dmap)
    assert e.state_error() == M.STATE_ERR_CROSS_MAP
    for n, a in before.items():
        assert e.get(n).tobytes() == a.tobytes(), n
    # out of range and across scenes at once: both bits
    wmap[1] = W
    e.mem.h2d(dmap, wmap)
    e.state_load(blob, dmap)
    assert e.state_error() == M.STATE_ERR_CROSS_MAP | M.STATE_ERR_MAP
    # world 7 (D) from world 6 (D, the same range): fine; world 5 (C) from world 0 (A): the same
    # collisions.bin, another scene directory -- refused
    wmap[:] = -1
    wmap[7] = 6
    e.mem.h2d(dmap, wmap)
    e.state_load(blob, dmap)
    assert e.state_error() == 0
    wmap[5] = 0
    e.mem.h2d(dmap, wmap)
    e.state_load(blob, dmap)
    assert e.state_error() == M.STATE_ERR_CROSS_MAP
    e.mem.free(dmap)
    e.mem.free(blob)
    e.close()


def test_a_snapshot_of_another_range_layout_is_refused():
    ts, spec, off, _, seed = SHAPES["3v3"]
    e = engine_at("3v3", 2)
    other = M.MapEngine(M.ranges_of([("A", 3), ("B", 2), ("C", 1), ("D", 2)]), ts, world_id_offset=off,
                        sim_flags=SIM_FLAGS)
    other.put_ctrl([0, 1, 1])
    other.init()
    assert other.state_bytes() == e.state_bytes() and T.state_dims(other) == T.state_dims(e)
    blob = other.new_state_blob()
    other.state_save(blob)
    before = {n: e.get(n) for n in T.DEBUG_OUTPUTS}
    e.state_load(blob)
    assert e.state_error() == M.STATE_ERR_HEADER
    for n, a in before.items():
        assert e.get(n).tobytes() == a.tobytes(), n
    # and its own snapshot is taken
    e.state_save(blob)
    e.state_load(blob)
    assert e.state_error() == 0
    # a single-map manager's header words stay zero
    hdr = np.empty(64, np.uint32)
    single = T.Engine(8, ts, sim_flags=SIM_FLAGS)
    sblob = single.new_state_blob()
    single.state_save(sblob)
    single.mem.hip.hipDeviceSynchronize()
    single.mem.d2h(sblob, hdr.nbytes, hdr)
    assert not hdr[12:].any()
    e.mem.hip.hipDeviceSynchronize()
    e.mem.d2h(blob, hdr.nbytes, hdr)
    assert hdr[12:14].any() and not hdr[14:].any()
    single.mem.free(sblob)
    single.close()
    other.mem.free(blob)
    other.close()
    e.close()


# ----------------------------------------------------------------------- camera
def test_camera_renders_each_range_against_its_own_scene():
    rec, acts = record("3v3")
    ts, spec, _, _, _ = SHAPES["3v3"]
    N = 2 * ts
    cfg = Cam.config(16, 8)

    def expected(state):
        af, ai = state["DEBUG_AGENT_F32"], state["DEBUG_AGENT_I32"]
        parts, a0 = [], 0
        for k, n in spec:
            sl = slice(a0, a0 + n * N)
            parts.append(Cam.expected(cfg, af[sl, 0:3].copy(), af[sl, 12:16].copy(), ai[sl, 0].copy(), N,
                                      scene=M.scene(k)))
            a0 += n * N
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def on_map_a(state):
        return Cam.expected(cfg, state["DEBUG_AGENT_F32"][:, 0:3].copy(), state["DEBUG_AGENT_F32"][:, 12:16].copy(),
                            state["DEBUG_AGENT_I32"][:, 0].copy(), N, scene=M.scene("A"))

    e = engine_at("3v3", 19)
    assert Cam.enable(e, cfg) == 0
    assert Cam.render(e) == 0
    exp19 = expected(rec[19])
    # the precondition, from the oracle alone: B's boxes are in view, so a range rendered against
    # range 0's scene would differ
    assert not np.array_equal(exp19[0].view(np.uint32), on_map_a(rec[19])[0].view(np.uint32))
    Cam.check_images(e, exp19, "rendered after step 19")
    blob = e.new_state_blob()
    e.state_save(blob)
    # behind a step
    e.set_actions(acts[20])
    e.step()
    exp20 = expected(rec[20])
    assert not np.array_equal(exp20[0].view(np.uint32), on_map_a(rec[20])[0].view(np.uint32))
    Cam.check_images(e, exp20, "behind step 20")
    e.state_load(blob)
    assert Cam.render(e) == 0
    Cam.check_images(e, exp19, "rendered after the load")
    e.mem.free(blob)
    e.close()


# ----------------------------------------------------------------------- policy
def test_policy_plays_team_0_as_in_single_map_managers(tmp_path):
    d = tmp_path / "ckpt"
    P.write_checkpoint(d, 21)
    ts, n = 3, 2
    N = 2 * ts
    kinds = ["A", "B"]
    m = M.MapEngine(M.ranges_of([(k, n) for k in kinds]), ts, sim_flags=SIM_FLAGS)
    singles = [T.Engine(n, ts, sim_flags=SIM_FLAGS, scene=M.scene(k), world_id_offset=r * n) for r, k in enumerate(kinds)]
    ids = np.zeros((n, N), np.int32)
    ids[:, ts:] = -2  # team 1 keeps the tape's actions
    for e in [m] + singles:
        e.put_ctrl([0, 1, 1])
        e.put("AGENT_POLICY", np.resize(ids.reshape(-1, 1), (e.W * N, 1)))
        e.init()
        assert e.lib.mpenv_policy_load(e.h, str(d).encode()) == 0, e.lib.mpenv_last_error().decode()
    pol = np.resize(ids.reshape(-1) >= 0, m.W * N)
    played_differs = False
    for s in range(20):
        tape = T.mpenv_tape.tape_actions(1234, s, 0, m.W * N)
        m.set_actions(tape)
        m.step()
        for r, e in enumerate(singles):
            e.set_actions(tape[r * n * N:(r + 1) * n * N])
            e.step()
        want = {nm: np.concatenate([e.get(nm) for e in singles]) for nm in M.COMPARED}
        compare_all(outputs(m), want, f"step {s}")
        played = np.concatenate([m.get("PVP_DISCRETE_ACTION"), m.get("PVP_DISCRETE_AIM_ACTION")], axis=1)
        played_differs |= not np.array_equal(played[pol], tape[pol])
    assert played_differs, "the policy never played an action of its own"
    for e in [m] + singles:
        e.close()


# -------------------------------------------------------------------- refusals
def test_refused_calls_leave_the_manager_stepping(tmp_path):
    rec, acts = record("3v3")
    e = engine_at("3v3", 4, rec)
    lib = e.lib

    def unsupported(rc, *needles):
        msg = lib.mpenv_last_error().decode()
        assert rc == M.ERR_UNSUPPORTED and "map-set manager" in msg, (rc, msg)
        for nd in needles:
            assert nd in msg, msg

    unsupported(lib.mpenv_set_world_groups(e.h, 2), "mpenv_set_world_groups")
    assert lib.mpenv_set_world_groups(e.h, 1) == 0
    unsupported(lib.mpenv_set_lidar_branch(e.h, 1), "mpenv_set_lidar_branch")
    nbytes = C.c_int64(-1)
    unsupported(lib.mpenv_wire_bytes(e.h, 1, C.byref(nbytes)), "mpenv_wire_bytes", "gather")
    assert nbytes.value == -1
    buf = e.mem.upload(np.zeros(64, np.uint8))
    unsupported(lib.mpenv_wire_pack(e.h, buf, 1, None), "mpenv_wire_pack")
    unsupported(lib.mpenv_wire_unpack(e.h, buf, 1, None), "mpenv_wire_unpack")
    e.mem.free(buf)
    ts, spec, off, _, seed = SHAPES["3v3"]
    for key in ("replay", "record", "events", "curriculum"):
        rc, h, msg = M.create(M.ranges_of(spec), ts, **{key: str(tmp_path / key)})
        assert rc == M.ERR_UNSUPPORTED and h is None and "one map" in msg, (key, rc, msg)
    for s in range(5, 10):
        e.set_actions(acts[s])
        e.step()
        compare_all(outputs(e), rec[s], f"step {s} after the refusals")
    assert e.graph_captures() == 1
    e.close()


def test_stats_timings_and_setters_over_a_map_set():
    """enable_stats shares its one buffer over the ranges, kernel_timings sums
    each kernel over them, and trigger_reset, set_hp, copy_actions and the
    device aim-bot address worlds and agents of the whole batch."""
    rec, acts = record("3v3")
    ts, spec, _, _, _ = SHAPES["3v3"]
    N = 2 * ts
    e = engine_at("3v3", 2)
    # copy_actions and the device aim-bot (mode 1 = seek_combat_actions) in place of set_actions
    for s in range(3, 6):
        tape = np.concatenate([T.mpenv_tape.tape_actions(1234, s, 0, n * N) for _, n in spec])
        dev = e.mem.upload(tape)
        e.combat_actions(dev, None, 1)
        e.mem.hip.hipDeviceSynchronize()
        e.mem.free(dev)
        e.step()
        compare_all(outputs(e), rec[s], f"aim-bot step {s}")
    e.enable_stats(True)
    e.lib.mpenv_enable_kernel_timing(e.h, 1)
    dev = e.mem.upload(acts[6])
    e.copy_actions(dev)
    e.step()
    e.mem.free(dev)
    compare_all(outputs(e), rec[6], "timed step 6")
    stats = e.read_stats()
    alive = int((rec[5]["ALIVE"] != 0).sum())
    assert stats["alive_agents"] == alive, (stats, alive)
    names, ms, launches = (C.c_char_p * 8)(), (C.c_float * 8)(), (C.c_int32 * 8)()
    assert e.lib.mpenv_kernel_timings(e.h, 8, names, ms, launches) == 5
    assert list(launches)[:5] == [1] * 5 and all(v > 0 for v in list(ms)[:5])
    e.lib.mpenv_enable_kernel_timing(e.h, 0)
    e.enable_stats(False)
    # a reset of world 3 (B) and a set_hp in world 6 (D) land in those worlds only
    e.trigger_reset(3)
    e.set_hp(6, 1, 37)
    assert e.get("HP")[6 * N + 1, 0] == 37 and e.get("RESET")[3, 0] == 1 and e.get("RESET").sum() == 1
    e.close()
