"""The manager's scene list and range list (csrc/manager.h) at the seams
between a single map, a map set and world groups: a list of one range is a
single map, the ray and geometry hooks answer for range 0's scene, and world
groups crossed with a residency switch, the workload counters and the camera
compute what one group computes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # before the engine initialises HIP

import camera_testlib as Cam
import geom_cases as G
import maps_testlib as M
import mpenv_testlib as T
import scene_residency_testlib as R
from test_geom_queries_gpu import LIDAR_RAY, Hook

pytestmark = pytest.mark.gpu


def outputs(e):
    out = {n: e.get(n) for n in M.COMPARED}
    out["EXPLORE"] = T.explore_visited(e)
    return out


def same_outputs(e, want, where):
    for n, a in want.items():
        T.compare(T.explore_visited(e) if n == "EXPLORE" else e.get(n), a, f"{n} @ {where}")


def header_reserved(e):
    """reserved[0..1] of a snapshot's StateHeader (engine.h: u32 words at bytes 48 and 52)"""
    blob = e.new_state_blob()
    e.state_save(blob)
    e.mem.hip.hipDeviceSynchronize()
    head = np.empty(256, np.uint8)
    e.mem.d2h(blob, 256, head)
    e.mem.free(blob)
    return tuple(int(x) for x in head[48:56].view(np.uint32))


def fnv1a64(data, h=1469598103934665603):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_a_one_range_list_is_a_single_map():
    """mpenv_create_maps([(simple_map, 5)]) against mpenv_create on the same
    directory, 3v3, the same seed and world_id_offset: every compared output
    and the explore grid bit-equal after init and after each of 20 steps under
    the captured graph; one map, described alike.  The snapshot header's
    reserved[0..1] stay as each kind of manager has them: zeros from
    mpenv_create, from a list the layout hash (FNV-1a 64 over the range's
    world count and its collisions.bin hash, as u64 bytes in little-endian
    order)."""
    W, ts, seed, off = 5, 3, 7, 3
    one = T.Engine(W, ts, rand_seed=seed, sim_flags=1, world_id_offset=off)
    lst = M.MapEngine([(T.SCENE, W)], ts, rand_seed=seed, sim_flags=1, world_id_offset=off)
    for e in (one, lst):
        e.put_ctrl([0, 1, 1])
        e.init()
    same_outputs(lst, outputs(one), "init")
    for s in range(20):
        acts = T.seek_combat_actions(one, s)
        for e in (one, lst):
            e.set_actions(acts)
            e.step()
        same_outputs(lst, outputs(one), f"step {s}")
    assert (one.graph_captures(), lst.graph_captures()) == (1, 1)
    assert one.graph_status()[0] == 1 and lst.graph_status()[0] == 1
    n = M.i32(-1)
    assert M.lib().mpenv_num_maps(one.h, C.byref(n)) == 0 and n.value == 1
    assert lst.num_maps() == 1
    info = M.MapEngine.map_info(one, 0)
    assert info == lst.map_info(0)
    assert info == dict(path=T.SCENE, first_world=0, num_worlds=W, scene=0, residency=M.LDS)
    h = fnv1a64(open(os.path.join(T.SCENE, "collisions.bin"), "rb").read())
    h = fnv1a64(W.to_bytes(8, "little") + h.to_bytes(8, "little"))
    assert h & 0xFFFFFFFF and h >> 32
    assert header_reserved(one) == (0, 0)
    assert header_reserved(lst) == (h & 0xFFFFFFFF, h >> 32)
    one.close()
    lst.close()


def oracle_rays(scene, org, d, order):
    """oracle_trace_ray_batch on `scene`: order 0 the collision tree in slot
    order, 1 the lidar tree in octant order."""
    o = M.Oracle(1, 1, scene=scene)
    t, h = np.zeros(len(org), np.float32), np.zeros(len(org), np.int32)
    o.lib.oracle_trace_ray_batch(o.h, len(org), T.fptr(org), T.fptr(d), order, T.fptr(t), h.ctypes.data)
    o.close()
    return t, h


def differing(a, b):
    """rays the two (t, hit) answers tell apart: by the hit, or by t where both hit"""
    (ta, ha), (tb, hb) = a, b
    return (ha != hb) | ((ha == 1) & (hb == 1) & (ta.view(np.uint32) != tb.view(np.uint32)))


def test_the_hooks_answer_for_range_0s_scene():
    """On the map set [B x 1, A x 1] mpenv_debug_trace_rays and the lidar-ray
    mode of mpenv_debug_geom_queries give what a single-map manager on B
    gives, bit for bit, over 48 rays of geom_cases: 16 the oracle answers
    differently on A and B on the collision tree, 16 on the lidar tree (the
    precondition, asserted on the CPU), and 16 it answers alike."""
    A, B = M.scene("A"), M.scene("B")
    org, d, _ = G.rays()
    # the first 30000 (the edge-aimed rays and the rollouts' lidar fans) hold all three kinds
    org, d = np.ascontiguousarray(org[:30000], np.float32), np.ascontiguousarray(d[:30000], np.float32)
    want = {order: {k: oracle_rays(p, org, d, order) for k, p in (("A", A), ("B", B))} for order in (0, 1)}
    dc, dl = (differing(want[order]["A"], want[order]["B"]) for order in (0, 1))
    pick = np.concatenate([np.flatnonzero(dc)[:16], np.flatnonzero(dl & ~dc)[:16], np.flatnonzero(~dc & ~dl)[:16]])
    assert dc[pick].sum() >= 1 and dl[pick].sum() >= 1 and len(pick) > 32, (dc.sum(), dl.sum())
    org, d = np.ascontiguousarray(org[pick]), np.ascontiguousarray(d[pick])
    n = len(pick)

    sims = {"set": M.MapEngine(M.ranges_of([("B", 1), ("A", 1)]), 1), "B": T.Engine(1, 1, scene=B),
            "A": T.Engine(1, 1, scene=A)}
    assert [sims["set"].map_info(r)["residency"] for r in (0, 1)] == [M.GLOBAL, M.LDS]
    od, dd = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    got = {}
    for k, e in sims.items():
        for mode in (0, 1):
            t = torch.zeros(n, dtype=torch.float32, device="cuda")
            h = torch.zeros(n, dtype=torch.int32, device="cuda")
            rc = e.lib.mpenv_debug_trace_rays(e.h, od.data_ptr(), dd.data_ptr(), n, mode, t.data_ptr(), h.data_ptr(), None)
            assert rc == 0, e.lib.mpenv_last_error().decode()
            got[k, "trace", mode] = (t.cpu().numpy(), h.cpu().numpy())
        r = Hook(e, o=org, d=d).run(LIDAR_RAY, n, dict(t=((n,), np.float32), i0=((n,), np.int32)))
        got[k, "lidar"] = (r["t"], r["i0"])
    for what in (("trace", 0), ("trace", 1), ("lidar",)):
        (t, h), (tb, hb), (ta, ha) = (got[(k,) + what] for k in ("set", "B", "A"))
        T.compare(h, hb, f"{what}: hit, map set against a manager on B")
        T.compare(t, tb, f"{what}: t, map set against a manager on B")
        assert differing((t, h), (ta, ha)).any(), f"{what}: the map set answers as a manager on A does"
        # and B's answers are the oracle's on B
        t_ref, h_ref = (a[pick] for a in want[0 if what[0] == "trace" else 1]["B"])
        T.compare(h, h_ref, f"{what}: hit, against the oracle on B")
        T.compare(t[h_ref == 1], t_ref[h_ref == 1], f"{what}: t, against the oracle on B")
    for e in sims.values():
        e.close()


def test_world_groups_cross_residency_stats_and_camera():
    """3v3 x 5 worlds on simple_map in 2 and then 3 world groups (5 divides by
    neither), the residency switched global -> lds in the middle of each,
    workload counters on and an 8 x 8 camera enabled: at every step the
    outputs and both images are bit-equal to a one-group twin's that switches
    alike, the counters equal the twin's, and every switch costs exactly one
    graph capture."""
    W, ts = 5, 3
    cfg = Cam.config(8, 8)
    grp, twin = T.Engine(W, ts, sim_flags=1), T.Engine(W, ts, sim_flags=1)
    for e in (grp, twin):
        assert Cam.enable(e, cfg) == 0, e.lib.mpenv_last_error().decode()
        e.enable_stats()
        e.put_ctrl([0, 1, 1])
    captures, step = 0, 0

    def run(steps):
        nonlocal step
        for _ in range(steps):
            acts = T.seek_combat_actions(twin, step)
            for e in (grp, twin):
                e.set_actions(acts)
                e.step()
            same_outputs(grp, outputs(twin), f"step {step}")
            Cam.check_images(grp, Cam.images(twin), f"step {step}")
            assert grp.read_stats() == twin.read_stats(), f"step {step}"
            assert (grp.graph_captures(), twin.graph_captures()) == (captures, captures), f"step {step}"
            step += 1

    for groups in (2, 3):
        grp.set_world_groups(groups)
        for mode in (R.GLOBAL, R.LDS):
            for e in (grp, twin):
                assert R.set_residency(e, mode) == 0, e.lib.mpenv_last_error().decode()
                assert R.residency(e) == mode
            if step == 0:
                for e in (grp, twin):
                    e.init()
                same_outputs(grp, outputs(twin), "init")
                Cam.check_images(grp, Cam.images(twin), "init")
            captures += 1
            run(4)
    assert captures == 4 and grp.read_stats()["alive_agents"] > 0
    grp.close()
    twin.close()
