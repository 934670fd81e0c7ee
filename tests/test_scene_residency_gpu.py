"""Scene residency on the GPU (include/mpenv_scene_residency.h):
the global-resident instantiation of every kernel that walks a BVH, bit for
bit against the oracle -- simple_map forced GLOBAL beside an LDS-resident
twin, the pillar scenes the LDS path cannot hold (tests/big_scene.py), the ray
and geometry hooks query by query, switching between steps, and one crossing
with world checkpoints and gpuStreamStep."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # before the engine initialises HIP

import big_scene
import mpenv_testlib as T
import scene_residency_testlib as R
from test_geom_queries_gpu import CASTS, LIDAR_RAY, SIGHT, WORLD_RAY, Hook, sizes

pytestmark = pytest.mark.gpu

ALL = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS
SEED = 1234


def make_pair(scene, ts, W, residency=None, **kw):
    e = T.Engine(W, ts, sim_flags=1, scene=scene, **kw)
    if residency is not None:
        assert R.set_residency(e, residency) == 0, e.lib.mpenv_last_error().decode()
    o = T.Oracle(W, ts, sim_flags=1, scene=scene, **kw)
    for s in (e, o):
        s.put_ctrl([0, 1, 1])
        s.init()
    return e, o


def compare_all(e, o, where, names=ALL):
    for n in names:
        T.compare(e.get(n), o.get(n), f"{n} @ {where}")


def step_both(sims, o, s, reset_world=None):
    """One step of seek_combat_actions computed from the oracle's rows."""
    acts = T.seek_combat_actions(o, s, SEED)
    for sim in list(sims) + [o]:
        if reset_world is not None:
            if isinstance(sim, T.Oracle):
                sim.view("RESET")[reset_world] = 1
            else:
                sim.trigger_reset(reset_world)
        sim.set_actions(acts)
        sim.step()
    return acts


@pytest.mark.parametrize("ts,W", [(3, 5), (1, 2)])
def test_simple_map_forced_global_matches_oracle_and_lds_twin(ts, W):
    e, o = make_pair(T.SCENE, ts, W, R.GLOBAL)
    twin = T.Engine(W, ts, sim_flags=1)
    twin.put_ctrl([0, 1, 1])
    twin.init()
    assert R.residency(e) == R.GLOBAL and R.residency(twin) == R.LDS
    compare_all(e, o, "init")
    for s in range(40):
        step_both([e, twin], o, s)
        compare_all(e, o, f"step {s}")
        for n in ALL:
            T.compare(e.get(n), twin.get(n), f"{n} global vs LDS twin @ step {s}")
    assert o.get("DONE").shape[0] == W * 2 * ts
    for x in (e, twin, o):
        x.close()


def test_pillars_100_matches_oracle_with_resets():
    """6v6 x 3 worlds, 150 steps with auto-reset and a forced reset of world 1
    at step 50.  The parent commit refuses this scene at mpenv_create (more
    than 256 nodes)."""
    scene = R.pillars(100)
    rc, info = R.scene_info(scene)
    assert rc == 0 and info.collision_nodes > 256 and info.lidar_stack > 16
    e, o = make_pair(scene, 6, 3)
    assert R.residency(e) == R.GLOBAL
    compare_all(e, o, "init")
    hurt = 0
    for s in range(150):
        step_both([e], o, s, reset_world=1 if s == 50 else None)
        compare_all(e, o, f"step {s}")
        hurt += int((o.get("HP") < 100).sum())
    assert hurt > 100  # fights happened: the shots' world rays found agents behind and between the pillars
    e.close()
    o.close()


def test_pillars_40_matches_oracle():
    """2v2 x 4 worlds, 30 steps.  Under the LDS path's count limits, over its
    LDS budget (k_lidar would ask for 183,744 B): the parent commit creates
    this scene and cannot launch a step on it."""
    scene = R.pillars(40)
    rc, info = R.scene_info(scene)
    assert rc == 0 and info.collision_nodes <= 256 and info.lds_bytes_lidar > 64 * 1024
    e, o = make_pair(scene, 2, 4)
    assert R.residency(e) == R.GLOBAL
    compare_all(e, o, "init")
    for s in range(30):
        step_both([e], o, s)
        compare_all(e, o, f"step {s}")
    e.close()
    o.close()


# ------------------------------------------------------------ query by query

@pytest.fixture(scope="module")
def big():
    """(engine, oracle) on pillar_scene(n=100), 1v1 x 1 world; the oracle's
    geometry hooks do not depend on its state."""
    scene = R.pillars(100)
    e = T.Engine(1, 1, scene=scene)
    o = T.Oracle(1, 1, scene=scene)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    o.lib.oracle_trace_world_batch.argtypes = [C.c_void_p, C.c_int32, fp, fp, fp, C.c_int32, ip, fp, ip]
    o.scene = scene
    yield e, o
    e.close()
    o.close()


def big_rays(o, n_seeded=3000, lidar=False):
    verts = o.lverts if lidar else o.verts
    bounds = big_scene.read_collisions(os.path.join(o.scene, "collisions.bin"))["bounds"]
    so, sd = R.seeded_rays(n_seeded, 21, bounds)
    eo, ed = T.edge_aimed_rays(verts, 1, 22)
    return np.concatenate([eo, so]), np.concatenate([ed, sd])


def oracle_trace(o, org, d, order):
    n = len(org)
    t, h = np.zeros(n, np.float32), np.zeros(n, np.int32)
    o.lib.oracle_trace_ray_batch(o.h, n, T.fptr(np.ascontiguousarray(org)), T.fptr(np.ascontiguousarray(d)), order,
                                 T.fptr(t), h.ctypes.data)
    return t, h


def test_trace_rays_on_the_big_scene_match_oracle(big):
    e, o = big
    assert R.residency(e) == R.GLOBAL
    org, d = big_rays(o)
    n = len(org)
    t_ref, h_ref = oracle_trace(o, org, d, 0)
    od, dd = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    for mode in (0, 1):
        t = torch.zeros(n, dtype=torch.float32, device="cuda")
        h = torch.zeros(n, dtype=torch.int32, device="cuda")
        rc = e.lib.mpenv_debug_trace_rays(e.h, od.data_ptr(), dd.data_ptr(), n, mode, t.data_ptr(), h.data_ptr(), None)
        assert rc == 0, e.lib.mpenv_last_error().decode()
        T.compare(h.cpu().numpy(), h_ref, f"trace rays hit mode {mode}")
        T.compare(t.cpu().numpy()[h_ref == 1], t_ref[h_ref == 1], f"trace rays t mode {mode}")
    assert h_ref.sum() > 3000


def test_lidar_and_world_rays_and_sight_on_the_big_scene_match_oracle(big):
    e, o = big
    org, d = big_rays(o, lidar=True)
    n_all = len(org)
    t_ref, h_ref = oracle_trace(o, org, d, 1)  # octant order on the lidar tree
    hook = Hook(e, o=org, d=d)
    for n in sizes(n_all):
        r = hook.run(LIDAR_RAY, n, dict(t=((n_all,), np.float32), i0=((n_all,), np.int32)))
        T.compare(r["i0"][:n], h_ref[:n], f"lidar ray hit n={n}")
        T.compare(r["t"][:n], t_ref[:n], f"lidar ray t n={n}")
    # world rays and sight: capsules on the ray, before and behind the first triangle
    org, d = big_rays(o, 2000)
    n_all = len(org)
    t_tri, h_tri = oracle_trace(o, org, d, 0)
    rng = np.random.default_rng(5)
    N = 4
    along = np.where(h_tri == 1, t_tri, 500.0)[:, None] * rng.uniform(0.2, 1.6, (n_all, N))
    caps = (org[:, None, :] + d[:, None, :] * along[:, :, None] + rng.normal(0, 6.0, (n_all, N, 3))).astype(np.float32)
    caps[:, :, 2] -= 32.0  # capsule base below its middle
    caps = np.ascontiguousarray(caps)
    hit, t, ent = (np.zeros(n_all, np.int32), np.zeros(n_all, np.float32), np.zeros(n_all, np.int32))
    o.lib.oracle_trace_world_batch(o.h, n_all, T.fptr(org), T.fptr(d), T.fptr(caps), N,
                                   hit.ctypes.data_as(C.POINTER(C.c_int32)), T.fptr(t),
                                   ent.ctypes.data_as(C.POINTER(C.c_int32)))
    none = np.full(n_all, -1, np.int32)
    outs = dict(t=((n_all,), np.float32), i0=((n_all,), np.int32), i1=((n_all,), np.int32))
    hook = Hook(e, o=org, d=d, caps=caps, sel=none)
    for n in sizes(n_all):
        r = hook.run(WORLD_RAY, n, outs, num_caps=N)
        T.compare(r["i0"][:n], hit[:n], f"world ray hit n={n}")
        T.compare(r["t"][:n], t[:n], f"world ray t n={n}")
        T.compare(r["i1"][:n], ent[:n], f"world ray entity n={n}")
    assert (ent >= 0).sum() > 200 and ((ent < 0) & (hit == 1)).sum() > 200
    target = rng.integers(0, N, n_all).astype(np.int32)
    seen_ref = ((hit == 1) & (ent == target)).astype(np.int32)
    hook = Hook(e, o=org, d=d, caps=caps, sel=target)
    outs = dict(i0=((n_all,), np.int32))
    no_hint = np.full(n_all, 0xffff, np.uint16)
    for n in sizes(n_all):
        r = hook.run(SIGHT, n, outs, num_caps=N, sub=1)
        T.compare(r["i0"][:n], seen_ref[:n], f"visibleRayD n={n}")
        r = hook.run(SIGHT, n, outs, num_caps=N, sub=0, hint=no_hint)
        T.compare(r["i0"][:n], seen_ref[:n], f"sight n={n}")
    r2 = hook.run(SIGHT, n_all, outs, num_caps=N, sub=0, hint=r["hint"])  # fed the occluders it wrote
    T.compare(r2["i0"], seen_ref, "sight, second pass")
    assert (r["hint"] != no_hint).sum() > 200 and seen_ref.sum() > 50


def test_sphere_casts_on_the_big_scene_match_oracle(big):
    """CASTS subs 0-3 (bvhSphereCastD, castNearD, castNear2D, castFirstNearD)
    from origins a capsule could have: above the floor, inside the bounds."""
    e, o = big
    rng = np.random.default_rng(9)
    n_all = 6000
    b = big_scene.read_collisions(os.path.join(o.scene, "collisions.bin"))["bounds"]
    oh = rng.uniform([b[0] + 60, b[1] + 60, 10.0], [b[3] - 60, b[4] - 60, 60.0], (n_all, 3)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, n_all)
    dh = np.stack([np.cos(ang), np.sin(ang), np.zeros(n_all)], 1).astype(np.float32)
    bh = rng.uniform(5.0, 400.0, n_all).astype(np.float32)
    z1 = (oh[:, 2] + rng.uniform(5.0, 40.0, n_all)).astype(np.float32)
    act1 = rng.integers(0, 2, n_all).astype(np.int32)

    def casts(org, d):
        t, nrm = np.zeros(len(org), np.float32), np.zeros((len(org), 3), np.float32)
        o.lib.oracle_sphere_cast_batch(o.h, len(org), T.fptr(np.ascontiguousarray(org)),
                                       T.fptr(np.ascontiguousarray(d)), 15.0, None, T.fptr(t), T.fptr(nrm))
        return t, nrm

    def check_near(t, nrm, t_ref, n_ref, B, name):
        near = t_ref < B
        T.compare(t[near], t_ref[near], name + " t")
        T.compare(nrm[near], n_ref[near], name + " normal")
        assert (t[~near] >= B[~near]).all(), name
        return int(near.sum())

    t_ref, n_ref = casts(oh, dh)
    o1 = oh.copy()
    o1[:, 2] = z1
    t_ref1, n_ref1 = casts(o1, dh)
    outs1 = dict(t=((n_all,), np.float32), normal=((n_all, 3), np.float32))
    outs2 = dict(t=((n_all, 2), np.float32), normal=((n_all, 2, 3), np.float32))
    hook = Hook(e, o=oh, d=dh, bound=bh, z1=z1, sel=act1)
    compared = 0
    for n in sizes(n_all):
        r = hook.run(CASTS, n, outs1, sub=0)
        T.compare(r["t"][:n], t_ref[:n], f"full cast t n={n}")
        hit = t_ref[:n] < 3.0e38
        T.compare(r["normal"][:n][hit], n_ref[:n][hit], f"full cast normal n={n}")
        r1 = hook.run(CASTS, n, outs1, sub=1)
        compared = check_near(r1["t"][:n], r1["normal"][:n], t_ref[:n], n_ref[:n], bh[:n], f"castNearD n={n}")
        r2 = hook.run(CASTS, n, outs2, sub=2)
        T.compare(r2["t"][:n, 0], r1["t"][:n], f"castNear2D low t n={n}")
        T.compare(r2["normal"][:n, 0], r1["normal"][:n], f"castNear2D low normal n={n}")
    on = act1 == 1
    compared += check_near(r2["t"][on, 1], r2["normal"][on, 1], t_ref1[on], n_ref1[on], bh[on], "castNear2D high")
    dv = np.tile(np.array([0, 0, -1], np.float32), (n_all, 1))
    bv = rng.uniform(20.0, 120.0, n_all).astype(np.float32)
    tv_ref, _ = casts(oh, dv)
    hv = Hook(e, o=oh, d=dv, bound=bv)
    for n in sizes(n_all):
        r = hv.run(CASTS, n, dict(t=((n_all,), np.float32)), sub=3)
        T.compare(r["t"][:n], tv_ref[:n], f"castFirstNearD n={n}")
    assert compared > 500 and (t_ref < 3.0e38).sum() > 3000


# ------------------------------------------------------------ switching

def test_switching_residency_between_steps():
    ts, W = 2, 3
    e, o = make_pair(T.SCENE, ts, W)
    twin = T.Engine(W, ts, sim_flags=1)
    twin.put_ctrl([0, 1, 1])
    twin.init()
    assert R.residency(e) == R.LDS
    caps = []
    for s in range(12):
        if s == 6:
            assert R.set_residency(e, R.GLOBAL) == 0
            assert R.residency(e) == R.GLOBAL
        step_both([e, twin], o, s)
        caps.append(e.graph_captures())
        for n in ALL:
            T.compare(e.get(n), twin.get(n), f"{n} switched vs unswitched twin @ step {s}")
        compare_all(e, o, f"step {s}")
    assert caps[0] >= 1 and len(set(caps[:6])) == 1 and len(set(caps[6:])) == 1, caps
    assert caps[6] == caps[5] + 1, caps  # exactly one more capture
    assert twin.graph_captures() == caps[0]
    assert R.set_residency(e, 7) == R.ERR_INVALID and R.residency(e) == R.GLOBAL
    for x in (e, twin, o):
        x.close()
    # LDS on a scene that does not fit: refused, nothing changes, the next step still matches
    e, o = make_pair(R.pillars(100), ts, W)
    step_both([e], o, 0)
    c0 = e.graph_captures()
    assert R.set_residency(e, R.LDS) == R.ERR_INVALID
    msg = e.lib.mpenv_last_error().decode()
    assert "does not fit" in msg and "nodes" in msg, msg
    assert R.residency(e) == R.GLOBAL
    step_both([e], o, 1)
    compare_all(e, o, "step after the refused switch")
    assert e.graph_captures() == c0
    assert R.set_residency(e, R.AUTO) == 0 and R.residency(e) == R.GLOBAL
    e.close()
    o.close()


# ------------------------------------------------------------ one crossing

def test_checkpoints_and_stream_step_on_the_big_scene():
    """state_save at step 10, on to step 20, state_load of worlds {0, 2}:
    they repeat steps 11-20 bit for bit while worlds 1 and 3 go on; then one
    direct gpuStreamStep fills the caller's buffers with what the plain step
    gives (the oracle's rows)."""
    ts, W = 3, 4
    N = 2 * ts
    e, o = make_pair(R.pillars(100), ts, W)
    stream = torch.cuda.Stream()
    blob = e.new_state_blob()
    rec, acts = {}, {}
    for s in range(21):
        acts[s] = step_both([e], o, s)
        compare_all(e, o, f"step {s}")
        rec[s] = {n: e.get(n) for n in ALL}
        if s == 10:
            e.state_save(blob)
    wmap = np.array([0, -1, 2, -1], np.int32)
    mp = e.mem.upload(wmap)
    e.state_load(blob, mp)
    assert e.state_error() == 0
    rows = {w: slice(w * N, (w + 1) * N) for w in range(W)}
    for s in range(11, 21):
        e.set_actions(acts[s])  # worlds 1 and 3 get some actions too; only 0 and 2 are compared
        e.step()
        for n in ("SELF_OBSERVATION", "HP", "FWD_LIDAR", "REAR_LIDAR", "REWARD", "OPPONENT_MASKS", "SELF_POSITION",
                  "DEBUG_AGENT_F32", "DEBUG_AGENT_I32"):
            got = e.get(n)
            for w in (0, 2):
                T.compare(got[rows[w]], rec[s][n][rows[w]], f"{n} world {w} replayed step {s}")
    e.mem.free(mp)
    e.mem.free(blob)
    e.close()
    # the stream step, on a fresh engine in step with the oracle
    e = T.Engine(W, ts, sim_flags=1, scene=R.pillars(100))
    e.put_ctrl([0, 1, 1])
    sb = T.StreamBuffers(e)
    torch.cuda.synchronize()
    e.gpu_stream_init(stream.cuda_stream, sb.arrs[0])
    stream.synchronize()
    o2 = T.Oracle(W, ts, sim_flags=1, scene=R.pillars(100))
    o2.put_ctrl([0, 1, 1])
    o2.init()
    for s in range(3):
        a = T.seek_combat_actions(o2, s, SEED)
        o2.set_actions(a)
        o2.step()
        if s < 2:
            e.set_actions(a)
            e.step()
            continue
        sb.set_actions(1, a)
        sb.put(1, "resets", np.zeros(W, np.int32))
        torch.cuda.synchronize()
        e.gpu_stream_step(stream.cuda_stream, sb.arrs[1])
        stream.synchronize()
    for (io, nm, ename, _, _), b in zip(sb.ti, sb.sets[1]):
        if io == 1 and "agent_map" not in nm:
            T.compare(b.cpu().numpy(), o2.get(ename), f"caller's {ename} after a direct stream step")
    for x in (e, o, o2):
        x.close()
