"""k_lidar's octant node images without their back-facing triangles (scene.h
octantNodeImages with prune, DESIGN.md section 2 definition 16), on the
device: the LIDAR_RAY hook of mpenv_debug_geom_queries walks the uploaded
(pruned) images with k_lidar's traversal, and its hit and t equal the oracle's
octant order over the full tree bit for bit on the adversarial ray sets of
tests/lidar_backface_cases.py; whole steps give the oracle's lidar exports and
every other step output byte for byte."""
import os
import sys

import numpy as np
import pytest

import lidar_backface_cases as B
import mpenv_testlib as T
from test_geom_queries_gpu import LIDAR_RAY, Hook, sizes

sys.path.insert(0, os.path.join(T.ROOT, "tools"))
from dump_lidar_rays import rays_for  # noqa: E402

pytestmark = pytest.mark.gpu


def _fans():
    """Lidar fans after 16 tape steps and after 16 more under the aim-bot."""
    o = T.Oracle(2, 6)
    o.put_ctrl([0, 1, 1])
    o.init()
    out = []
    for s in range(32):
        o.set_actions(T.seek_combat_actions(o, s) if s >= 16 else T.mpenv_tape.tape_actions(1234, s, 0, o.W * 12))
        o.step()
        if s % 16 == 15:
            out.append(rays_for(o.get("DEBUG_AGENT_F32"), o.get("DEBUG_AGENT_I32")))
    o.close()
    r = np.concatenate(out)
    return r[:, :3].astype(B.F32), r[:, 3:].astype(B.F32)


def test_lidar_ray_hook_on_pruned_images_matches_oracle_on_adversarial_rays():
    import torch  # noqa: F401  (before the engine initialises HIP)
    _, verts, _ = T.scene_bvh(lidar=True)
    sets = [B.random_rays(60000, 21), T.edge_aimed_rays(verts, 6, seed=11), B.near_axis_rays(verts, 20000, 22),
            B.skimming_rays(verts, 10, 23, False), B.skimming_rays(verts, 10, 24, True), _fans()]
    org = np.ascontiguousarray(np.concatenate([s[0] for s in sets]), B.F32)
    d = np.ascontiguousarray(np.concatenate([s[1] for s in sets]), B.F32)
    n_all = len(org)
    assert 100000 < n_all <= 200000
    o = T.Oracle(1, 1)
    t_ref, h_ref = np.zeros(n_all, B.F32), np.zeros(n_all, np.int32)
    o.lib.oracle_trace_ray_batch(o.h, n_all, T.fptr(org), T.fptr(d), 1, T.fptr(t_ref), h_ref.ctypes.data)
    o.close()
    at = 0
    for s in sets:  # each set exercises hits
        assert h_ref[at:at + len(s[0])].sum() * 4 > len(s[0])
        at += len(s[0])
    e = T.Engine(1, 1)
    hook = Hook(e, o=org, d=d)
    for n in sizes(n_all):
        r = hook.run(LIDAR_RAY, n, dict(t=((n_all,), np.float32), i0=((n_all,), np.int32)))
        T.compare(r["i0"][:n], h_ref[:n], f"lidar ray hit n={n}")
        T.compare(r["t"][:n], t_ref[:n], f"lidar ray t n={n}")
        assert not r["i0"][n:].any() and not r["t"][n:].any()
    e.close()


@pytest.mark.parametrize("ts,W", [(6, 3), (3, 5)], ids=["6v6x3", "3v3x5"])
def test_whole_steps_match_oracle_byte_for_byte(ts, W):
    e, o = T.Engine(W, ts), T.Oracle(W, ts)
    for sim in (e, o):
        sim.put_ctrl([0, 1, 1])
        sim.init()
    A = W * 2 * ts
    lidar = ("FWD_LIDAR", "REAR_LIDAR", "FULL_TEAM_FWD_LIDAR", "FULL_TEAM_REAR_LIDAR")
    assert set(lidar) <= set(T.STEP_OUTPUTS)
    for s in range(52):
        if s == 43:
            e.trigger_reset(1)
            o.view("RESET")[1] = 1
        acts = T.seek_combat_actions(o, s) if s < 40 else T.mpenv_tape.tape_actions(1234, s, 0, A)
        e.set_actions(acts)
        o.set_actions(acts)
        e.step()
        o.step()
        for name in T.STEP_OUTPUTS:
            T.compare(e.get(name), o.get(name), f"{name} @ step {s}")
    assert np.isfinite(o.get("FWD_LIDAR")).all()
    e.close()
    o.close()
