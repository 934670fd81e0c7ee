"""The egocentric depth camera without a GPU (include/mpenv_camera.h, DESIGN.md
§2 definition 18): buffer sizes and refused configurations, the rays of
mpenv_camera_rays against a float64 pinhole written here, and the coverage of
the expectations tests/test_camera_gpu.py compares the kernel with."""
import ctypes as C

import numpy as np
import pytest

import camera_testlib as K
import mpenv_testlib as T

F32_EPS = float(np.finfo(np.float32).eps)


def test_layout_bytes():
    for (w, h, W, team) in ((8, 8, 1, 1), (64, 32, 16384, 6), (24, 16, 5, 3), (128, 128, 7, 2)):
        rc, depth, label = K.layout(K.config(w, h), W, team)
        A = W * 2 * team
        assert rc == 0 and depth == A * h * w * 4 and label == A * h * w, (w, h, W, team, rc, depth, label)
    # C3 at 64 x 32: 196,608 agents x 2,048 pixels x 5 B
    rc, depth, label = K.layout(K.config(64, 32), 16384, 6)
    assert depth + label == 196608 * 2048 * 5 == 2013265920


@pytest.mark.parametrize("w,h,fov,needle", [
    (12, 8, 90.0, "width"), (8, 0, 90.0, "height"), (136, 8, 90.0, "width"), (8, 136, 90.0, "height"),
    (8, 8, 0.0, "hfov"), (8, 8, 170.0, "hfov"), (8, 8, float("nan"), "hfov"), (-8, 8, 90.0, "width"),
])
def test_bad_configurations_are_refused_with_the_reason(w, h, fov, needle):
    lib = K.lib()
    rc, depth, label = K.layout(K.config(w, h, fov), 4, 3)
    assert rc == K.ERR_INVALID and (depth, label) == (-1, -1)
    assert needle in lib.mpenv_last_error().decode()
    one = np.zeros(4, np.float32)
    out = np.zeros(3 * max(w, 8) * max(h, 8), np.float32)
    cfg = K.config(w, h, fov)
    rc = lib.mpenv_camera_rays(C.byref(cfg), 1, T.fptr(one), T.fptr(one), np.zeros(1, np.int32).ctypes.data_as(
        C.POINTER(C.c_int32)), T.fptr(one), T.fptr(out))
    assert rc == K.ERR_INVALID and needle in lib.mpenv_last_error().decode()


def test_layout_refuses_a_bad_batch():
    assert K.layout(K.config(8, 8), 0, 3)[0] == K.ERR_INVALID
    assert K.layout(K.config(8, 8), 4, 7)[0] == K.ERR_INVALID


# ------------------------------------------------ the float64 pinhole model
def qrot64(q, v):
    """Rotation of v by the quaternion q = (w, x, y, z), normalised first, in float64."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q)
    w, p = q[0], q[1:]
    t = 2.0 * np.cross(p, v)
    return v + w * t + np.cross(p, t)


def pinhole64(width, height, hfov_deg, quat):
    """Unit directions [height, width, 3] of the model in the issue, float64, no library call."""
    th = np.tan(np.deg2rad(np.float64(hfov_deg)) / 2)
    sx = th * ((2 * np.arange(width) + 1) / width - 1)
    sy = th * (height / width) * (1 - (2 * np.arange(height) + 1) / height)
    fwd, right, up = (qrot64(quat, np.array(v, np.float64)) for v in ((0, 1, 0), (1, 0, 0), (0, 0, 1)))
    d = fwd[None, None] + sx[None, :, None] * right[None, None] + sy[:, None, None] * up[None, None]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _poses():
    """The identity, a yaw of 2.5 rad with pitch +-pi/4, and 50 random unit quaternions."""
    rng = np.random.default_rng(18)
    q = rng.normal(size=(50, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    named = [np.array([1.0, 0, 0, 0]), K.quat_yaw_pitch(2.5, np.pi / 4), K.quat_yaw_pitch(2.5, -np.pi / 4)]
    return np.concatenate([np.array(named), q]).astype(np.float32)


@pytest.mark.parametrize("w,h,fov", [(64, 32, 90.0), (8, 8, 60.0)])
def test_rays_against_a_float64_pinhole(w, h, fov):
    quat = _poses()
    n = len(quat)
    rng = np.random.default_rng(3)
    pos = rng.uniform(-2000, 2000, (n, 3)).astype(np.float32)
    pose = (np.arange(n) % 3).astype(np.int32)
    org, d = K.rays(K.config(w, h, fov), pos, quat, pose)
    # unit length to 2 ulp (of 1.0)
    ln = np.linalg.norm(d.astype(np.float64), axis=-1)
    assert np.abs(ln - 1).max() <= 2 * F32_EPS, np.abs(ln - 1).max()
    worst = 0.0
    for k in range(n):
        ref = pinhole64(w, h, fov, quat[k].astype(np.float64))
        dk = d[k].astype(np.float64)
        # the angle between the two, from the cross product (accurate for small angles)
        ang = np.arctan2(np.linalg.norm(np.cross(dk, ref), axis=-1), (dk * ref).sum(-1))
        worst = max(worst, float(ang.max()))
    assert worst <= 1e-6, worst
    # origins: pos + (0, 0, viewHeight(pose)), one float addition
    exp = pos.copy()
    exp[:, 2] += K.VIEW_HEIGHT[pose]
    T.compare(org, exp, "camera origins")


@pytest.mark.parametrize("w,h,fov", [(64, 32, 90.0), (8, 8, 60.0)])
def test_centre_corners_and_origins(w, h, fov):
    quat = _poses()[:3]
    pos = np.array([[0, 0, 0], [100.5, -3.25, 7.125], [-1999.9, 1234.5, 0.39369965]], np.float32)
    pose = np.array([0, 1, 2], np.int32)
    org, d = K.rays(K.config(w, h, fov), pos, quat, pose)
    exp = pos.copy()
    exp[:, 2] += np.array([50, 32, 15], np.float32)
    T.compare(org, exp, "camera origins (stand, crouch, prone)")
    th = np.tan(np.deg2rad(fov) / 2)
    for k in range(3):
        q = quat[k].astype(np.float64)
        fwd, right, up = (qrot64(q, np.array(v, np.float64)) for v in ((0, 1, 0), (1, 0, 0), (0, 0, 1)))
        mid = d[k, h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1].astype(np.float64).reshape(4, 3).sum(0)
        mid /= np.linalg.norm(mid)
        assert np.abs(mid - fwd).max() <= 1e-6, (k, mid, fwd)
        # a corner pixel's centre lies half a pixel inside the configured half-angles
        for r, c, sgx, sgy in ((0, 0, -1, 1), (0, w - 1, 1, 1), (h - 1, 0, -1, -1), (h - 1, w - 1, 1, -1)):
            v = d[k, r, c].astype(np.float64)
            x, y, z = v @ right, v @ up, v @ fwd
            assert abs(x / z - sgx * th * (1 - 1 / w)) <= 1e-6 and abs(y / z - sgy * th * (h / w) * (1 - 1 / h)) <= 1e-6
    if fov == 90.0:
        # identity pose: forward is +y, the left column looks towards -x, the top row up
        assert d[0, 0, 0, 0] < 0 < d[0, 0, 0, 2] and d[0, h - 1, w - 1, 0] > 0 > d[0, h - 1, w - 1, 2]


def test_python_module_exposes_the_camera_model():
    import madrona_mp_env as m

    for name in ("enable_camera", "disable_camera", "camera_config", "render_camera", "camera_depth", "camera_label"):
        assert hasattr(m.SimManager, name), name
    lay = m.camera_layout(64, 32, 90.0, num_worlds=16384, team_size=6)
    assert lay["shape"] == (196608, 32, 64) and lay["depth_bytes"] == 4 * lay["label_bytes"] == 196608 * 2048 * 4
    quat = _poses()[:5]
    pos = np.arange(15, dtype=np.float32).reshape(5, 3)
    pose = np.array([0, 1, 2, 0, 1], np.int32)
    org, d = m.camera_rays(8, 8, 60.0, pos, quat, pose)
    o2, d2 = K.rays(K.config(8, 8, 60.0), pos, quat, pose)
    T.compare(np.asarray(org), o2, "camera_rays origins")
    T.compare(np.asarray(d), d2, "camera_rays directions")
    with pytest.raises(Exception, match="width"):
        m.camera_rays(12, 8, 60.0, pos, quat, pose)
    with pytest.raises(Exception, match="hfov"):
        m.camera_layout(8, 8, 170.0)


# --------------------------------------------------- the expectation builder
@pytest.mark.parametrize("name", list(K.CONFIGS))
def test_gpu_configurations_cover_every_label_and_the_clamp(name):
    """Conditions on what tests/test_camera_gpu.py compares, not measurements: each configuration's
    expectations (the rollout's snapshots and the chosen poses together) hold at least 100 pixels of
    every label and at least one pixel clamped at the lidar range.

    Which supplies what: the rollout under seek_combat_actions gives the misses (0), the map (1)
    and, from three agents a team, teammates (2); the teams rarely have each other in view within
    the few steps a quick test can afford, and a killed agent respawns within its step, so the
    opponents (3) come from the chosen poses "front", "pitched" and "low" and the clamped pixels
    from "dead" (an agent parked at z = 10000 looking down at the map).  With one agent a team
    (1 world 1v1) there is no teammate in the world and label 2 cannot occur: that configuration
    is held to labels 0, 1 and 3."""
    c = K.CONFIGS[name]
    cfg, tape, steps, posed = K.plan(name)
    assert len(tape) == max(c["snaps"]) + 1 and [s for s, _ in steps] == list(c["snaps"])
    assert [p[0] for p in posed] == ["front", "pitched", "edge", "low", "dead"]
    exps = [e for _, e in steps] + [p[4] for p in posed]
    A = c["W"] * 2 * c["team"]
    for depth, label in exps:
        assert depth.shape == label.shape == (A, cfg.height, cfg.width)
        assert depth.dtype == np.float32 and label.dtype == np.uint8
        assert ((depth == -1) == (label == 0)).all() and (depth[label != 0] > 0).all()
    counts, clamped = K.coverage(exps, K.scene_of(name))
    need = (0, 1, 3) if c["team"] == 1 else (0, 1, 2, 3)
    for lab in need:
        assert counts[lab] >= 100, (name, lab, counts)
    if c["team"] == 1:
        assert counts[2] == 0
    assert clamped >= 1, name
    # the chosen poses do what their names say
    by = {p[0]: p[4] for p in posed}
    team = c["team"]
    assert (by["front"][1][0] == 3).sum() > 0 and (by["front"][1][team] == 3).sum() > 0
    if team >= 3:
        assert (by["front"][1][0] == 2).sum() > 0
    assert (by["pitched"][1][0][0] == 0).any(), "the top row of a viewer pitched up by pi/4 holds sky"
    assert (by["pitched"][1][team][-1] != 0).all(), "the bottom row of a viewer pitched down by pi/4 holds no sky"
    md = K.max_dist(K.scene_of(name))
    assert (by["dead"][0][team] == md).any() and not (by["dead"][1][team] == 3).any()
