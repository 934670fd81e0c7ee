"""Test infrastructure for the egocentric depth camera (include/mpenv_camera.h,
DESIGN.md §2 definition 18): the ctypes binding of the header's functions, and
the expectation builder the CPU and the GPU tests share -- rays from
mpenv_camera_rays, the closest hit of the lidar tree from the oracle's octant
-order batch query, the world's capsules from the oracle's capsule test in
ascending index, depth and label formed as the kernel forms them.

Nothing here is imported by the product.
"""
import ctypes as C
import functools

import numpy as np

import mpenv_testlib as T
import scene_residency_testlib as R

vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
fp = C.POINTER(C.c_float)
ERR_INVALID, ERR_HIP = -1, -3
DEPTH, LABEL = 0, 1
DTYPE_F32, DTYPE_U8 = 1, 3
FLT_MAX = np.float32(3.40282346638528859812e+38)
CAPSULE_R, CAPSULE_H = 15.0, 35.0  # consts::agentRadius, standHeight - 2 * agentRadius
VIEW_HEIGHT = np.array([50.0, 32.0, 15.0], np.float32)  # stand, crouch, prone


class CameraConfig(C.Structure):
    _fields_ = [("width", i32), ("height", i32), ("hfov_deg", C.c_float), ("reserved", i32)]


SIGNATURES = {
    "mpenv_camera_enable": (i32, [vp, C.POINTER(CameraConfig)]),
    "mpenv_camera_disable": (i32, [vp]),
    "mpenv_camera_enabled": (i32, [vp, C.POINTER(CameraConfig), C.POINTER(i32)]),
    "mpenv_camera_render": (i32, [vp, vp]),
    "mpenv_camera_tensor": (i32, [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64),
                                  C.POINTER(i32)]),
    "mpenv_camera_layout": (i32, [C.POINTER(CameraConfig), u32, u32, C.POINTER(i64), C.POINTER(i64)]),
    "mpenv_camera_rays": (i32, [C.POINTER(CameraConfig), i32, fp, fp, C.POINTER(i32), fp, fp]),
}


def lib():
    l = T.lib_mpenv()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    return l


def config(width, height, hfov_deg=90.0):
    return CameraConfig(width, height, hfov_deg, 0)


def layout(cfg, num_worlds, team_size):
    """(return code, depth bytes, label bytes)"""
    d, l = i64(-1), i64(-1)
    rc = lib().mpenv_camera_layout(C.byref(cfg), num_worlds, team_size, C.byref(d), C.byref(l))
    return rc, d.value, l.value


def rays(cfg, pos, quat, pose):
    """mpenv_camera_rays: origins [n, 3] and directions [n, height, width, 3]."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    quat = np.ascontiguousarray(quat, np.float32).reshape(-1, 4)
    pose = np.ascontiguousarray(pose, np.int32).reshape(-1)
    n = len(pose)
    assert len(pos) == n and len(quat) == n
    org = np.empty((n, 3), np.float32)
    d = np.empty((n, cfg.height, cfg.width, 3), np.float32)
    rc = lib().mpenv_camera_rays(C.byref(cfg), n, T.fptr(pos), T.fptr(quat), pose.ctypes.data_as(C.POINTER(i32)),
                                 T.fptr(org), T.fptr(d))
    assert rc == 0, lib().mpenv_last_error().decode()
    return org, d


# ------------------------------------------------------------ the engine's side
def enable(e, cfg):
    """The status code: callers assert."""
    return lib().mpenv_camera_enable(e.h, C.byref(cfg))


def disable(e):
    return lib().mpenv_camera_disable(e.h)


def enabled(e):
    """(on, CameraConfig)"""
    on, cfg = i32(-1), CameraConfig()
    assert lib().mpenv_camera_enabled(e.h, C.byref(cfg), C.byref(on)) == 0
    return on.value, cfg


def render(e, stream=None):
    return lib().mpenv_camera_render(e.h, stream)


def tensor(e, which):
    """(return code, device pointer, dtype code, shape)"""
    ptr, dt, nd, gpu = vp(), i32(-1), i32(-1), i32(-1)
    dims = (i64 * 8)()
    rc = lib().mpenv_camera_tensor(e.h, which, C.byref(ptr), C.byref(dt), C.byref(nd), dims, C.byref(gpu))
    return rc, ptr.value, dt.value, tuple(dims[k] for k in range(max(nd.value, 0)))


def images(e):
    """The engine's (depth f32, label u8) images, copied to the host."""
    rc, p, dt, shape = tensor(e, DEPTH)
    assert rc == 0 and dt == DTYPE_F32, lib().mpenv_last_error().decode()
    depth = np.empty(shape, np.float32)
    e.mem.d2h(p, depth.nbytes, depth)
    rc, p, dt, lshape = tensor(e, LABEL)
    assert rc == 0 and dt == DTYPE_U8 and lshape == shape
    label = np.empty(shape, np.uint8)
    e.mem.d2h(p, label.nbytes, label)
    return depth, label


def check_images(e, exp, what):
    """Bit for bit: the depth by its bit patterns, the label by value."""
    depth, label = images(e)
    T.compare(depth, exp[0], f"camera depth, {what}")
    T.compare(label, exp[1], f"camera label, {what}")


# ------------------------------------------------------- the expectation builder
@functools.lru_cache(maxsize=None)
def lidar_tree(scene=T.SCENE):
    """An oracle whose per-tree queries walk the scene's lidar tree."""
    return R.TreeOracle(scene, lidar=True)


def max_dist(scene=T.SCENE):
    """The scene's lidar range: the world bounds' diagonal (collisions.bin's
    first six floats) in the float arithmetic of mpenv_core.h's length()."""
    wb = np.fromfile(scene + "/collisions.bin", np.float32, 6)
    d = wb[3:] - wb[:3]
    return np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def agent_state(sim):
    """(pos [A, 3], aim quaternion [A, 4], current pose [A]) of an oracle or an engine."""
    af, ai = sim.get("DEBUG_AGENT_F32"), sim.get("DEBUG_AGENT_I32")
    return af[:, 0:3].copy(), af[:, 12:16].copy(), ai[:, 0].copy()


def expected(cfg, pos, quat, pose, N, scene=T.SCENE):
    """(depth [A, H, W] f32, label [A, H, W] u8) for agents in world-major order, N per world, the
    first N / 2 of a world one team: traceRayAgainstWorld per pixel, from the oracle's parts."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    A, px = len(pos), cfg.height * cfg.width
    assert A % N == 0
    org, d = rays(cfg, pos, quat, pose)
    n = A * px
    o = np.ascontiguousarray(np.repeat(org, px, axis=0))
    d = np.ascontiguousarray(d.reshape(n, 3))
    tree = lidar_tree(scene)
    t = np.zeros(n, np.float32)
    hit = np.zeros(n, np.int32)
    tree.lib.oracle_trace_ray_batch(tree.h, n, T.fptr(o), T.fptr(d), 1, T.fptr(t), hit.ctypes.data)
    hit = hit != 0
    min_t = np.where(hit, t, FLT_MAX).astype(np.float32)
    ent = np.full(n, -1, np.int32)
    agent = np.repeat(np.arange(A), px)
    first = (agent // N) * N  # the world's first agent
    ocap = T.lib_oracle()
    ocap.oracle_capsule_batch.argtypes = [i32, fp, fp, C.c_float, C.c_float, fp]
    for j in range(N):
        base = pos[first + j].copy()
        base[:, 2] += np.float32(CAPSULE_R)
        tr = np.ascontiguousarray(o - base)
        tc = np.zeros(n, np.float32)
        ocap.oracle_capsule_batch(n, T.fptr(tr), T.fptr(d), CAPSULE_R, CAPSULE_H, T.fptr(tc))
        with np.errstate(invalid="ignore"):
            upd = (tc != 0) & (tc < min_t)
        min_t = np.where(upd, tc, min_t)
        ent = np.where(upd, j, ent)
        hit = hit | upd
    depth = np.where(hit, np.minimum(min_t, max_dist(scene)), np.float32(-1.0)).astype(np.float32)
    team = N // 2
    mate = (ent >= team) == ((agent - first) >= team)
    label = np.where(~hit, 0, np.where(ent == -1, 1, np.where(mate, 2, 3))).astype(np.uint8)
    shape = (A, cfg.height, cfg.width)
    return depth.reshape(shape), label.reshape(shape)


def coverage(exps, scene=T.SCENE):
    """Pixels of each label 0-3 and pixels clamped at the lidar range over a list of expectations."""
    md = max_dist(scene)
    counts = np.zeros(4, np.int64)
    clamped = 0
    for depth, label in exps:
        counts += np.bincount(label.reshape(-1), minlength=4)[:4]
        clamped += int((depth == md).sum())
    return counts, clamped


# ------------------------------------------------------------------- rollouts
@functools.lru_cache(maxsize=None)
def rollout(W, team, snaps, seed=1234, scene=T.SCENE):
    """An oracle rollout under the zone-seeking aim-bot.  snaps: the steps after which the agents'
    state is kept, -1 for the state after init.  Returns (tape, states): tape[s] the [A, 6] actions
    of step s up to the last snapshot, states {s: (pos, quat, pose)}."""
    o = T.Oracle(W, team, scene=scene)
    o.put_ctrl([0, 1, 1])
    o.init()
    states, tape = {}, []
    if -1 in snaps:
        states[-1] = agent_state(o)
    for s in range(max(snaps) + 1):
        acts = T.seek_combat_actions(o, s, seed)
        tape.append(acts)
        o.set_actions(acts)
        o.step()
        if s in snaps:
            states[s] = agent_state(o)
    o.close()
    return tape, states


# --------------------------------------------------------------- chosen poses
def quat_yaw_pitch(yaw, pitch):
    """angleAxis(yaw, up) * angleAxis(pitch, right) as (w, x, y, z), float64."""
    cy, sy, cp, sp = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2)
    # (cy, 0, 0, sy) * (cp, sp, 0, 0)
    return np.array([cy * cp, cy * sp, sy * sp, sy * cp])


def quat_towards(d):
    """A level-roll aim whose forward axis (0, 1, 0) points along the unit vector d."""
    return quat_yaw_pitch(np.arctan2(-d[0], d[1]), np.arcsin(d[2]))


def posed_cases(state, N, scene=T.SCENE):
    """The chosen poses, each an edit of one rollout state (pos, quat, pose): [(name, pos, quat, pose)].
    Every edit touches world 0 only.  "front" puts agent 0's first opponent and (team size permitting)
    two teammates 40 units in front of it, all three looking back at it; the other cases start from
    that arrangement.  With one agent per team there is no teammate to place."""
    team = N // 2
    yaw = 0.7
    fwd, right = np.array([-np.sin(yaw), np.cos(yaw), 0.0]), np.array([np.cos(yaw), np.sin(yaw), 0.0])

    def front(pos, quat, pose):
        quat[0] = quat_yaw_pitch(yaw, 0.0)
        pose[0] = 0
        others = [(team, 0.0)] + ([(1, -32.0), (2, 32.0)] if team >= 3 else [])
        for k, side in others:
            pos[k] = pos[0] + (40.0 * fwd + side * right).astype(np.float32)
            quat[k] = quat_yaw_pitch(yaw + np.pi, 0.0)
            pose[k] = 0

    def pitched(pos, quat, pose):
        quat[0] = quat_yaw_pitch(yaw, np.pi / 4)              # sky rows
        quat[team] = quat_yaw_pitch(yaw + np.pi, -np.pi / 4)  # floor rows

    def edge(pos, quat, pose):
        # the centre of agent 0's image aimed at a vertex or an edge midpoint of the lidar tree
        _, verts, _ = T.scene_bvh(scene, lidar=True)
        oo, dd = T.edge_aimed_rays(verts, 1, 11)
        k = int(np.argmax(np.abs(dd[:, 2]) < 0.3))
        pos[0] = oo[k] - np.array([0, 0, VIEW_HEIGHT[0]], np.float32)
        quat[0] = quat_towards(dd[k].astype(np.float64))

    def low(pos, quat, pose):
        pose[0] = 2        # prone
        pose[team] = 1     # crouched

    def dead(pos, quat, pose):
        # where the step parks a dead agent, looking almost straight down: the map lies beyond the lidar range
        pos[team] = (0.0, 0.0, 10000.0)
        quat[team] = quat_yaw_pitch(0.3, -1.45)

    out = []
    base = tuple(a.copy() for a in state)
    front(*base)
    out.append(("front",) + base)
    for name, edit in (("pitched", pitched), ("edge", edge), ("low", low), ("dead", dead)):
        pos, quat, pose = (a.copy() for a in base)
        edit(pos, quat, pose)
        out.append((name, pos, quat, pose))
    return out


# The batches and camera sizes the GPU tests run, and the steps whose images they compare (-1: after
# init).  test_camera_rays.py checks on the CPU that each holds every label and a clamped pixel.
CONFIGS = {
    "1x1v1_8x8": dict(W=1, team=1, cam=(8, 8, 60.0), snaps=(-1, 3, 40)),
    "3x3v3_16x8": dict(W=3, team=3, cam=(16, 8, 90.0), snaps=(-1, 3, 40)),
    "5x6v6_24x16": dict(W=5, team=6, cam=(24, 16, 100.0), snaps=(-1, 3, 40)),
    "5x6v6_64x32": dict(W=5, team=6, cam=(64, 32, 90.0), snaps=(40,)),
    # a scene beyond the LDS path's limits (scene_residency_testlib.pillars): global-resident under "auto"
    "pillars_3x3v3_16x8": dict(W=3, team=3, cam=(16, 8, 90.0), snaps=(-1, 3), pillars=100),
}


def scene_of(name):
    c = CONFIGS[name]
    return R.pillars(c["pillars"]) if "pillars" in c else T.SCENE


@functools.lru_cache(maxsize=None)
def plan(name):
    """What one configuration renders: (cfg, tape, [(step, expectation)], [(case name, pos, quat, pose,
    expectation)]).  The posed cases edit the first snapshot."""
    c = CONFIGS[name]
    scene = scene_of(name)
    cfg = config(*c["cam"])
    N = 2 * c["team"]
    tape, states = rollout(c["W"], c["team"], c["snaps"], scene=scene)
    steps = [(s, expected(cfg, *states[s], N, scene)) for s in c["snaps"]]
    posed = [(nm, p, q, ps, expected(cfg, p, q, ps, N, scene))
             for nm, p, q, ps in posed_cases(states[c["snaps"][0]], N, scene)]
    return cfg, tape, steps, posed
