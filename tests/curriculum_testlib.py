"""Test infrastructure for the live curriculum pool (include/mpenv_curriculum.h,
DESIGN.md §2 definition 21): the ctypes binding of the header's functions, the
numpy restatement of selection, filter and packing (built on
mpenv_tape.threefry2x32), and the engine-side helpers the GPU tests share.

Nothing here is imported by the product.
"""
import ctypes as C

import numpy as np

import mpenv_testlib as T

import mpenv_curriculum as MC  # noqa: E402  (the package directory is on sys.path through mpenv_testlib)

vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
ip, lp, fp = C.POINTER(i32), C.POINTER(i64), C.POINTER(C.c_float)
ERR_INVALID = -1
POOL, TICKS = 0, 1
DTYPE_U32, DTYPE_U8 = 2, 3
KEY_UPPER = 0x43555252
NEED_CAPTURED, NEED_CONTESTED, NEED_BOTH_ALIVE = 1, 2, 4
EPISODE_LEN = 3000
SNAPSHOT = MC.SNAPSHOT
PI = np.float32(3.14159265358979323846)

# DEBUG_WORLD_I32 / DEBUG_AGENT_* columns (include/mpenv.h)
WI_TEAM_A, WI_CUR_STEP, WI_FINISHED, WI_CUR_ZONE, WI_CONTROLLING, WI_CONTESTED, WI_CAPTURED = 0, 1, 2, 3, 4, 5, 6
WI_ZONE_STEPS, WI_STEPS_UNTIL_POINT = 8, 9
AF_POS, AF_YAW, AF_PITCH = 0, 10, 11
AI_CUR_POSE, AI_LANDED_ON = 0, 6


class PoolConfig(C.Structure):
    _fields_ = [("capacity", i32), ("period", i32), ("step_lo", i32), ("step_hi", i32), ("need", u32), ("seed", u32)]


class World(C.Structure):
    _fields_ = [("cur_step", i32), ("cur_zone", i32), ("captured", i32), ("controlling", i32), ("zone_steps", i32),
                ("steps_until_point", i32), ("pos", fp), ("yaw", fp), ("pitch", fp), ("hp", fp), ("magazine", ip),
                ("cur_pose", ip), ("landed_on", ip)]


SIGNATURES = {
    "mpenv_curriculum_pool_enable": (i32, [vp, C.POINTER(PoolConfig)]),
    "mpenv_curriculum_pool_disable": (i32, [vp]),
    "mpenv_curriculum_pool_enabled": (i32, [vp, C.POINTER(PoolConfig), ip]),
    "mpenv_curriculum_pool_tensor": (i32, [vp, i32, C.POINTER(vp), ip, ip, lp, ip]),
    "mpenv_curriculum_pool_tick": (i32, [vp, C.POINTER(u32)]),
    "mpenv_curriculum_pool_set": (i32, [vp, i32, i32, i32, vp]),
    "mpenv_curriculum_pool_configure": (i32, [vp, C.POINTER(PoolConfig)]),
    "mpenv_curriculum_pool_layout": (i32, [C.POINTER(PoolConfig), i32, lp, lp]),
    "mpenv_curriculum_pool_select": (i32, [u32, u32, u32, u32, u32, i32, i32, i32, ip, ip]),
    "mpenv_curriculum_pool_pack": (i32, [C.POINTER(World), i32, vp]),
}


def lib():
    l = T.lib_mpenv()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    return l


def err():
    return lib().mpenv_last_error().decode()


def config(capacity, period=64, step_range=(0, EPISODE_LEN - 1), need=0, seed=0):
    return PoolConfig(capacity, period, step_range[0], step_range[1], need, seed)


def layout(cfg, num_ranges):
    p, t = i64(-1), i64(-1)
    rc = lib().mpenv_curriculum_pool_layout(C.byref(cfg), num_ranges, C.byref(p), C.byref(t))
    return rc, p.value, t.value


def select(seed, offset, r, slot, tick, period, first, n):
    """mpenv_curriculum_pool_select: (return code, refresh, world)"""
    ref, w = i32(-1), i32(-1)
    rc = lib().mpenv_curriculum_pool_select(seed, offset, r, slot, tick, period, first, n, C.byref(ref), C.byref(w))
    return rc, ref.value, w.value


def world_rows(cur_step, cur_zone, captured, controlling, zone_steps, steps_until_point, pos, yaw, pitch, hp, magazine,
               cur_pose, landed_on):
    """One world's state as the plain arrays pack() and ref_pack() take."""
    return dict(cur_step=int(cur_step), cur_zone=int(cur_zone), captured=int(captured), controlling=int(controlling),
                zone_steps=int(zone_steps), steps_until_point=int(steps_until_point),
                pos=np.ascontiguousarray(pos, np.float32).reshape(-1, 3), yaw=np.ascontiguousarray(yaw, np.float32),
                pitch=np.ascontiguousarray(pitch, np.float32), hp=np.ascontiguousarray(hp, np.float32),
                magazine=np.ascontiguousarray(magazine, np.int32).reshape(-1, 2),
                cur_pose=np.ascontiguousarray(cur_pose, np.int32), landed_on=np.ascontiguousarray(landed_on, np.int32))


def pack(rows, team_size):
    """mpenv_curriculum_pool_pack: (return code, one SNAPSHOT record); the output starts as 0xA5 bytes"""
    w = World(rows["cur_step"], rows["cur_zone"], rows["captured"], rows["controlling"], rows["zone_steps"],
              rows["steps_until_point"], rows["pos"].ctypes.data_as(fp), rows["yaw"].ctypes.data_as(fp),
              rows["pitch"].ctypes.data_as(fp), rows["hp"].ctypes.data_as(fp), rows["magazine"].ctypes.data_as(ip),
              rows["cur_pose"].ctypes.data_as(ip), rows["landed_on"].ctypes.data_as(ip))
    out = np.full(176, 0xA5, np.uint8)
    rc = lib().mpenv_curriculum_pool_pack(C.byref(w), team_size, out.ctypes.data)
    return rc, out.view(SNAPSHOT)[0]


# ------------------------------------------------------------ the restatement
def ref_hash(seed, global_first, slots, tick):
    """(lo32, hi32) uint32 arrays over `slots`; global_first = world_id_offset + the range's first world"""
    slots = np.asarray(slots, np.uint32)
    one = np.ones(1, np.uint32)
    a, b = T.mpenv_tape.threefry2x32(one * np.uint32(seed), one * np.uint32(KEY_UPPER), one * np.uint32(global_first),
                                     one * np.uint32(0))
    return T.mpenv_tape.threefry2x32(np.broadcast_to(a, slots.shape), np.broadcast_to(b, slots.shape), slots,
                                     np.full(slots.shape, tick, np.uint32))


def ref_select(seed, offset, slots, tick, period, first, n):
    """(refresh bool [len(slots)], world int [len(slots)])"""
    lo, hi = ref_hash(seed, offset + first, slots, tick)
    refresh = (lo % np.uint32(period) == 0) if period > 0 else np.zeros(len(lo), bool)
    return refresh, first + (hi % np.uint32(n)).astype(np.int64)


def _i16(x):
    """float32 -> int32 (towards zero) -> int16 (wrapping)"""
    return np.asarray(x, np.float32).astype(np.int32).astype(np.int16)


def ref_pack(rows, team_size):
    sn = np.zeros(1, SNAPSHOT)[0]
    sn["step"] = max(rows["cur_step"] - 1, 0)
    sn["cur_zone"] = rows["cur_zone"]
    sn["controller"] = rows["controlling"] if rows["captured"] else -1
    sn["zone_steps_remaining"] = rows["zone_steps"]
    sn["steps_until_point"] = rows["steps_until_point"]
    n = 2 * team_size
    pl = sn["players"]
    pl["pos"][:n] = _i16(rows["pos"][:n])
    pl["yaw"][:n] = _i16(rows["yaw"][:n] * np.float32(32768) / PI)
    pl["pitch"][:n] = _i16(rows["pitch"][:n] * np.float32(32768) / PI)
    pl["mag"][:n] = rows["magazine"][:n, 0].astype(np.uint16).astype(np.uint8)
    pl["reloading"][:n] = rows["magazine"][:n, 1].astype(np.uint8)
    pl["hp"][:n] = rows["hp"][:n].astype(np.int32).astype(np.uint8)
    pose = rows["cur_pose"][:n]
    pl["flags"][:n] = 2 * (rows["landed_on"][:n] != -1) + 4 * (pose == 1) + 8 * (pose == 2)
    return sn


def ref_accept(finished, cur_step, cfg, captured, contested, hp, team_size):
    """The filter on one world; hp [n]"""
    if finished != 0 or not cfg.step_lo <= cur_step <= cfg.step_hi:
        return False
    if cfg.need & NEED_CAPTURED and not captured:
        return False
    if cfg.need & NEED_CONTESTED and not contested:
        return False
    if cfg.need & NEED_BOTH_ALIVE and not ((hp[:team_size] > 0).any() and (hp[team_size:2 * team_size] > 0).any()):
        return False
    return True


# ------------------------------------------------------------ the engine's side
class State:
    """What k_harvest reads, from the engine's (or the oracle's) exports."""

    def __init__(self, sim):
        W, N = sim.W, sim.N
        self.W, self.N = W, N
        self.af = sim.get("DEBUG_AGENT_F32").reshape(W, N, -1)
        self.ai = sim.get("DEBUG_AGENT_I32").reshape(W, N, -1)
        self.wi = sim.get("DEBUG_WORLD_I32").reshape(W, -1)
        self.hp = sim.get("HP").reshape(W, N)
        self.mag = sim.get("MAGAZINE").reshape(W, N, 2)

    def rows(self, w):
        wi = self.wi[w]
        return world_rows(wi[WI_CUR_STEP], wi[WI_CUR_ZONE], wi[WI_CAPTURED], wi[WI_CONTROLLING], wi[WI_ZONE_STEPS],
                          wi[WI_STEPS_UNTIL_POINT], self.af[w, :, AF_POS:AF_POS + 3], self.af[w, :, AF_YAW],
                          self.af[w, :, AF_PITCH], self.hp[w], self.mag[w], self.ai[w, :, AI_CUR_POSE],
                          self.ai[w, :, AI_LANDED_ON])

    def pack(self, w):
        return ref_pack(self.rows(w), self.N // 2)

    def accept(self, w, cfg):
        wi = self.wi[w]
        return ref_accept(wi[WI_FINISHED], wi[WI_CUR_STEP], cfg, wi[WI_CAPTURED], wi[WI_CONTESTED], self.hp[w], self.N // 2)


def enable(e, cfg):
    return lib().mpenv_curriculum_pool_enable(e.h, C.byref(cfg))


def disable(e):
    return lib().mpenv_curriculum_pool_disable(e.h)


def configure(e, cfg):
    return lib().mpenv_curriculum_pool_configure(e.h, C.byref(cfg))


def enabled(e):
    on, cfg = i32(-1), PoolConfig()
    assert lib().mpenv_curriculum_pool_enabled(e.h, C.byref(cfg), C.byref(on)) == 0
    return on.value, cfg


def tick(e):
    t = u32(0xFFFFFFFF)
    assert lib().mpenv_curriculum_pool_tick(e.h, C.byref(t)) == 0, err()
    return t.value


def tensor(e, which):
    """(return code, device pointer, dtype code, shape)"""
    ptr, dt, nd, gpu = vp(), i32(-1), i32(-1), i32(-1)
    dims = (i64 * 8)()
    rc = lib().mpenv_curriculum_pool_tensor(e.h, which, C.byref(ptr), C.byref(dt), C.byref(nd), dims, C.byref(gpu))
    return rc, ptr.value, dt.value, tuple(dims[k] for k in range(max(nd.value, 0)))


def read(e):
    """(pool as SNAPSHOT [R, capacity], ticks uint32 [R, capacity]) after a device synchronise"""
    e.mem.hip.hipDeviceSynchronize()
    rc, p, dt, shape = tensor(e, POOL)
    assert rc == 0 and dt == DTYPE_U8 and shape[2] == 176, err()
    assert p % 16 == 0
    raw = np.empty(shape, np.uint8)
    e.mem.d2h(p, raw.nbytes, raw)
    rc, p, dt, tshape = tensor(e, TICKS)
    assert rc == 0 and dt == DTYPE_U32 and tshape == shape[:2], err()
    ticks = np.empty(tshape, np.uint32)
    e.mem.d2h(p, ticks.nbytes, ticks)
    return raw.view(SNAPSHOT).reshape(shape[:2]), ticks


def pool_set(e, snaps, map_range=0, first_slot=0):
    snaps = np.ascontiguousarray(snaps)
    assert snaps.nbytes % 176 == 0
    return lib().mpenv_curriculum_pool_set(e.h, map_range, first_slot, snaps.nbytes // 176, snaps.ctypes.data)


def model_harvest(pool, ticks, state, cfg, t, ranges, offset=0):
    """The restated k_harvest at tick t on copies of (pool, ticks): -> (pool, ticks, refreshed [R, cap] bool,
    candidate world [R, cap]).  ranges: [(first_world, num_worlds)] per pool row."""
    pool, ticks = pool.copy(), ticks.copy()
    cap = pool.shape[1]
    refreshed = np.zeros(pool.shape, bool)
    cands = np.zeros(pool.shape, np.int64)
    for r, (first, n) in enumerate(ranges):
        ref, world = ref_select(cfg.seed, offset, np.arange(cap), t, cfg.period, first, n)
        refreshed[r], cands[r] = ref, world
        for s in np.flatnonzero(ref):
            if state.accept(world[s], cfg):
                pool[r, s] = state.pack(world[s])
                ticks[r, s] = t
    return pool, ticks, refreshed, cands


def started_from(wi_row, af_world, hp_world, snap, n):
    """Whether a world's post-reset state is snapshot `snap` applied (as tests/test_curriculum_data.py
    recognises it): step, zone, and every player's position and hp under the world's team order."""
    if wi_row[WI_CUR_STEP] != snap["step"] or wi_row[WI_CUR_ZONE] != snap["cur_zone"]:
        return False
    half = n // 2
    order = np.arange(n) if wi_row[WI_TEAM_A] == 0 else np.r_[half:n, 0:half]
    p = snap["players"][:n]
    return bool(np.array_equal(af_world[order, 0:3], p["pos"].astype(np.float32)) and
                np.array_equal(hp_world[order], p["hp"].astype(np.float32)))
