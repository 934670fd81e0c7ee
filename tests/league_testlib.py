"""Test infrastructure for the league scheduler (include/mpenv_league.h, DESIGN.md
§2 definition 20): the ctypes binding of the header's functions, the numpy
restatement of the definitions (built on mpenv_tape.threefry2x32), and the
posed episode ends the GPU tests share.

Nothing here is imported by the product.
"""
import ctypes as C

import numpy as np

import mpenv_testlib as T
import posed_testlib as PT

vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
ip, lp = C.POINTER(i32), C.POINTER(i64)
ERR_INVALID = -1
NONE, TEAM1, BOTH = 0, 1, 2
TABLE, WEIGHTS, DRAWS = 0, 1, 2
DTYPE_I32, DTYPE_U32, DTYPE_I64 = 0, 2, 6
KEY_UPPER = 0x4C454147
MAX_WEIGHT = 65535
SIMFLAG_SUB_ZONES = 1 << 11


class LeagueConfig(C.Structure):
    _fields_ = [("num_policies", i32), ("draw", i32), ("seed", u32), ("reserved", i32)]


SIGNATURES = {
    "mpenv_league_enable": (i32, [vp, C.POINTER(LeagueConfig)]),
    "mpenv_league_disable": (i32, [vp]),
    "mpenv_league_enabled": (i32, [vp, C.POINTER(LeagueConfig), ip]),
    "mpenv_league_tensor": (i32, [vp, i32, C.POINTER(vp), ip, ip, lp, ip]),
    "mpenv_league_clear": (i32, [vp, vp]),
    "mpenv_league_set_weights": (i32, [vp, ip]),
    "mpenv_league_layout": (i32, [C.POINTER(LeagueConfig), u32, lp, lp, lp]),
    "mpenv_league_draw": (i32, [C.POINTER(LeagueConfig), u32, u32, ip, i32, ip]),
    "mpenv_league_record": (i32, [C.POINTER(LeagueConfig), ip, ip, i32, lp]),
}


def lib():
    l = T.lib_mpenv()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    return l


def err():
    return lib().mpenv_last_error().decode()


def config(P, draw=TEAM1, seed=0):
    return LeagueConfig(P, draw, seed, 0)


def _ip(a):
    return a.ctypes.data_as(ip)


def draw(cfg, world, n, weights, ids):
    """mpenv_league_draw on a copy of ids [2, T]: (return code, new ids)."""
    out = np.ascontiguousarray(ids, np.int32).copy()
    w = None if weights is None else _ip(np.ascontiguousarray(weights, np.int32))
    rc = lib().mpenv_league_draw(C.byref(cfg), world, n, w, out.shape[1], _ip(out))
    return rc, out


def record(cfg, mr, ids, table):
    """mpenv_league_record into table (int64, in place): the return code."""
    ids = np.ascontiguousarray(ids, np.int32)
    mr = np.ascontiguousarray(mr, np.int32)
    assert table.dtype == np.int64 and table.flags.c_contiguous
    return lib().mpenv_league_record(C.byref(cfg), _ip(mr), _ip(ids), ids.shape[1], table.ctypes.data_as(lp))


def layout(cfg, num_worlds):
    t, w, d = i64(-1), i64(-1), i64(-1)
    rc = lib().mpenv_league_layout(C.byref(cfg), num_worlds, C.byref(t), C.byref(w), C.byref(d))
    return rc, t.value, w.value, d.value


# ------------------------------------------------------------ the restatement
def ref_bucket(p, P):
    return int(p) if 0 <= p < P else P


def ref_team_id(rows):
    rows = np.asarray(rows).reshape(-1)
    return int(rows[0]) if (rows == rows[0]).all() else -1


def ref_pick(row, x):
    """None for no change."""
    w = np.clip(np.asarray(row, np.int64), 0, MAX_WEIGHT)
    tot = int(w.sum())
    if tot == 0:
        return None
    r = (int(x) * tot) >> 32
    return int(np.flatnonzero(np.cumsum(w) > r)[0])


def ref_hash(seed, gworld, n):
    a, b = T.mpenv_tape.threefry2x32(np.array([seed], np.uint32), np.array([KEY_UPPER], np.uint32),
                                     np.array([gworld], np.uint32), np.array([n], np.uint32))
    return int(a[0]), int(b[0])


def ref_draw(P, mode, seed, gworld, n, weights, ids):
    """ids [2, T] -> new ids [2, T]"""
    out = np.array(ids, np.int32)
    if mode == NONE:
        return out
    weights = np.ones((P + 1, P), np.int32) if weights is None else np.asarray(weights).reshape(P + 1, P)
    ha, hb = ref_hash(seed, gworld, n)
    i0 = ref_team_id(out[0])
    if mode == BOTH:
        p0 = ref_pick(weights[P], ha)
        if p0 is not None:
            out[0] = i0 = p0
    p1 = ref_pick(weights[ref_bucket(i0, P)], hb)
    if p1 is not None:
        out[1] = p1
    return out


def ref_record(P, mr, ids, table):
    c = table[ref_bucket(ref_team_id(ids[0]), P), ref_bucket(ref_team_id(ids[1]), P)]
    c[0] += 1
    for k in range(3):
        c[1 + k] += int(mr[0] == k)
    c[4:8] += np.asarray(mr[1:5], np.int64)


class Ref:
    """The restated league of one manager: visit() is what k_league does behind a step (or an init)
    from that step's DONE / MATCH_RESULT / AGENT_POLICY exports."""

    def __init__(self, P, mode, seed, W, T_, offset=0):
        self.P, self.mode, self.seed, self.W, self.T, self.offset = P, mode, seed, W, T_, offset
        self.table = np.zeros((P + 1, P + 1, 8), np.int64)
        self.weights = np.ones((P + 1, P), np.int32)
        self.draws = np.zeros(W, np.uint32)

    def visit(self, done, mr, policy, init=False):
        """-> the AGENT_POLICY column after the visit [A, 1]; init: done and mr are not read"""
        N = 2 * self.T
        pol = np.array(policy, np.int32).reshape(self.W, 2, self.T)
        if not init:
            done = np.asarray(done).reshape(self.W, N)
            mr = np.asarray(mr).reshape(self.W, -1)
        for w in range(self.W):
            if not (init or done[w, 0] == 1):
                continue
            if not init:
                ref_record(self.P, mr[w], pol[w], self.table)
            if self.mode != NONE:
                pol[w] = ref_draw(self.P, self.mode, self.seed, self.offset + w, int(self.draws[w]), self.weights, pol[w])
                self.draws[w] += 1
        return pol.reshape(-1, 1)


# ------------------------------------------------------------ the engine's side
def enable(e, cfg):
    return lib().mpenv_league_enable(e.h, C.byref(cfg))


def disable(e):
    return lib().mpenv_league_disable(e.h)


def enabled(e):
    on, cfg = i32(-1), LeagueConfig()
    assert lib().mpenv_league_enabled(e.h, C.byref(cfg), C.byref(on)) == 0
    return on.value, cfg


def tensor(e, which):
    """(return code, device pointer, dtype code, shape)"""
    ptr, dt, nd, gpu = vp(), i32(-1), i32(-1), i32(-1)
    dims = (i64 * 8)()
    rc = lib().mpenv_league_tensor(e.h, which, C.byref(ptr), C.byref(dt), C.byref(nd), dims, C.byref(gpu))
    return rc, ptr.value, dt.value, tuple(dims[k] for k in range(max(nd.value, 0)))


def read(e, which):
    rc, p, dt, shape = tensor(e, which)
    assert rc == 0, err()
    out = np.empty(shape, {DTYPE_I64: np.int64, DTYPE_I32: np.int32, DTYPE_U32: np.uint32}[dt])
    e.mem.hip.hipDeviceSynchronize()
    e.mem.d2h(p, out.nbytes, out)
    return out


def set_weights(e, w):
    w = np.ascontiguousarray(w, np.int32)
    return lib().mpenv_league_set_weights(e.h, _ip(w))


def clear(e):
    return lib().mpenv_league_clear(e.h, None)


def check(e, ref, where, policy=None):
    """The engine's three league buffers, and its AGENT_POLICY column, equal the restatement's."""
    T.compare(read(e, TABLE), ref.table, f"league table @ {where}")
    T.compare(read(e, DRAWS), ref.draws, f"league draws @ {where}")
    T.compare(read(e, WEIGHTS), ref.weights, f"league weights @ {where}")
    if policy is not None:
        T.compare(e.get("AGENT_POLICY"), policy, f"AGENT_POLICY @ {where}")


# ------------------------------------------------------------ posed episode ends
W, TEAM, P = 70, 2, 3
TAPE_SEED = 1234
STEPS = 5


def pose_ends(e, policy, cur_step=None, first_world=0):
    """Through a snapshot: curStep = 2998 - w % 3 (or cur_step for every world), MATCH_RESULT rows
    {-1, 3, 1, w % 5, w % 4}, AGENT_POLICY = policy [A]; loaded.  w counts from first_world (a shard)."""
    sec = PT.sections(e)
    nw = e.W
    w = first_world + np.arange(nw)
    blob = e.new_state_blob()
    try:
        e.state_save(blob)
        e.mem.hip.hipDeviceSynchronize()

        def put_step(r):
            r[:, 0] = (2998 - w % 3) if cur_step is None else cur_step

        def put_mr(r):
            r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = -1, 3, 1, w % 5, w % 4

        def put_pol(r):
            r[:, 0] = np.asarray(policy, np.int32).reshape(-1)

        PT._blob_rw(e, blob, sec["curStep"], np.int32, put_step)
        PT._blob_rw(e, blob, sec["MATCH_RESULT"], np.int32, put_mr)
        PT._blob_rw(e, blob, sec["AGENT_POLICY"], np.int32, put_pol)
        e.state_load(blob)
        assert e.state_error() == 0
        e.mem.hip.hipDeviceSynchronize()
    finally:
        e.mem.free(blob)


def standings_ids(nw=W, team=TEAM, P_=P):
    """AGENT_POLICY [A] for the standings tests: the worlds of the first wave (0..63) all sit in
    cell [1][2]; the second wave's six worlds hold six distinct cells: a mixed team, an external
    one (-1), ids of P and above, and plain ones."""
    pol = np.zeros((nw, 2, team), np.int32)
    pol[:, 0], pol[:, 1] = 1, 2
    tail = [((0, 0), (1, 1)), ((0, 1), (2, 2)), ((-1, -1), (0, 0)), ((2, 2), (P_, P_)), ((40, 40), (40, 40)),
            ((2, 2), (1, 1)), ((1, 1), (-1, -1))]
    for k, (a, b) in enumerate(tail):
        if 64 + k < nw:
            pol[64 + k, 0], pol[64 + k, 1] = a[:team], b[:team]
    return pol.reshape(-1)


def tape_step(e, k, first_world=0):
    """Step k of the tape for an engine whose world 0 is world `first_world` of the run."""
    e.set_actions(T.mpenv_tape.tape_actions(TAPE_SEED, k, first_world * e.N, e.W * e.N))
    e.step()
