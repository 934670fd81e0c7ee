"""Posed-state parity (test infrastructure; DESIGN.md §7 "Posed states").

pose() writes one edit into the engine and the oracle from a state both
already share: the oracle through its DEBUG_* buffers and oracle_put_debug,
the engine through a snapshot whose sections are overwritten at the offsets
mpenv_state_section names.  The column-to-section table below restates k_debug
(csrc/hooks.hip) and is checked after every pose: before any step the engine's
debug gather and state exports must equal the oracle's bit for bit.

The case families (bots, combat, zone, movement, crumbs) are built from the
oracle and numpy alone, so tests/test_posed_states.py can show on the CPU that
every family reaches the branch it is meant for; tests/test_posed_states_gpu.py
runs the same families on both sides.

Nothing here is imported by the product.
"""
import functools
import os
import shutil
import tempfile

import numpy as np

import mpenv_testlib as T

# ------------------------------------------------------------ the column table
# k_debug's rows in order: debug column k of each export is the snapshot
# section (= DevState member) of that name.
AGENT_F32 = ["px", "py", "pz", "vx", "vy", "vz", "rw", "rx", "ry", "rz", "ayaw", "apitch", "aw", "ax", "ay", "az",
             "maxVel", "minDistZone", "firedT", "bcPenalty", "sx", "sy", "sz", "minDistSub"]
AGENT_I32 = ["curPose", "tgtPose", "transRem", "rngA", "rngB", "rngCtr", "landedOn", "respawnSteps",
             "autohealSteps", "flags", "wasShot", "weapon", "bcLast", "bcSteps", "visMask", "newCells"]
WORLD_I32 = ["teamA", "curStep", "finished", "curZone", "controlling", "contested", "captured", "earned",
             "zoneSteps", "stepsUntilPoint", "episode", "episodeCounter", "wRngA", "wRngB", "wRngCtr", "numCrumbs",
             "filtAct0", "filtAct1", "filtMatched0", "filtMatched1", "crumbOverflow", "subState"]
WORLD_F32 = ["teamRew0", "teamRew1", "goalMin0", "goalMin1", "goalTeam0", "goalTeam1"]
COLUMNS = {}
for _exp, _names in (("DEBUG_AGENT_F32", AGENT_F32), ("DEBUG_AGENT_I32", AGENT_I32),
                     ("DEBUG_WORLD_I32", WORLD_I32), ("DEBUG_WORLD_F32", WORLD_F32)):
    for _k, _n in enumerate(_names):
        COLUMNS[_n] = (_exp, _k)
# the debug column shows the low six bits of `flags`; visMask is a byte column
FLAG_BITS = 63
# state-backed exports: the oracle's export memory is its state, and the
# engine's snapshot section carries the export's name
STATE_EXPORTS = ["HP", "ALIVE", "MAGAZINE", "FWD_LIDAR", "AGENT_POLICY", "OPPONENT_LAST_KNOWN_OBSERVATIONS",
                 "OPPONENT_LAST_KNOWN_POSITIONS"]
# compared after a pose, before any step
POSE_CHECK = T.DEBUG_OUTPUTS + ["HP", "ALIVE", "MAGAZINE", "FWD_LIDAR", "AGENT_POLICY"]

MAX_CRUMBS = 128
DMG = np.float32(10.0)        # kDmgPerBullet
EPISODE_LEN = 3000            # kEpisodeLen
STAND, CROUCH, PRONE = 0, 1, 2


def sections(e):
    w, t, l = T.state_dims(e)
    out, k = {}, 0
    while True:
        sec = T.state_section(k, w, t, l)
        if sec is None:
            return out
        out[sec["name"]] = sec
        k += 1


def _blob_rw(e, blob, sec, dtype, fn):
    """Section `sec` of the snapshot at `blob` as rows of `dtype`: read, fn(rows), written back."""
    buf = np.empty(sec["bytes"], np.uint8)
    e.mem.d2h(blob + sec["offset"], buf.nbytes, buf)
    rows = buf.view(dtype).reshape(sec["bytes"] // sec["row_bytes"], -1)
    fn(rows)
    e.mem.h2d(blob + sec["offset"], buf)


def _pose_oracle(o, edits):
    o.lib.oracle_refresh_debug(o.h)
    for name, (rows, vals) in edits.items():
        if name in COLUMNS:
            exp, col = COLUMNS[name]
            o.view(exp)[rows, col] = vals
        elif name == "crumbs":
            o.view("DEBUG_CRUMBS")[rows] = vals
        else:
            assert name in STATE_EXPORTS, name
            v = o.view(name)
            v.reshape(v.shape[0], -1)[rows] = np.asarray(vals).reshape(-1, int(np.prod(v.shape[1:])))
    o.put_debug()


def _pose_engine(e, edits):
    sec = sections(e)
    blob = e.new_state_blob()
    try:
        e.state_save(blob)
        e.mem.hip.hipDeviceSynchronize()
        for name, (rows, vals) in edits.items():
            if name == "crumbs":
                # DEBUG_CRUMBS row {x, y, z, penalty, team, offset, id, 1} -> float4 pair
                # {x, y, z, penalty}, {team, offset, id's bits, 0}
                vals = np.asarray(vals, np.float32).reshape(-1, MAX_CRUMBS, 8)

                def put(r, vals=vals, rows=rows):
                    c = np.zeros((len(vals), MAX_CRUMBS, 8), np.float32)
                    c[:, :, :4] = vals[:, :, :4]
                    c[:, :, 4:6] = vals[:, :, 4:6]
                    c[:, :, 6] = vals[:, :, 6].astype(np.int32).view(np.float32)
                    c[vals[:, :, 7] == 0] = 0
                    r[rows] = c.reshape(len(vals), -1)
                _blob_rw(e, blob, sec["crumbs"], np.float32, put)
            elif name == "flags":
                def put(r, vals=vals, rows=rows):
                    r[rows, 0] = (r[rows, 0] & ~FLAG_BITS) | (np.asarray(vals, np.int32) & FLAG_BITS)
                _blob_rw(e, blob, sec[name], np.int32, put)
            elif name in COLUMNS:
                s = sec[name]
                dt = np.uint8 if s["row_bytes"] == 1 else (np.float32 if COLUMNS[name][0].endswith("F32") else np.int32)

                def put(r, vals=vals, rows=rows):
                    r[rows, 0] = vals
                _blob_rw(e, blob, s, dt, put)
            else:
                assert name in STATE_EXPORTS, name
                dt = e.desc(name)[1]

                def put(r, vals=vals, rows=rows):
                    r[rows] = np.asarray(vals).reshape(-1, r.shape[1])
                _blob_rw(e, blob, sec[name], dt, put)
        e.state_load(blob)
        assert e.state_error() == 0
        e.mem.hip.hipDeviceSynchronize()
    finally:
        e.mem.free(blob)


def check_pose(e, o, where):
    """The pose landed identically: every debug column and state export, bit for bit."""
    for n in POSE_CHECK:
        T.compare(e.get(n), o.get(n), f"{n} after the pose @ {where}")


def pose(e, o, edits, where="pose"):
    """The same edit on both sides.  edits: {column or export name: (rows, values)}; `rows` indexes
    agents or worlds (an index array or slice), `values` broadcasts over them.  "crumbs" takes whole
    DEBUG_CRUMBS rows [n, 128, 8] and goes with a "numCrumbs" edit.  e may be None (oracle alone)."""
    _pose_oracle(o, edits)
    if e is not None:
        _pose_engine(e, edits)
        check_pose(e, o, where)


def compare_step(e, o, where):
    # STEP_OUTPUTS holds the two action columns the bots write (PVP_DISCRETE_ACTION, PVP_AIM_ACTION)
    for n in T.STEP_OUTPUTS + T.DEBUG_OUTPUTS:
        T.compare(e.get(n), o.get(n), f"{n} @ {where}")
    T.compare(T.explore_visited(e), T.explore_visited(o), f"explore cells @ {where}")


# ------------------------------------------------------------ running a family
RECORDED = ["PVP_DISCRETE_ACTION", "PVP_AIM_ACTION", "HP", "ALIVE", "MAGAZINE", "DONE", "MATCH_RESULT",
            "DEBUG_AGENT_F32", "DEBUG_AGENT_I32", "DEBUG_WORLD_I32", "DEBUG_WORLD_F32"]


def snapshot(o):
    return {n: o.get(n) for n in RECORDED}


class Family:
    """cfg: Oracle / Engine keyword arguments; prep(sims, oracle) brings every side to the shared rollout
    state; rounds(o): yields (name, edits, acts6 or None, info) -- built from the oracle's state when
    the round starts, which is the engine's too."""

    def __init__(self, name, cfg, prep, rounds):
        self.name, self.cfg, self.prep, self.rounds = name, cfg, prep, rounds


def run_family(fam, engine=False, setup=None, after=None):
    """Rolls out, then per round: pose, two steps, compare after each (with an engine).  Returns a
    record per round: the oracle's outputs before the pose's first step and after each step.
    setup(engine) runs before init, after(engine) behind the last step."""
    o = T.Oracle(**fam.cfg)
    e = T.Engine(**fam.cfg) if engine else None
    sims = [s for s in (e, o) if s is not None]
    try:
        out = _run_rounds(fam, e, o, sims, setup)
        if after is not None and e is not None:
            after(e)
        return out
    finally:
        for s in sims:
            s.close()


def _run_rounds(fam, e, o, sims, setup):
    for s in sims:
        s.put_ctrl([0, 1, 1])
    if setup is not None and e is not None:
        setup(e)
    fam.prep(sims, o)
    if e is not None:
        compare_step(e, o, f"{fam.name}: rollout state")
    A = o.W * o.N
    out = []
    for name, edits, acts, info in fam.rounds(o):
        where = f"{fam.name}/{name}"
        pose(e, o, edits, where)
        rec = dict(name=name, info=info, posed=snapshot(o), steps=[])
        acts = np.zeros((A, 6), np.int32) if acts is None else np.asarray(acts, np.int32)
        for k in range(2):
            for s in sims:
                s.set_actions(acts)
                s.step()
            if e is not None:
                compare_step(e, o, f"{where} step {k + 1}")
            rec["steps"].append(snapshot(o))
        out.append(rec)
    return out


def tape_prep(steps, seed=1234):
    def prep(sims, o):
        A = o.W * o.N
        for s in sims:
            s.init()
        for k in range(steps):
            acts = T.mpenv_tape.tape_actions(seed, k, 0, A)
            for s in sims:
                s.set_actions(acts)
                s.step()
    return prep


def combat_prep(steps):
    def prep(sims, o):
        for s in sims:
            s.init()
        for k in range(steps):
            acts = T.seek_combat_actions(o, k)
            for s in sims:
                s.set_actions(acts)
                s.step()
    return prep


# ------------------------------------------------------------ navmesh in float64
@functools.lru_cache(maxsize=None)
def nav():
    """(tris [T,3,3] f64, astar [T,T], zone boxes [Z,6] f32, goal triangle per zone)"""
    o = T.Oracle(1, 1)
    tv, _, astar = o.navmesh()
    o.close()
    raw = open(os.path.join(T.SCENE, "zones.bin"), "rb").read()
    n = int(np.frombuffer(raw[:4], np.uint32)[0])
    boxes = np.frombuffer(raw[4:4 + 24 * n], np.float32).reshape(n, 6).copy()
    tris = tv.astype(np.float64)
    # the goal lookup sees the centre's own z (the bot's position goes in with z = 0)
    goals = [nearest_nav_tri(tris, zone_centre(boxes, z, xy=False))[0] for z in range(n)]
    return tris, astar, boxes, goals


def zone_centre(boxes, z, xy=True):
    """(pMin + pMax) / 2 in f32, as planAStar forms it."""
    b = boxes[z]
    c = ((b[:3] + b[3:]) / np.float32(2)).astype(np.float64)
    return c[:2] if xy else c


def nearest_nav_tri(tris, pos):
    """NearestNavTri restated in float64: (triangle, found by containment)."""
    e = np.roll(tris, -1, axis=1) - tris
    vp = pos[None, None, :] - tris
    cz = e[:, :, 0] * vp[:, :, 1] - e[:, :, 1] * vp[:, :, 0]
    gtz = cz > 0
    inside = np.flatnonzero((gtz[:, 0] == gtz[:, 1]) & (gtz[:, 1] == gtz[:, 2]))
    if len(inside):
        return int(inside[0]), True
    # the fallback's bookkeeping, in the reference's order (`closest` ends up holding |c.z|)
    closest, idx = np.inf, -1
    for t in range(len(tris)):
        for k in range(3):
            d2 = float(np.dot(vp[t, k], vp[t, k]))
            if d2 < closest:
                perp = vp[t, k] * (-np.dot(e[t, k], vp[t, k]) / np.dot(e[t, k], e[t, k])) + e[t, k]
                if float(np.dot(perp, perp)) < closest:
                    closest, idx = abs(cz[t, k]), t
    return idx, False


def classify(pos_xy, zone):
    return _classify(float(pos_xy[0]), float(pos_xy[1]), int(zone))


@functools.lru_cache(maxsize=None)
def _classify(x, y, zone):
    """(start triangle, by containment, hop kind, target xy) of a bot at pos_xy heading for `zone`;
    hop kind is "none" (table entry -1), "goal" or "hop"."""
    tris, astar, boxes, goals = nav()
    start, inside = nearest_nav_tri(tris, np.array([x, y, 0.0]))
    nxt = int(astar[start, goals[zone]])
    if nxt == -1:
        return start, inside, "none", np.zeros(2)
    if nxt == goals[zone]:
        return start, inside, "goal", zone_centre(boxes, zone)
    return start, inside, "hop", tris[nxt].mean(0)[:2]


def yaw_towards(pos_xy, tgt_xy, turn=0.0):
    """The yaw whose forward (-sin, cos) points from pos to tgt, turned by `turn`."""
    d = np.asarray(tgt_xy, np.float64) - np.asarray(pos_xy, np.float64)
    return np.arctan2(-d[0], d[1]) + turn


def ulps(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf))
    return x


def oracle_sin(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    T.lib_oracle().oracle_eval_math(0, T.fptr(x), T.fptr(x), T.fptr(out), len(x))
    return out


@functools.lru_cache(maxsize=None)
def yaws_at_dot_06():
    """{0: a yaw whose forward x, -sinf_(yaw), is exactly 0.6f by the shared sine; 1 / -1: the nearest
    yaws whose forward x is the next float above / below}.  With the target due +x at a power-of-two
    distance the bot's dot product is that number: the `> 0.6f` threshold and its two neighbours."""
    y0 = np.float32(-np.arcsin(0.6))
    cand = np.array([ulps(y0, k) for k in range(-64, 65)], np.float32)
    fx = -oracle_sin(cand)
    t = np.float32(0.6)
    out = {}
    for n, want in ((0, t), (1, np.nextafter(t, np.float32(1))), (-1, np.nextafter(t, np.float32(0)))):
        hit = np.flatnonzero(fx == want)
        assert len(hit), f"no yaw near -asin(0.6) has -sinf_(yaw) == {want!r}"
        out[n] = cand[hit[len(hit) // 2]]
    return out


# ------------------------------------------------------------ the bot family
BOT_CFG = dict(num_worlds=13, team_size=6)
NO_WALL = np.float32(100.0)
BELOW_16 = np.nextafter(np.float32(16.0), np.float32(0.0))


def _lidar(A, cols=None):
    """FWD_LIDAR rows [A, 2, 32, 4] with every depth 100 (no wall); cols[g] = [(row, column, depth)]."""
    l = np.zeros((A, 2, 32, 4), np.float32)
    l[..., 0] = NO_WALL
    for g, hits in (cols or {}).items():
        for y, x, d in hits:
            l[g, y, x, 0] = d
    return l


def _bot_round(name, o, pos, yaw, zone_of_world, lidar=None, mag=None, vis=None, info=None):
    A = o.W * o.N
    rows = slice(None)
    pos = np.asarray(pos, np.float32)
    edits = {
        "AGENT_POLICY": (rows, np.full((A, 1), -1, np.int32)),
        "px": (rows, pos[:, 0]), "py": (rows, pos[:, 1]),
        "vx": (rows, np.float32(0)), "vy": (rows, np.float32(0)),
        "ayaw": (rows, np.asarray(yaw, np.float32)),
        "curZone": (rows, np.asarray(zone_of_world, np.int32)),
        "FWD_LIDAR": (rows, _lidar(A) if lidar is None else lidar),
        "HP": (rows, np.full((A, 1), 100, np.float32)), "ALIVE": (rows, np.ones((A, 1), np.float32)),
    }
    if mag is not None:
        edits["MAGAZINE"] = (rows, mag)
    if vis is not None:
        edits["visMask"] = (rows, vis)
    return name, edits, None, info


YAW_TURNS = ["toward", "away", "in+", "in-", "out+", "out-", "left", "right"]


def _yaw_pattern(k, pos_xy, tgt_xy):
    """Agent k's yaw: exactly at / away from the target, a few ulps either side of the 0.6 cone
    on both flanks, and square to it on either hand."""
    c = np.arccos(0.6)
    kind = YAW_TURNS[k % len(YAW_TURNS)]
    if kind == "toward":
        return np.float32(yaw_towards(pos_xy, tgt_xy))
    if kind == "away":
        return np.float32(yaw_towards(pos_xy, tgt_xy, np.pi))
    if kind in ("left", "right"):
        return np.float32(yaw_towards(pos_xy, tgt_xy, np.pi / 2 if kind == "left" else -np.pi / 2))
    side = 1 if kind[-1] == "+" else -1
    base = np.float32(yaw_towards(pos_xy, tgt_xy, side * c))
    # inside the cone: towards the target by 1-3 ulps; outside: away from it
    n = 1 + (k // len(YAW_TURNS)) % 3
    return ulps(base, -side * n if kind.startswith("in") else side * n)


def bot_positions():
    """{round: [156, 2] f64}: triangle centroids; edge midpoints and vertices; 0.5 and 50 units
    outside the mesh's bounding box."""
    tris = nav()[0]
    T_ = len(tris)
    idx = np.arange(156) % T_
    cen = tris[idx].mean(1)[:, :2]
    k3 = np.arange(156) % 3
    edge = 0.5 * (tris[idx, k3] + tris[idx, (k3 + 1) % 3])[:, :2]
    vert = tris[idx, k3][:, :2]
    shared = np.where((np.arange(156) % 2 == 0)[:, None], edge, vert)
    lo, hi = tris[:, :, :2].reshape(-1, 2).min(0), tris[:, :, :2].reshape(-1, 2).max(0)
    out = np.zeros((156, 2))
    for k in range(156):
        d = 0.5 if k % 2 == 0 else 50.0
        t = (k // 8) / 19.0  # along the side
        side = (k // 2) % 4
        x = lo[0] + t * (hi[0] - lo[0])
        y = lo[1] + t * (hi[1] - lo[1])
        out[k] = [(x, lo[1] - d), (x, hi[1] + d), (lo[0] - d, y), (hi[0] + d, y)][side]
    return dict(centroid=cen, shared=shared, outside=out)


def bot_rounds(o):
    tris, astar, boxes, goals = nav()
    A, N, W = o.W * o.N, o.N, o.W
    P = bot_positions()

    def plan(pos, zones):
        cls = [classify(pos[g], zones[g // N]) for g in range(A)]
        yaw = [_yaw_pattern(g, pos[g], cls[g][3]) for g in range(A)]
        return cls, np.array(yaw, np.float32)

    # one round per zone from the centroids; every tenth bot sees an opponent, every
    # twentieth of them with an empty magazine (reload beats fire)
    for z in range(len(boxes)):
        zones = np.full(W, z, np.int32)
        cls, yaw = plan(P["centroid"], zones)
        vis = np.where(np.arange(A) % 10 == 0, 1, 0).astype(np.int32)
        mag = np.tile(np.array([[30, 0]], np.int32), (A, 1))
        mag[np.arange(A) % 20 == 0, 0] = 0
        yield _bot_round(f"centroids zone {z}", o, P["centroid"], yaw, zones, mag=mag, vis=vis,
                         info=dict(kind="nav", cls=cls, vis=vis, mag=mag[:, 0].copy()))
    for nm in ("shared", "outside"):
        zones = (np.arange(W) % len(boxes)).astype(np.int32)
        cls, yaw = plan(P[nm], zones)
        yield _bot_round(f"{nm} points", o, P[nm], yaw, zones, info=dict(kind="nav", cls=cls))

    # exactly at the zone centre (normalize of a zero vector), and due -x of it at power-of-two
    # distances with the yaw one ulp either side of, and exactly on, dot == 0.6f
    zones = (np.arange(W) % len(boxes)).astype(np.int32)
    y06 = yaws_at_dot_06()
    pos = np.zeros((A, 2))
    yaw = np.zeros(A, np.float32)
    exact = {}
    for g in range(A):
        c = zone_centre(boxes, zones[g // N])
        i = g % N
        if i < 3:
            pos[g] = c
            yaw[g] = np.float32([0.0, 1.0, -2.5][i])
        else:
            d = [64.0, 32.0, 16.0][(i // 3) % 3]
            pos[g] = c - [d, 0.0]
            # the target must be the zone centre itself and the difference exact
            assert np.float32(c[0]) - np.float32(pos[g][0]) == np.float32(d)
            if classify(pos[g], zones[g // N])[2] == "goal":
                n = i % 3 - 1  # dot one float below 0.6f, on it, one above
                yaw[g] = y06[n]
                exact[g] = n
    cls = [classify(pos[g], zones[g // N]) for g in range(A)]
    yield _bot_round("zone centre and dot == 0.6", o, pos, yaw, zones, info=dict(kind="exact", cls=cls, exact=exact))

    # wall avoidance: the mean hit column in every case of the switch and on its boundaries
    cols, want = {}, {}
    for g in range(A):
        y = (g // 32) % 2
        if g < 64:                       # one hit at column g % 32, either row
            cols[g], want[g] = [(y, g % 32, np.float32(3.0))], float(g % 32)
        elif g < 96:                     # two hits, means k + 0.5 .. (row 0 and row 1)
            x = g - 64
            cols[g], want[g] = [(0, x, np.float32(15.0)), (1, min(x + 1, 31), BELOW_16)], (x + min(x + 1, 31)) / 2
        elif g < 104:                    # means exactly 4, 12, 20, 28 from two columns
            m = [4, 12, 20, 28][(g - 96) % 4]
            cols[g], want[g] = [(0, m - 3, np.float32(0.0)), (1, m + 3, np.float32(8.0))], float(m)
        elif g < 112:                    # 16.0f is no hit: alone -> no wall; beside a hit -> ignored
            x = [2, 9, 18, 30][(g - 104) % 4]
            if g < 108:
                cols[g], want[g] = [(0, x, np.float32(16.0))], None
            else:
                cols[g], want[g] = [(0, 16 if x != 18 else 3, np.float32(16.0)), (1, x, BELOW_16)], float(x)
        else:
            want[g] = None               # no wall
    zones = (np.arange(W) % len(boxes)).astype(np.int32)
    cls, yaw = plan(P["centroid"], zones)
    yield _bot_round("wall avoidance", o, P["centroid"], yaw, zones, lidar=_lidar(A, cols),
                     info=dict(kind="wall", cls=cls, mean=want))


BOTS = Family("bots", BOT_CFG, tape_prep(3), bot_rounds)


# ------------------------------------------------------------ the combat family
COMBAT_CFG = dict(num_worlds=5, team_size=3, sim_flags=1)
COMBAT_STEPS = 40


def combat_rounds(o):
    """Per world a pair (a of team 0 sees b of team 1) from the rollout state; b is moved onto the
    sight line at short range and both are turned to face each other, then hp, magazines, timers
    and poses are edited: the worlds with such a pair take the scenarios in turn, round after round."""
    N, W, ts = o.N, o.W, o.N // 2
    A = W * N
    af = o.get("DEBUG_AGENT_F32")
    ai = o.get("DEBUG_AGENT_I32")
    alive = o.get("ALIVE").reshape(-1)
    pairs = {}
    for w in range(W):
        for a in range(ts):
            ga = w * N + a
            seen = [k for k in range(ts) if (ai[ga, 14] >> k) & 1 and alive[ga] and alive[w * N + ts + k]]
            if seen:
                pairs[w] = (ga, w * N + ts + seen[0])
                break
    assert pairs, "no world of the rollout state has an agent that sees an opponent"
    geo = {}
    for w, (ga, gb) in pairs.items():
        pa, pb = af[ga, :3].astype(np.float64), af[gb, :3].astype(np.float64)
        d = pb - pa
        dist = np.linalg.norm(d[:2])
        u = d / dist
        geo[w] = dict(a=ga, b=gb, pa=pa, pb=pa + u * min(80.0, dist), u=u,
                      a2=w * N + (ga - w * N + 1) % ts, side=np.array([-u[1], u[0], 0.0]))
    NSC = 10
    for r in range((NSC + len(geo) - 1) // len(geo)):
        cols = {k: {} for k in ("px", "py", "pz", "vx", "vy", "vz", "ayaw", "apitch", "curPose", "tgtPose",
                                "transRem", "respawnSteps", "autohealSteps")}
        hp, mag = {}, {}
        acts = np.zeros((A, 6), np.int32)
        acts[:, 4], acts[:, 5] = 6, 3  # no discrete turn
        info = {}
        for k, (w, G) in enumerate(sorted(geo.items())):
            sc = (r * len(geo) + k) % NSC
            a, b, a2 = G["a"], G["b"], G["a2"]
            place = {a: G["pa"], b: G["pb"]}
            face = {a: b, b: a}
            acts[a, 2] = acts[b, 2] = 1
            hp[a] = hp[b] = np.float32(100)
            mag[a] = mag[b] = (30, 0)
            if sc == 0:      # exact damage on both sides: a mutual kill
                hp[a] = hp[b] = DMG
            elif sc == 1:    # one ulp above a shot's damage survives it
                hp[a], hp[b] = DMG, ulps(DMG, 1)
            elif sc == 2:    # two shooters on one target: 20 hp gone in one step
                place[a2] = G["pa"] + 30.0 * G["side"]
                face[a2] = b
                acts[a2, 2] = 1
                hp[a2], mag[a2], hp[b] = np.float32(100), (30, 0), np.float32(20)
            elif sc == 3:    # the last round, then an empty magazine; the other side reloads
                mag[a], mag[b] = (1, 0), (0, 0)
                acts[b, 2] = 2
            elif sc == 4:    # timers at 1: b is invincible for this step, a heals on the next
                cols["respawnSteps"][b] = 1
                cols["autohealSteps"][a] = 1
                hp[a] = np.float32(50)
                acts[b, 2] = 0
            elif sc == 5:    # autoheal due on the step, up to the cap
                cols["autohealSteps"][a] = 0
                cols["autohealSteps"][b] = 0
                hp[a], hp[b] = np.float32(97), np.float32(40)
                acts[a, 2] = acts[b, 2] = 0
            elif sc == 6:    # a prone target
                cols["curPose"][b] = cols["tgtPose"][b] = PRONE
                cols["transRem"][b] = 0
            elif sc == 7:    # a crouched target with hp of exactly one shot
                cols["curPose"][b] = cols["tgtPose"][b] = CROUCH
                cols["transRem"][b] = 0
                hp[b] = DMG
            elif sc == 8:    # a teammate on the line of fire
                place[a2] = 0.5 * (G["pa"] + G["pb"])
                face[a2] = b
                hp[a2], mag[a2] = np.float32(100), (30, 0)
            else:            # magazine 1 -> 0 on a killing shot, reload on an empty one
                mag[a], hp[b] = (1, 0), DMG
                acts[b, 2] = 0
            for g, p in place.items():
                cols["px"][g], cols["py"][g], cols["pz"][g] = np.float32(p[0]), np.float32(p[1]), np.float32(p[2])
                cols["vx"][g] = cols["vy"][g] = cols["vz"][g] = np.float32(0)
                cols["apitch"][g] = np.float32(0)
                cols["respawnSteps"].setdefault(g, 0)
            for g, at in face.items():
                cols["ayaw"][g] = np.float32(yaw_towards(place[g][:2], place[at][:2]))
            info[w] = dict(scenario=sc, a=a, b=b, a2=a2)
        edits = {}
        for nm, d in cols.items():
            if d:
                g = np.array(sorted(d))
                dt = np.float32 if COLUMNS[nm][0].endswith("F32") else np.int32
                edits[nm] = (g, np.array([d[k] for k in g], dt))
        g = np.array(sorted(hp))
        edits["HP"] = (g, np.array([hp[k] for k in g], np.float32).reshape(-1, 1))
        edits["ALIVE"] = (g, np.ones((len(g), 1), np.float32))
        g = np.array(sorted(mag))
        edits["MAGAZINE"] = (g, np.array([mag[k] for k in g], np.int32))
        yield f"scenarios round {r}", edits, acts, dict(kind="combat", worlds=info)


COMBAT = Family("combat", COMBAT_CFG, combat_prep(COMBAT_STEPS), combat_rounds)


# ------------------------------------------------------------ the zone family
_tmp = None
ZONE_ROT = np.array([0.3, -0.7, 0.5], np.float32)


@functools.lru_cache(maxsize=None)
def rotated_zone_scene():
    """simple_map with its three zones rotated about z (zones.bin's rotation column); the boxes,
    and so the zone centres, stay."""
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="mpenv_posed_")
    d = os.path.join(_tmp.name, "rotated_zones")
    os.makedirs(d, exist_ok=True)
    for f in ("collisions.bin", "navmesh.bin", "spawns.bin"):
        shutil.copy(os.path.join(T.SCENE, f), d)
    raw = open(os.path.join(T.SCENE, "zones.bin"), "rb").read()
    n = int(np.frombuffer(raw[:4], np.uint32)[0])
    assert n == len(ZONE_ROT)
    with open(os.path.join(d, "zones.bin"), "wb") as f:
        f.write(raw[:4 + 24 * n])
        f.write(ZONE_ROT.tobytes())
    return d


def zone_point(z, fx, fy, rot):
    """The world xy of the point at fractions (fx, fy) of zone z's rotated box: 0 and 1 are its faces.
    zoneSystem rotates the box's corners and the agent by the inverse rotation."""
    b = nav()[2][z].astype(np.float64)
    c, s = np.cos(-rot[z]), np.sin(-rot[z])
    R = np.array([[c, -s], [s, c]])              # world -> zone frame
    lo, hi = R @ b[0:2], R @ b[3:5]
    p = np.array([lo[0] + fx * (hi[0] - lo[0]), lo[1] + fy * (hi[1] - lo[1])])
    return R.T @ p


def zone_rounds(rot):
    def rounds(o):
        N, W, ts = o.N, o.W, o.N // 2
        A = W * N
        Z = len(rot)
        for z in range(Z):
            inside = zone_point(z, 0.5, 0.5, rot)
            far = zone_point(z, 3.0, 3.0, rot)
            pos = np.tile(far, (A, 1))
            wi = {k: np.zeros(W, np.int32) for k in ("curStep", "controlling", "contested", "captured",
                                                     "zoneSteps", "stepsUntilPoint")}
            wi["curStep"][:] = 100
            wi["controlling"][:] = -1
            wi["zoneSteps"][:] = 300
            wi["stepsUntilPoint"][:] = 10
            rew = np.zeros((W, 2), np.float32)
            # world 0: team 0 holds the zone, its last step: the zone changes
            pos[0 * N + 0] = inside
            wi["controlling"][0], wi["zoneSteps"][0] = 0, 1
            # world 1: team 1 holds it, a point is due: earned, and the capture
            pos[1 * N + ts] = inside
            wi["controlling"][1], wi["stepsUntilPoint"][1] = 1, 1
            # world 2: the episode's last step, team rewards equal
            wi["curStep"][2] = EPISODE_LEN - 1
            rew[2] = 0.25
            pos[2 * N + 1] = inside
            # world 3: contested, one head each, both counters at 1
            pos[3 * N + 0] = inside
            pos[3 * N + ts] = zone_point(z, 0.25, 0.75, rot)
            wi["controlling"][3], wi["zoneSteps"][3], wi["stepsUntilPoint"][3] = 0, 1, 1
            # world 4: on the faces and corners of the box
            marks = [(0, 0.5), (1, 0.5), (0.5, 0), (0.5, 1), (0, 0), (1, 1)]
            for i in range(N):
                pos[4 * N + i] = zone_point(z, *marks[i % len(marks)], rot)
            wi["controlling"][4] = 1
            rows = slice(None)
            edits = {k: (rows, v) for k, v in wi.items()}
            edits.update({
                "curZone": (rows, np.full(W, z, np.int32)),
                "px": (rows, pos[:, 0].astype(np.float32)), "py": (rows, pos[:, 1].astype(np.float32)),
                "vx": (rows, np.float32(0)), "vy": (rows, np.float32(0)),
                "teamRew0": (rows, rew[:, 0]), "teamRew1": (rows, rew[:, 1]),
                "HP": (rows, np.full((A, 1), 100, np.float32)), "ALIVE": (rows, np.ones((A, 1), np.float32)),
            })
            yield f"zone {z}", edits, None, dict(kind="zone", zone=z)
    return rounds


def zone_family(auto_reset=True, rotated=True):
    rot = ZONE_ROT if rotated else np.zeros(3, np.float32)
    cfg = dict(num_worlds=5, team_size=3, auto_reset=auto_reset)
    if rotated:
        cfg["scene"] = rotated_zone_scene()
    return Family(f"zone{'' if auto_reset else '_noreset'}{'_rot' if rotated else ''}", cfg, tape_prep(5),
                  zone_rounds(rot))


# ------------------------------------------------------------ movement and crumbs
def move_rounds(o):
    N, W = o.N, o.W
    A = W * N
    af = o.get("DEBUG_AGENT_F32")
    acts = np.zeros((A, 6), np.int32)
    acts[:, 4], acts[:, 5] = 6, 3
    g = np.arange(A)
    # world 0: a pose transition's last step with another pose asked for
    acts[0, 3], acts[1, 3] = PRONE, CROUCH
    # world 1: at top speed, pushing on / turning across
    acts[N:2 * N, 0] = 2
    acts[N + 1, 1] = 2
    # world 2: 30 units above the floor, and falling while moving
    acts[2 * N + 1, 0] = 2
    vmax = af[:, 16]
    yaw = af[:, 10].astype(np.float64)
    vx, vy = af[:, 3].copy(), af[:, 4].copy()
    w1 = slice(N, 2 * N)
    vx[w1] = (-np.sin(yaw[w1]) * vmax[w1]).astype(np.float32)
    vy[w1] = (np.cos(yaw[w1]) * vmax[w1]).astype(np.float32)
    vx[N] = vmax[N]  # exactly maxVel along x
    vy[N] = 0
    pz = af[:, 2].copy()
    pz[2 * N:3 * N] += np.float32(30)
    cur = np.zeros(A, np.int32)
    tgt = np.zeros(A, np.int32)
    tr = np.zeros(A, np.int32)
    cur[0:N], tgt[0:N], tr[0:N] = STAND, CROUCH, 1
    edits = {"vx": (g, vx), "vy": (g, vy), "pz": (g, pz), "curPose": (g, cur), "tgtPose": (g, tgt),
             "transRem": (g, tr), "HP": (g, np.full((A, 1), 100, np.float32)),
             "ALIVE": (g, np.ones((A, 1), np.float32))}
    yield "transition, top speed, fall", edits, acts, dict(kind="move")


MOVE = Family("move", dict(num_worlds=3, team_size=1), tape_prep(5), move_rounds)


def crumb_rounds(o):
    N, W = o.N, o.W
    A = W * N
    ts = N // 2
    c = np.zeros((W, MAX_CRUMBS, 8), np.float32)
    n = MAX_CRUMBS - 1
    k = np.arange(n)
    c[:, :n, 0] = 5000.0 + 40.0 * k  # far from every agent
    c[:, :n, 1] = 5000.0
    c[:, :n, 3] = 1.0
    c[:, :n, 4] = k % 2
    c[:, :n, 5] = k % ts
    c[:, :n, 6] = 1000 + k           # ids clear of the rollout's counter
    c[:, :n, 7] = 1.0
    # world 1: the oldest crumbs expire on the step, making room again
    c[1, :4, 3] = 0.025
    rows = slice(None)
    edits = {"crumbs": (rows, c), "numCrumbs": (rows, np.full(W, n, np.int32)),
             "bcSteps": (rows, np.full(A, 10, np.int32)), "bcLast": (rows, np.full(A, -1, np.int32)),
             "HP": (rows, np.full((A, 1), 100, np.float32)), "ALIVE": (rows, np.ones((A, 1), np.float32))}
    yield "pool one short", edits, None, dict(kind="crumbs")


CRUMBS = Family("crumbs", dict(num_worlds=5, team_size=3), tape_prep(5), crumb_rounds)
