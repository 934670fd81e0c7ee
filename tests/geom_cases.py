"""Seeded inputs for the query-level geometry tests (tests/test_geom_cases.py
on the CPU, tests/test_geom_queries_gpu.py on the device): rays, sight /
world-ray families with capsules placed on the thresholds of the device's
culls, occluder hints, sphere casts and stuck-fallback waves.  Everything is
a deterministic function of the seeds below; both test files use every
generator, so the conditions test_geom_cases.py asserts on these inputs hold
for what the GPU test compares.

Helpers here restate, on the CPU: the device's three capsule culls in
float64 (geom_dev.h capsulesD / visibleFullD), a float64 line-of-sight
answer (Moller-Trumbore over every triangle and an analytic vertical
capsule), and the stuck fallback's four casts (sim.cpp:962-984) in float32
numpy over the oracle's sin / cos and sphere cast."""
import ctypes as C
import functools
import os
import sys

import numpy as np

import mpenv_testlib as T
import test_quirk_grid as Q

sys.path.insert(0, os.path.join(T.ROOT, "tools"))
from dump_lidar_rays import rays_for  # noqa: E402

F32 = np.float32
R = 15.0          # consts::agentRadius = the capsule radius
SEG = 35.0        # standHeight - 2 r, the capsule's segment
CULL_R = 15.0 * 1.01
KFLT_MAX = F32(np.finfo(np.float32).max)
NUDGES = np.arange(-8, 9)
FAR_NUDGES = (-(1 << 15), 1 << 15)  # clearly in front of / inside the wall: decisive in float64
DELTAS = (0.0, 1e-6, -1e-6, 1e-3, -1e-3, 0.0099, 0.0101, 0.02)
EPS = (1e-4, -1e-4, 1e-2, -1e-2)


@functools.lru_cache(maxsize=None)
def oracle():
    """One shared oracle (2 worlds, 6v6): its query hooks take caller inputs
    and do not depend on its state, which rays() steps for the lidar fans."""
    o = T.Oracle(2, 6)
    o.put_ctrl([0, 1, 1])
    o.init()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    o.lib.oracle_trace_world_batch.argtypes = [C.c_void_p, C.c_int32, fp, fp, fp, C.c_int32, ip, fp, ip]
    o.lib.oracle_capsule_batch.argtypes = [C.c_int32, fp, fp, C.c_float, C.c_float, fp]
    return o


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def trace(org, d, order=0):
    """oracle_trace_ray_batch: (t, hit); order 0 slot order on the collision
    tree, 1 octant order on the lidar tree."""
    o = oracle()
    n = len(org)
    org, d = np.ascontiguousarray(org, F32), np.ascontiguousarray(d, F32)
    t, h = np.zeros(n, F32), np.zeros(n, np.int32)
    o.lib.oracle_trace_ray_batch(o.h, n, T.fptr(org), T.fptr(d), order, T.fptr(t), h.ctypes.data)
    return t, h


def trace_world(org, d, caps):
    """oracle_trace_world_batch: (hit, t, entity); caps [n][N][3]."""
    o = oracle()
    n, N = caps.shape[:2]
    org, d, caps = (np.ascontiguousarray(a, F32) for a in (org, d, caps))
    hit, ent, t = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, F32)
    o.lib.oracle_trace_world_batch(o.h, n, T.fptr(org), T.fptr(d), T.fptr(caps), N,
                                   hit.ctypes.data_as(C.POINTER(C.c_int32)), T.fptr(t),
                                   ent.ctypes.data_as(C.POINTER(C.c_int32)))
    return hit, t, ent


def capsule_t(org, d, base):
    """intersectRayZOriginCapsule as traceRayAgainstWorld calls it, per ray
    (float32)."""
    lib = oracle().lib
    out = np.zeros(len(org), F32)
    co = np.array(base, F32)
    co[:, 2] += F32(R)
    tr = np.ascontiguousarray(np.asarray(org, F32) - co, F32)
    d = np.ascontiguousarray(d, F32)
    lib.oracle_capsule_batch(len(org), T.fptr(tr), T.fptr(d), F32(R), F32(SEG), T.fptr(out))
    return out


# ------------------------------------------------------------------- rays
def _rollout_fans():
    """Lidar fans (tools/dump_lidar_rays.rays_for) after 16 tape steps and
    after 16 more steps under the combat aim-bot."""
    o = oracle()
    out = []
    for s in range(32):
        o.set_actions(T.seek_combat_actions(o, s) if s >= 16 else T.mpenv_tape.tape_actions(1234, s, 0, o.W * 12))
        o.step()
        if s % 16 == 15:
            out.append(rays_for(o.get("DEBUG_AGENT_F32"), o.get("DEBUG_AGENT_I32")))
    r = np.concatenate(out)
    return r[:, :3], r[:, 3:]


def _signed_zero_variants(d, zero):
    """Each row of d once per sign pattern of its zero components (zero: bool
    mask of the components that are exactly 0), +0 and -0."""
    out = []
    for pat in range(8):
        s = np.array([(pat >> k) & 1 for k in range(3)], bool)
        use = (~s[None, :] | zero).all(1)  # only patterns that flip zero components
        v = d[use].copy()
        v[:, s] = np.where(v[:, s] == 0, F32(-0.0), v[:, s])
        out.append((v, use))
    return out


@functools.lru_cache(maxsize=None)
def rays():
    """(org, d, first index of the signed-zero block): rays aimed at every
    vertex and edge midpoint from 40 origins, lidar fans of a tape and a
    combat rollout, axis-parallel and near-axis directions with every zero
    component once +0 and once -0, and directions with one tiny component."""
    _, verts, _ = T.scene_bvh()
    rng = np.random.default_rng(101)
    eo, ed = T.edge_aimed_rays(verts, 40, 12)
    fo, fd = _rollout_fans()
    v3 = verts.reshape(-1, 3)
    # origins for the axis rays: in the map, and on vertices' own coordinates
    # (an axis-parallel ray then runs along box faces and triangle edges)
    base_o = np.concatenate([rng.uniform([-1500, -1500, -50], [1500, 1500, 300], (120, 3)),
                             v3[rng.integers(0, len(v3), 60)] + np.array([0.0, 0.0, 20.0]),
                             v3[rng.integers(0, len(v3), 20)]]).astype(F32)
    dirs, zeros = [], []
    for ax in range(3):
        for sg in (1.0, -1.0):
            e = np.zeros(3, F32)
            e[ax] = sg
            dirs.append(e)
            zeros.append(e == 0)
            for other in range(3):  # near-axis: one more component, the third exactly 0
                if other == ax:
                    continue
                for small in (1e-3, -1e-3, 0.25):
                    v = np.zeros(3)
                    v[ax], v[other] = sg, small
                    v = (v / np.linalg.norm(v)).astype(F32)
                    dirs.append(v)
                    zeros.append(v == 0)
    dirs, zeros = np.array(dirs, F32), np.array(zeros)
    zo, zd = [], []
    for v, use in _signed_zero_variants(dirs, zeros):
        zo.append(np.repeat(base_o, len(v), axis=0))
        zd.append(np.tile(v, (len(base_o), 1)))
    zo, zd = np.concatenate(zo), np.concatenate(zd)
    # one component of magnitude 1e-8 .. 1e-4
    m = 6000
    td = _unit(rng.normal(size=(m, 3)))
    k = rng.integers(0, 3, m)
    td[np.arange(m), k] = 0
    td = _unit(td)
    td[np.arange(m), k] = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-8, -4, m)
    to = rng.uniform([-1500, -1500, -50], [1500, 1500, 300], (m, 3))
    org = np.concatenate([eo, fo, zo, to]).astype(F32)
    d = np.concatenate([ed, fd, zd, td]).astype(F32)
    z0 = len(eo) + len(fo)
    return org, d, (z0, z0 + len(zo))


# --------------------------------------------------- sight / world families
def _nudge(x, k):
    """x moved by k ulps (float32 arrays; x != 0 and far from 0)."""
    b = x.astype(F32).view(np.int32)
    return np.where(x >= 0, b + k, b - k).astype(np.int32).view(F32)


ANCHOR_TOL = 2e-6


def _base_rays(rng, n_free, n_aimed):
    """Near-horizontal rays (|pitch| <= 0.3) with a triangle hit at 40 < t <
    2000: random ones, half of them exactly horizontal, and rays aimed at
    vertices and edge midpoints (from the target's own height: d.z == 0, or
    from another height).  A ray is used only if the float64 restatement
    reproduces the oracle's hit distance on some triangle (widened by
    EDGE_SLACK) to ANCHOR_TOL t, a fifth of the 1e-5 t to which the sight test
    checks a recorded occluder in float64: the watertight test interpolates t
    from the vertices' depths, and on a long sliver crossed obliquely (the
    floor slab's 3,937 x 0.79 edge triangles) float32 is off by up to 2.4e-4
    t, so on those rays neither "the capsule is entered where the triangle is
    hit" nor that check means anything.  (Their closest hits are compared
    bit for bit by the ray tests.)"""
    _, verts, _ = T.scene_bvh()
    org = rng.uniform([-1500, -1500, 20], [1500, 1500, 90], (n_free, 3))
    ang = rng.uniform(0, 2 * np.pi, n_free)
    pitch = np.where(rng.integers(0, 2, n_free) == 0, 0.0, rng.uniform(-0.3, 0.3, n_free))
    d = np.stack([np.cos(ang) * np.cos(pitch), np.sin(ang) * np.cos(pitch), np.sin(pitch)], 1)
    tris = verts.reshape(-1, 3, 3).astype(np.float64)
    targets = np.concatenate([tris.reshape(-1, 3), 0.5 * (tris[:, 0] + tris[:, 1]),
                              0.5 * (tris[:, 1] + tris[:, 2]), 0.5 * (tris[:, 2] + tris[:, 0])])
    tg = targets[rng.integers(0, len(targets), n_aimed)]
    ao = tg + np.stack([rng.uniform(-900, 900, n_aimed), rng.uniform(-900, 900, n_aimed),
                        np.where(rng.integers(0, 2, n_aimed) == 0, 0.0, rng.uniform(-40, 40, n_aimed))], 1)
    ao = ao.astype(F32).astype(np.float64)
    ad = tg - ao
    keep = np.linalg.norm(ad[:, :2], axis=1) > 60
    ao, ad = ao[keep], _unit(ad[keep])
    keep = np.abs(np.arcsin(ad[:, 2])) <= 0.3
    org = np.concatenate([org, ao[keep]]).astype(F32)
    d = np.concatenate([_unit(d), ad[keep]]).astype(F32)
    t, h = trace(org, d)
    ok = (h == 1) & (t > 40) & (t < 2000)
    org, d, t = org[ok], d[ok], t[ok]
    loose = tri_hits64(org, d, verts, (EDGE_SLACK,))[0]
    ok = np.abs(loose - t.astype(np.float64)[:, None]).min(1) <= ANCHOR_TOL * t
    return org[ok], d[ok], t[ok]


N_KINDS = 18


def _other_capsules(kind, org, d, t_tri, rng):
    """Bases [F][11][3] of the non-target capsules of F rays (float64), kind
    [F][11]: each on a cull's threshold for its ray (org, d) with triangle
    hit t_tri: kinds 0-7 the xy-distance cull at r (1 + DELTAS[kind]); 8-11
    the behind-the-origin cull at EPS[kind - 8]; 12-15 the beyond-the-hit cull
    at EPS[kind - 12]; 16 origin inside the capsule; 17 origin on its axis."""
    F, S = kind.shape
    o, dd, tt = org[:, None, :], d[:, None, :], t_tri[:, None]
    dxy = d[:, :2] / np.maximum(np.linalg.norm(d[:, :2], axis=1, keepdims=True), 1e-30)
    perp = np.stack([-dxy[:, 1], dxy[:, 0]], 1)[:, None, :]
    up = rng.uniform(0, SEG, (F, S))  # how far up the capsule's segment the ray passes
    # xy distance
    s = rng.uniform(30.0, np.maximum(31.0, 1.2 * tt), (F, S))
    p = o + dd * s[..., None]
    side = np.where(rng.integers(0, 2, (F, S)) == 1, 1.0, -1.0)
    delta = np.array(DELTAS)[np.minimum(kind, 7)]
    xy = p[..., :2] + (side * R * (1.0 + delta))[..., None] * perp
    a = np.concatenate([xy, (p[..., 2] - R - up)[..., None]], -1)
    # behind the origin: ahead = along + max(0, h d.z) + 1.01 r == eps; beyond
    # the hit: along + min(0, h d.z) - 1.01 r == t_tri + eps
    eps = np.array(EPS)[kind & 3]
    dz = dd[..., 2]
    along = np.where(kind < 12, eps - np.maximum(0.0, SEG * dz) - CULL_R, tt + eps - np.minimum(0.0, SEG * dz) + CULL_R)
    co = o + dd * along[..., None]  # the capsule origin (base + r) on the ray's line
    b = co - np.array([0.0, 0.0, R])
    # origin inside the capsule / on its axis
    off = np.where((kind == 16)[..., None], rng.uniform(-0.6, 0.6, (F, S, 2)) * R, 0.0)
    c = np.concatenate([o[..., :2] + off, (o[..., 2] - R - up)[..., None]], -1)
    return np.where((kind < 8)[..., None], a, np.where((kind < 16)[..., None], b, c))


@functools.lru_cache(maxsize=None)
def families():
    """Sight / world-ray queries.  Per base ray a family of 19: the target
    capsule placed so that the ray enters its side where it hits the
    triangle, its base moved -8 .. +8 ulps along the dominant xy axis of d,
    and two members moved 2^15 ulps (about a unit) either way.
    N is 2 or 12; the other capsules sit on the culls' thresholds
    (_other_capsules), one on the ray origin's axis at index `self`.  Plus
    near-vertical and vertical rays over and under capsules.
    Returns a dict of arrays over the queries, those with N = 2 first:
    org, d [n][3]; caps [n][12][3] (the first N used); N, target, self_,
    family, nudge [n] (ulps; 0 for the vertical rays); kinds [n][12]
    (-1 target, -2 unused); ray_org, ray_d: each family's ray."""
    rng = np.random.default_rng(202)
    bo, bd, bt = _base_rays(rng, 4000, 1500)
    F = len(bo)
    o64, d64 = bo.astype(np.float64), bd.astype(np.float64)
    hit = o64 + d64 * bt.astype(np.float64)[:, None]
    dxy = d64[:, :2] / np.linalg.norm(d64[:, :2], axis=1, keepdims=True)
    tbase = np.stack([hit[:, 0] + dxy[:, 0] * R, hit[:, 1] + dxy[:, 1] * R, hit[:, 2] - R - 17.0], 1).astype(F32)
    ax = np.where(np.abs(bd[:, 0]) > np.abs(bd[:, 1]), 0, 1)
    fam_N = np.where(np.arange(F) % 2 == 0, 2, 12)
    target = np.where(fam_N == 2, np.arange(F) // 2 % 2, rng.integers(0, 12, F))
    # slot s of a family (its s-th non-target capsule) gets kind k0 + 5 s mod
    # 18: 5 is coprime to 18, so a family of 12 holds 11 distinct kinds
    kind = (rng.integers(0, N_KINDS, F)[:, None] + 5 * np.arange(11)[None, :]) % N_KINDS
    other = _other_capsules(kind, o64, d64, bt.astype(np.float64), rng).astype(F32)
    on_axis = kind == 17
    other[..., :2] = np.where(on_axis[..., None], bo[:, None, :2], other[..., :2])
    caps = np.full((F, 12, 3), 1e4, F32)  # unused slots (never read): far away
    kinds = np.full((F, 12), -2, np.int32)
    self_ = np.full(F, -1, np.int32)
    rows = np.arange(F)
    for s_ in range(11):
        j = s_ + (s_ >= target)  # the s-th index that is not the target
        use = j < fam_N
        caps[rows[use], j[use]] = other[use, s_]
        kinds[rows[use], j[use]] = kind[use, s_]
        me = use & on_axis[:, s_]
        self_[me] = j[me]
    kinds[rows, target] = -1
    nudges = np.array(list(NUDGES) + list(FAR_NUDGES), np.int32)
    K = len(nudges)
    rep = np.repeat(rows, K)
    nud = np.tile(nudges, F)
    c_all = caps[rep]
    tb = tbase[rep]
    axr = ax[rep]
    tb[np.arange(F * K), axr] = _nudge(tb[np.arange(F * K), axr], nud)
    c_all[np.arange(F * K), target[rep]] = tb
    # vertical and near-vertical rays: down onto / up under a capsule (target),
    # a second capsule beside it
    m = 600
    im = np.arange(m)
    vo = rng.uniform([-1200, -1200, 60], [1200, 1200, 250], (m, 3)).astype(F32)
    tilt = np.where(im % 3 == 0, 0.0, 10.0 ** rng.uniform(-7, -2, m))
    a = rng.uniform(0, 2 * np.pi, m)
    vd = _unit(np.stack([np.cos(a) * tilt, np.sin(a) * tilt, np.where(im % 2 == 0, -1.0, 1.0)], 1)).astype(F32)
    vd[im % 3 == 0, :2] = np.where(im[im % 3 == 0, None] % 4 < 2, F32(0.0), F32(-0.0))
    vc = np.full((m, 12, 3), 1e4, F32)
    dist = rng.uniform(20, 60, m)
    off = rng.uniform(-1, 1, (m, 2)) * rng.choice([0.0, 5.0, R * 0.999, R * 1.0101], m)[:, None]
    top = vo.astype(np.float64) + vd.astype(np.float64) * dist[:, None]
    vc[:, 0] = np.stack([top[:, 0] + off[:, 0], top[:, 1] + off[:, 1],
                         top[:, 2] - np.where(vd[:, 2] < 0, 2 * R + SEG, 0.0)], 1)
    vc[:, 1] = np.stack([vo[:, 0] + F32(R * 1.005), vo[:, 1], vc[:, 0, 2]], 1)
    vk = np.full((m, 12), -2, np.int32)
    vk[:, 0], vk[:, 1] = -1, 0
    out = dict(org=np.concatenate([bo[rep], vo]), d=np.concatenate([bd[rep], vd]), caps=np.concatenate([c_all, vc]),
               N=np.concatenate([fam_N[rep], np.full(m, 2)]).astype(np.int32),
               target=np.concatenate([target[rep], np.zeros(m)]).astype(np.int32),
               self_=np.concatenate([self_[rep], np.full(m, -1)]).astype(np.int32),
               family=np.concatenate([rep, F + im]).astype(np.int32),
               kinds=np.concatenate([kinds[rep], vk]), nudge=np.concatenate([nud, np.zeros(m)]).astype(np.int32))
    order = np.argsort(out["N"], kind="stable")
    out = {k: np.ascontiguousarray(v[order]) for k, v in out.items()}
    out["num_nudged_families"] = F
    out["ray_org"], out["ray_d"] = np.concatenate([bo, vo]), np.concatenate([bd, vd])
    return out


def by_N(fam):
    """[(N, slice)] of the queries with each capsule count (N = 2 first)."""
    n2 = int((fam["N"] == 2).sum())
    return [(2, slice(0, n2)), (12, slice(n2, len(fam["N"])))]


@functools.lru_cache(maxsize=None)
def family_answers():
    """The oracle on families(): t_tri, tri_hit (collision tree, slot order),
    t_c (the target capsule), and hit / t / entity of the world ray."""
    fam = families()
    t_tri, tri_hit = trace(fam["org"], fam["d"])
    n = len(fam["N"])
    t_c = capsule_t(fam["org"], fam["d"], fam["caps"][np.arange(n), fam["target"]])
    hit, t, ent = np.zeros(n, np.int32), np.zeros(n, F32), np.zeros(n, np.int32)
    for N, sl in by_N(fam):
        hit[sl], t[sl], ent[sl] = trace_world(fam["org"][sl], fam["d"][sl], fam["caps"][sl][:, :N])
    return dict(t_tri=t_tri, tri_hit=tri_hit, t_c=t_c, hit=hit, t=t, entity=ent,
                seen=((hit == 1) & (ent == fam["target"])).astype(np.int32))


def cull_terms(fam, t_tri, tri_hit):
    """The three cull expressions of capsulesD / visibleFullD in float64, per
    query and capsule slot [n][12]: (cr^2 - cull_r2 dxy2, ahead, beyond) --
    the capsule is culled when the first is > 0, the second < 0, or the third
    > 0 (with min_t = the triangle hit, FLT_MAX on a miss)."""
    o = fam["org"].astype(np.float64)[:, None, :]
    d = fam["d"].astype(np.float64)[:, None, :]
    co = fam["caps"].astype(np.float64).copy()
    co[:, :, 2] += R
    tr = o - co
    dxy2 = d[..., 0] ** 2 + d[..., 1] ** 2
    cr = tr[..., 0] * d[..., 1] - tr[..., 1] * d[..., 0]
    along = -(tr * d).sum(-1)
    ahead = along + np.maximum(0.0, SEG * d[..., 2]) + CULL_R
    min_t = np.where(tri_hit == 1, t_tri.astype(np.float64), float(KFLT_MAX))[:, None]
    beyond = along + np.minimum(0.0, SEG * d[..., 2]) - CULL_R - min_t
    return cr * cr - CULL_R * CULL_R * dxy2, ahead, beyond


# ----------------------------------------------------- float64 restatement
def tri_hits64(org, d, verts, edge_eps=(0.0,)):
    """Moller-Trumbore in float64 over every triangle, front faces only (the
    watertight test accepts n . d < 0, n = (b - a) x (c - a)): per value of
    edge_eps a table t [n][T], inf where missed.  edge_eps widens (> 0) or
    narrows (< 0) every triangle in barycentric units."""
    tris = verts.reshape(-1, 3, 3).astype(np.float64)
    a, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    nrm = np.cross(e1, e2)
    out = [np.full((len(org), len(tris)), np.inf) for _ in edge_eps]
    for s in range(0, len(org), 2048):
        o = org[s:s + 2048].astype(np.float64)[:, None, :]
        dd = d[s:s + 2048].astype(np.float64)[:, None, :]
        p = np.cross(dd, e2[None])
        det = (e1[None] * p).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - a[None]
            u = (tv * p).sum(-1) * inv
            q = np.cross(tv, e1[None])
            v = (dd * q).sum(-1) * inv
            t = (e2[None] * q).sum(-1) * inv
            front = ((nrm[None] * dd).sum(-1) < 0) & (t >= 0)
            for k, e in enumerate(edge_eps):
                ok = front & (u >= -e) & (v >= -e) & (u + v <= 1 + e)
                out[k][s:s + 2048] = np.where(ok, t, np.inf)
    return out


# The watertight test decides a triangle's edges on float32 coordinates
# sheared along the ray: each carries a few ulps of the largest coordinate
# difference (~2e3 units -> ~5e-4 units), against projected triangles tens to
# hundreds of units across, i.e. up to ~1e-4 in barycentric units.  Where a
# float64 test has to accept every triangle float32 can hit, triangles are
# widened by that much.
EDGE_SLACK = 1e-4


@functools.lru_cache(maxsize=None)
def family_tri64():
    """tri_hits64 of every family's ray [families][T] (collision-tree
    triangle order); the nearest t with every triangle widened and narrowed
    by 1e-6; the table with every triangle widened by EDGE_SLACK."""
    fam = families()
    _, verts, _ = T.scene_bvh()
    t64, wide, narrow, loose = tri_hits64(fam["ray_org"], fam["ray_d"], verts, (0.0, 1e-6, -1e-6, EDGE_SLACK))
    return t64, wide.min(1), narrow.min(1), loose


def capsule64(org, d, base):
    """The smallest t > 0 at which the ray enters the vertical capsule of
    radius R over base (segment base.z + R .. base.z + R + SEG), float64; 0
    when it misses or starts inside.  org, d [n][3]; base [n][3]."""
    o = org.astype(np.float64) - base.astype(np.float64)
    o[:, 2] -= R
    d = d.astype(np.float64)
    zc = np.clip(o[:, 2], 0, SEG)
    inside = o[:, 0] ** 2 + o[:, 1] ** 2 + (o[:, 2] - zc) ** 2 <= R * R
    best = np.full(len(o), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = d[:, 0] ** 2 + d[:, 1] ** 2
        b = o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]
        c = o[:, 0] ** 2 + o[:, 1] ** 2 - R * R
        disc = b * b - a * c
        t = (-b - np.sqrt(np.maximum(disc, 0))) / a
        z = o[:, 2] + t * d[:, 2]
        ok = (a > 0) & (disc >= 0) & (t > 0) & (z >= 0) & (z <= SEG)
        best = np.where(ok, t, best)
        dd = (d * d).sum(1)
        for h in (0.0, SEG):
            m = o.copy()
            m[:, 2] -= h
            b = (m * d).sum(1)
            c = (m * m).sum(1) - R * R
            disc = b * b - dd * c
            t = (-b - np.sqrt(np.maximum(disc, 0))) / dd
            ok = ~((c > 0) & (b > 0)) & (disc >= 0) & (t > 0) & (t < best)
            best = np.where(ok, t, best)
    return np.where(inside | ~np.isfinite(best), 0.0, best)


# ------------------------------------------------------------------ hints
def hint_sets(fam, ans, verts):
    """Per query the occluder hints to try, as triangle indices (u16) of the
    collision tree: none (0xffff), the triangle the oracle's closest hit lies
    on, a triangle hit beyond t_c, a triangle the ray misses, the triangle
    count and a value past it."""
    n = len(fam["N"])
    ntri = len(verts) // 9
    t64, _, _, loose = family_tri64()
    f = fam["family"]
    t_c = ans["t_c"].astype(np.float64)
    near_i = np.argmin(t64, axis=1)
    near_t = t64[np.arange(len(t64)), near_i]
    # the triangle the oracle's closest hit lies on: the float64 nearest when
    # its t agrees with the oracle's to 1e-5, else none
    on = np.isfinite(near_t[f]) & (ans["tri_hit"] == 1) & (np.abs(near_t[f] - ans["t_tri"]) <= 1e-5 * ans["t_tri"])
    closest = np.where(on, near_i[f], 0xffff)
    # a triangle hit beyond t_c: the farthest one on the ray
    fin = np.where(np.isfinite(t64), t64, -np.inf)
    far_i = np.argmax(fin, axis=1)
    far_t = fin[np.arange(len(t64)), far_i]
    beyond = np.where(far_t[f] > t_c * 1.01, far_i[f], 0xffff)
    missed = np.argmax(~np.isfinite(loose), axis=1)[f]  # missed even when widened by EDGE_SLACK
    sets = dict(none=np.full(n, 0xffff), closest=closest, beyond=beyond, missed=missed,
                num_tris=np.full(n, ntri), past_end=np.full(n, ntri + 7))
    return {name: h.astype(np.uint16) for name, h in sets.items()}


# ------------------------------------------------------------------ casts
@functools.lru_cache(maxsize=None)
def move_origins():
    """20,000 cast origins of test_quirk_grid.k_move_origins (one rollout,
    shared by the casts and the stuck waves; read-only)."""
    o, org = Q.k_move_origins(10000, np.random.default_rng(303), worlds=2, steps=60)
    o.close()
    org.setflags(write=False)
    return org


@functools.lru_cache(maxsize=None)
def casts():
    """10,000 horizontal casts (forward bound move + buffer + 4, z1 = z + 41,
    act1 alternating) and 10,000 vertical casts (bound 2 top + 10) from
    test_quirk_grid.k_move_origins."""
    rng = np.random.default_rng(304)
    org = move_origins()
    idx = rng.permutation(len(org))
    oh, ov = org[idx[:10000]], org[idx[10000:20000]]
    ang = rng.uniform(0, 2 * np.pi, 10000)
    dh = np.stack([np.sin(ang), np.cos(ang), np.zeros(10000)], 1).astype(F32)
    dh /= np.linalg.norm(dh, axis=1, keepdims=True).astype(F32)
    # axis-parallel ones, their zero component as -0 too
    dh[:40] = np.tile(np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], F32), (10, 1))
    dh[40:80] = np.where(dh[:40] == 0, F32(-0.0), dh[:40])
    move = rng.uniform(0, 20.0, 10000).astype(F32)
    bh = (move + Q.BUFFER) + Q.CAST_SLACK
    z1 = (oh[:, 2] + F32(41.0)).astype(F32)
    act1 = (np.arange(10000) % 2).astype(np.int32)
    dv = np.tile(np.array([0, 0, -1], F32), (10000, 1))
    top = np.array([50.0, 32.0, 30.0], F32)[rng.integers(0, 3, 10000)]  # stand, crouch, prone
    bv = (F32(2.0) * top + F32(10.0)).astype(F32)
    return dict(oh=oh, dh=dh, bh=bh, z1=z1, act1=act1, ov=ov, dv=dv, bv=bv)


def sphere_casts(org, d, t_max=None):
    return Q.casts(oracle(), org, d, t_max)


def cast_guards(c):
    """(path guard clear for the horizontal casts, cell guard clear for the
    vertical ones), as castPathQuirkFreeD / castQuirkFreeD decide."""
    q = Q.quirk_grid()
    px, py = c["oh"][:, 0] + c["oh"][:, 0], c["oh"][:, 1] + c["oh"][:, 1]
    path = Q.guard_path_clear(q, px, py, px + c["dh"][:, 0] * c["bh"], py + c["dh"][:, 1] * c["bh"])
    cell = Q.guard_clear(q, c["ov"][:, 0] + c["ov"][:, 0], c["ov"][:, 1] + c["ov"][:, 1])
    return path, cell


# ------------------------------------------------------------ stuck waves
def _eval(fn, x):
    x = np.ascontiguousarray(x, F32)
    out = np.zeros_like(x)
    oracle().lib.oracle_eval_math(fn, T.fptr(x), T.fptr(x), T.fptr(out), len(x))
    return out


def stuck_oracle(x, v, low_check):
    """The stuck fallback's four casts (sim.cpp:962-984) for every lane:
    hd[n][4], float32 step by step as the reference writes them."""
    n = len(x)
    hd = np.zeros((n, 4), F32)
    r = F32(R)
    for k in range(4):
        rad = np.full(n, F32(k) * F32(3.14159) * F32(0.5), F32)
        c, s = _eval(1, rad), _eval(0, rad)
        dv = np.stack([c * v[:, 0] - s * v[:, 1], s * v[:, 0] + c * v[:, 1], np.zeros(n, F32)], 1).astype(F32)
        ro = (x - dv * r * F32(2.0)).astype(F32)
        ro[:, 2] = ro[:, 2] + low_check
        hd[:, k], _ = sphere_casts(ro, dv)
    return hd


@functools.lru_cache(maxsize=None)
def stuck_waves():
    """Waves of 64 lanes for stuckCastsD: flags [n] (bit 0 active, bit 1
    need), x, v_norm [n][3], low_check [n], and per wave (na, need count).
    Active masks: all 64; lanes < 8 / 16 / 32; one lane; random masks with
    holes; lane 0 inactive.  need counts per mask: 0, 1, 2, 3, na / 4 + 1 and
    every active lane, so 4 k casts are dealt in 1, 2 and 4 rounds."""
    rng = np.random.default_rng(404)
    org = move_origins()
    lanes = np.arange(64)
    masks = [lanes < 64, lanes < 8, lanes < 16, lanes < 32, lanes == 37, lanes == 0,
             rng.random(64) < 0.5, rng.random(64) < 0.2, (rng.random(64) < 0.7) & (lanes > 0)]
    masks[6][0] = True
    flags, meta = [], []
    for m in masks:
        act = np.flatnonzero(m)
        na = len(act)
        for want in (0, 1, 2, 3, na // 4 + 1, na):
            k = min(want, na)
            f = m.astype(np.int32)
            f[rng.choice(act, k, replace=False)] |= 2
            if k and want != na and rng.integers(0, 2):  # also the last active lane
                f[act[-1]] |= 2
            # lanes that are gone may carry `need` garbage: it must not count
            f[~m] |= rng.integers(0, 2, 64)[~m] * 2
            flags.append(f)
            meta.append((na, int(((f & 3) == 3).sum())))
    flags = np.concatenate(flags).astype(np.int32)
    n = len(flags)
    x = org[rng.integers(0, len(org), n)].astype(F32)
    ang = rng.uniform(0, 2 * np.pi, n)
    v = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1).astype(F32)
    v /= np.linalg.norm(v, axis=1, keepdims=True).astype(F32)
    low = rng.choice(np.array([30.0, 30.0 - 15.0 + 0.75], F32), n).astype(F32)  # standing / prone
    return dict(flags=flags, x=x, v=v, low_check=low, meta=meta)
