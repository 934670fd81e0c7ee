"""The device's geometry shortcuts, query by query (mpenv_debug_geom_queries,
include/mpenv.h) against the plain oracle, bit for bit (T.compare): the lidar
ray on its octant images, the world ray with its capsule culls, line of sight
with its bounded search, early exit and occluder hints, the
bounded and paired sphere casts, and the stuck fallback's casts dealt over a
wave.  Inputs: tests/geom_cases.py (tests/test_geom_cases.py checks on the CPU
that they reach the cases they are built for).  The hook compiles the step
kernels' device functions a second time; the step kernels' own code
generation stays with the whole-step parity tests."""
import ctypes as C
import functools

import numpy as np
import pytest

import geom_cases as G
import mpenv_testlib as T
import scene_residency_testlib as R

pytestmark = pytest.mark.gpu

LIDAR_RAY, WORLD_RAY, SIGHT, CASTS, STUCK = range(5)
SIZES = (1, 255, 257)  # around the hook's 256-thread block; the full set comes on top


class Hook:
    """Uploads a query set once; run() launches the hook on its first n
    queries and returns the outputs as numpy arrays."""

    def __init__(self, engine, **inputs):
        import torch
        self.torch = torch
        self.e = engine
        self.lib = T.lib_mpenv()
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inputs.items()}

    def run(self, mode, n, outs, num_caps=0, sub=0, hint=None, t_init=None):
        torch = self.torch
        q = T.GeomQueries()
        for k, v in self.dev.items():
            setattr(q, k, v.data_ptr())
        bufs = {}
        for name, (shape, dt) in outs.items():
            bufs[name] = torch.zeros(shape, dtype={np.float32: torch.float32, np.int32: torch.int32}[dt], device="cuda")
            setattr(q, name, bufs[name].data_ptr())
        if t_init is not None:
            bufs["t"].copy_(torch.from_numpy(t_init.view(np.float32)))
        if hint is not None:
            hd = torch.from_numpy(np.ascontiguousarray(hint).view(np.int16)).cuda()
            q.hint = hd.data_ptr()
        q.num_caps, q.sub = num_caps, sub
        rc = self.lib.mpenv_debug_geom_queries(self.e.h, mode, n, C.byref(q), None)
        assert rc == 0, self.lib.mpenv_last_error().decode()
        res = {k: v.cpu().numpy() for k, v in bufs.items()}
        if hint is not None:
            res["hint"] = hd.cpu().numpy().view(np.uint16)
        return res


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401  (before the engine initialises HIP: importing it afterwards takes ten times as long)
    e = T.Engine(1, 1)
    yield e
    e.close()


def sizes(n):
    return [k for k in SIZES if k < n] + [n]


def test_lidar_ray_on_octant_images_matches_oracle(engine):
    """bvhTraceRayT<false, kOctNodeQ, true, true> on the image rayOctant(d)
    picks, as k_lidar: t and hit equal the oracle's octant order on the lidar
    tree on every ray, the +0 / -0 directions included (-0 counts as negative
    on both sides, DESIGN.md section 2 definition 12)."""
    org, d, (z0, z1) = G.rays()
    t_ref, h_ref = G.trace(org, d, 1)
    hook = Hook(engine, o=org, d=d)
    for n in sizes(len(org)):
        r = hook.run(LIDAR_RAY, n, dict(t=((len(org),), np.float32), i0=((len(org),), np.int32)))
        T.compare(r["i0"][:n], h_ref[:n], f"lidar ray hit n={n}")
        T.compare(r["t"][:n], t_ref[:n], f"lidar ray t n={n}")
        assert not r["i0"][n:].any() and not r["t"][n:].any()  # nothing past n is written
    assert h_ref[z0:z1].sum() > 1000


def test_world_ray_with_capsule_culls_matches_oracle(engine):
    """traceWorldD (collision tree, three conservative capsule culls, the
    `self` skip) against traceRayAgainstWorld's body with no cull: hit, t and
    entity; `self` = the capsule whose axis the origin is on gives the same
    as -1."""
    fam, ans = G.families(), G.family_answers()
    for N, sl in G.by_N(fam):
        org, d, caps = fam["org"][sl], fam["d"][sl], np.ascontiguousarray(fam["caps"][sl][:, :N])
        n_all = len(org)
        none = np.full(n_all, -1, np.int32)
        outs = dict(t=((n_all,), np.float32), i0=((n_all,), np.int32), i1=((n_all,), np.int32))
        res = {}
        for name, sel in (("self", fam["self_"][sl]), ("none", none)):
            hook = Hook(engine, o=org, d=d, caps=caps, sel=sel)
            for n in sizes(n_all) if name == "self" else [n_all]:
                r = hook.run(WORLD_RAY, n, outs, num_caps=N)
                T.compare(r["i0"][:n], ans["hit"][sl][:n], f"world ray hit N={N} {name} n={n}")
                T.compare(r["t"][:n], ans["t"][sl][:n], f"world ray t N={N} {name} n={n}")
                T.compare(r["i1"][:n], ans["entity"][sl][:n], f"world ray entity N={N} {name} n={n}")
            res[name] = r
        for k in ("i0", "t", "i1"):
            T.compare(res["self"][k], res["none"][k], f"world ray self vs -1 {k}")
        assert (fam["self_"][sl] >= 0).sum() > 100


def test_sight_matches_oracle_for_every_hint(engine):
    """visibleQuickD + visibleFullD (k_vis: search bounded at 1.001 t_c,
    early exit at any hit <= t_c, occluder hint) and visibleRayD without a
    hint (k_sim's flank sight) on the collision tree, against the oracle's
    closest-hit world ray: seen / not seen equal for every hint value; a hint
    written back names a triangle the float64 restatement hits no farther
    than t_c (1 + 1e-5); a second pass fed the written hints answers the
    same."""
    fam, ans = G.families(), G.family_answers()
    _, verts, _ = T.scene_bvh()
    hs = G.hint_sets(fam, ans, verts)
    ntri = len(verts) // 9
    loose = G.family_tri64()[3]
    for N, sl in G.by_N(fam):
        org, d, caps = fam["org"][sl], fam["d"][sl], np.ascontiguousarray(fam["caps"][sl][:, :N])
        n_all = len(org)
        seen_ref = ans["seen"][sl]
        t_c = ans["t_c"][sl].astype(np.float64)
        f = fam["family"][sl]
        hook = Hook(engine, o=org, d=d, caps=caps, sel=fam["target"][sl])
        outs = dict(i0=((n_all,), np.int32))
        for n in sizes(n_all):
            r = hook.run(SIGHT, n, outs, num_caps=N, sub=1)
            T.compare(r["i0"][:n], seen_ref[:n], f"visibleRayD N={N} n={n}")
        prev = None
        for name in ("none", "closest", "beyond", "missed", "num_tris", "past_end", "previous"):
            h_in = prev if name == "previous" else hs[name][sl]
            for n in sizes(n_all) if name == "none" else [n_all]:
                r = hook.run(SIGHT, n, outs, num_caps=N, sub=0, hint=h_in)
                T.compare(r["i0"][:n], seen_ref[:n], f"sight N={N} hint={name} n={n}")
                assert np.array_equal(r["hint"][n:], h_in[n:])
            written = np.flatnonzero(r["hint"] != h_in)
            assert (r["hint"][written] < ntri).all()
            assert (r["i0"][written] == 0).all()  # only an occluder is ever recorded
            t_hint = loose[f[written], r["hint"][written].astype(np.int64)]
            bad = ~(t_hint <= t_c[written] * (1 + 1e-5))
            assert not bad.any(), (name, N, written[bad][:5], t_hint[bad][:5], t_c[written][bad][:5])
            # a second pass over what this one wrote
            r2 = hook.run(SIGHT, n_all, outs, num_caps=N, sub=0, hint=r["hint"])
            T.compare(r2["i0"], seen_ref, f"sight N={N} hint={name} second pass")
            if name == "none":
                assert len(written) > 1000
            prev = r2["hint"]


def _cast_outs(n, two=False):
    return dict(t=((n, 2) if two else (n,), np.float32), normal=((n, 2, 3) if two else (n, 3), np.float32))


def _check_near(t, nrm, t_ref, n_ref, B, name):
    """castNearD's contract: the oracle's hit and normal where its full cast
    is nearer than B, else a result at or beyond B."""
    near = t_ref < B
    T.compare(t[near], t_ref[near], name + " t")
    T.compare(nrm[near], n_ref[near], name + " normal")
    assert (t[~near] >= B[~near]).all(), name
    return int(near.sum())


def test_sphere_casts_full_bounded_and_paired_match_oracle(engine):
    """bvhSphereCastD, castNearD, castNear2D (two casts, one traversal) and
    castFirstNearD against the oracle's unbounded MeshBVH::sphereCast."""
    c = G.casts()
    n_all = 10000
    t_ref, n_ref = G.sphere_casts(c["oh"], c["dh"])
    o1 = c["oh"].copy()
    o1[:, 2] = c["z1"]
    t_ref1, n_ref1 = G.sphere_casts(o1, c["dh"])
    hook = Hook(engine, o=c["oh"], d=c["dh"], bound=c["bh"], z1=c["z1"], sel=c["act1"])
    for n in sizes(n_all):
        r = hook.run(CASTS, n, _cast_outs(n_all), sub=0)
        T.compare(r["t"][:n], t_ref[:n], f"full cast t n={n}")
        hit = t_ref[:n] < G.KFLT_MAX
        T.compare(r["normal"][:n][hit], n_ref[:n][hit], f"full cast normal n={n}")
        r1 = hook.run(CASTS, n, _cast_outs(n_all), sub=1)
        _check_near(r1["t"][:n], r1["normal"][:n], t_ref[:n], n_ref[:n], c["bh"][:n], f"castNearD n={n}")
        r2 = hook.run(CASTS, n, _cast_outs(n_all, True), sub=2)
        T.compare(r2["t"][:n, 0], r1["t"][:n], f"castNear2D low t n={n}")
        T.compare(r2["normal"][:n, 0], r1["normal"][:n], f"castNear2D low normal n={n}")
        assert not r2["t"][n:].any()
    compared = _check_near(r1["t"], r1["normal"], t_ref, n_ref, c["bh"], "castNearD")
    # the high cast alone, through castNearD from (o.xy, z1)
    hook1 = Hook(engine, o=o1, d=c["dh"], bound=c["bh"])
    rh = hook1.run(CASTS, n_all, _cast_outs(n_all), sub=1)
    compared += _check_near(rh["t"], rh["normal"], t_ref1, n_ref1, c["bh"], "castNearD from z1")
    on = c["act1"] == 1
    T.compare(r2["t"][on, 1], rh["t"][on], "castNear2D high t")
    T.compare(r2["normal"][on, 1], rh["normal"][on], "castNear2D high normal")
    assert (r2["t"][~on, 1] == G.KFLT_MAX).all() and not r2["normal"][~on, 1].any()  # cast 1 not run
    # vertical casts
    tv_ref, _ = G.sphere_casts(c["ov"], c["dv"])
    hv = Hook(engine, o=c["ov"], d=c["dv"], bound=c["bv"])
    for n in sizes(n_all):
        r = hv.run(CASTS, n, dict(t=((n_all,), np.float32)), sub=3)
        T.compare(r["t"][:n], tv_ref[:n], f"castFirstNearD n={n}")
    r = hv.run(CASTS, n_all, _cast_outs(n_all), sub=0)
    T.compare(r["t"], tv_ref, "full vertical cast t")
    assert compared > 1000


@functools.lru_cache(maxsize=None)
def _stuck_ref():
    """G.stuck_waves() and the oracle's hd4 for every lane of it, computed once."""
    w = G.stuck_waves()
    return w, G.stuck_oracle(w["x"], w["v"], w["low_check"])


def _check_stuck(engine, lanes):
    """Launches the STUCK hook on the first k lanes for every k of lanes(n),
    the last being the whole set n: hd4 of the lanes with `need` equals the
    oracle's bit for bit, every other lane keeps its NaN-pattern prefill."""
    w, ref = _stuck_ref()
    n = len(w["flags"])
    fill = (np.uint32(0x7fc0a000) + np.arange(n * 4, dtype=np.uint32)).reshape(n, 4)
    hook = Hook(engine, o=w["x"], d=w["v"], bound=w["low_check"], sel=w["flags"])
    for k in lanes(n):
        r = hook.run(STUCK, k, dict(t=((n, 4), np.float32)), t_init=fill)
        got = r["t"]
        need = np.zeros(n, bool)
        need[:k] = (w["flags"][:k] & 3) == 3
        T.compare(got[need], ref[need], f"stuck hd4 lanes={k}")
        T.compare(got[~need].view(np.uint32), fill[~need], f"stuck untouched lanes={k}")
    assert need.sum() > 300


def test_stuck_casts_dealt_over_partial_waves_match_serial_oracle(engine):
    """stuckCastsD as applyVelocityD calls it, on waves with lanes that have
    left, with 0 .. every active lane stuck (1, 2 and 4 dealing rounds): hd4
    of every active lane with `need` equals the four serial casts of
    sim.cpp:962-984; every other lane's hd4 keeps its NaN-pattern prefill."""
    _check_stuck(engine, lambda n: sorted({64, 256 + 64, n}))  # one wave, a block and a wave, every wave


def test_stuck_casts_on_the_global_images_match_serial_oracle():
    """The same check through k_geom_queries_g<STUCK>: simple_map switched to
    the global-resident images (no other test runs this mode of the hook
    there), on the first wave and on every wave."""
    import torch  # noqa: F401  (before the engine initialises HIP, as in engine())
    e = T.Engine(1, 1)
    try:
        assert R.set_residency(e, R.GLOBAL) == 0, e.lib.mpenv_last_error().decode()
        assert R.residency(e) == R.GLOBAL
        _check_stuck(e, lambda n: [64, n])
    finally:
        e.close()
