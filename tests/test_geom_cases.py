"""The inputs of tests/test_geom_queries_gpu.py reach the cases they are built
for (tests/geom_cases.py), checked through the oracle alone -- conditions on
the inputs, not measurements of the device: exact capsule / triangle ties,
both sight answers, both sides of every capsule cull, both branches of the
casts' path guard; and the oracle's world-ray hook is checked against its
parts and against a float64 restatement of line of sight."""
import ctypes as C

import numpy as np

import geom_cases as G
import mpenv_testlib as T


def test_rays_hold_both_signed_zeros_and_tiny_components():
    org, d, (z0, z1) = G.rays()
    assert len(org) == len(d) and org.dtype == np.float32 and d.dtype == np.float32
    zd = d[z0:z1]
    neg0 = (zd == 0) & np.signbit(zd)
    pos0 = (zd == 0) & ~np.signbit(zd)
    for k in range(3):
        assert neg0[:, k].sum() >= 1000 and pos0[:, k].sum() >= 1000, (k, neg0[:, k].sum(), pos0[:, k].sum())
    # every pattern of a direction exists with the zero's other sign
    keys = {(r.tobytes()) for r in zd}
    flipped = np.where(zd == 0, -zd, zd)
    assert all(r.tobytes() in keys for r in flipped)
    tiny = d[z1:]
    mag = np.abs(tiny).min(1)
    assert ((mag >= 0.9e-8) & (mag <= 1.1e-4)).all()
    t, h = G.trace(org, d, 1)
    assert h[z0:z1].sum() > 1000 and h[z1:].sum() > 1000  # these rays do reach geometry
    print(f"\nrays {len(org)}: edge-aimed and fans {z0}, signed-zero {z1 - z0} ({h[z0:z1].sum()} hit), "
          f"tiny-component {len(org) - z1} ({h[z1:].sum()} hit)")


def test_sight_families_reach_ties_both_answers_and_every_cull():
    fam, ans = G.families(), G.family_answers()
    nudged = fam["family"] < fam["num_nudged_families"]
    t_c, t_tri = ans["t_c"], ans["t_tri"]
    m = nudged & (np.abs(fam["nudge"]) <= 8) & (t_c != 0) & (ans["tri_hit"] == 1)  # the +-8-ulp members only
    lt, eq, gt = (t_c[m] < t_tri[m]).sum(), (t_c[m] == t_tri[m]).sum(), (t_c[m] > t_tri[m]).sum()
    tie_families = len(np.unique(fam["family"][m & (t_c == t_tri)]))
    seen, unseen = int(ans["seen"].sum()), int((ans["seen"] == 0).sum())
    print(f"\nfamilies {fam['num_nudged_families']} ({m.sum()} queries): t_c < t_tri {lt}, == {eq}, > {gt}; "
          f"families reaching a tie {tie_families}; seen {seen}, not seen {unseen}")
    assert tie_families >= 200
    assert min(lt, eq, gt) >= 1000
    assert min(seen, unseen) >= 1000
    # at a tie the triangle wins (utils.cpp:57-69 `t < min_hit_t`): the
    # target is not the entity unless another path made it so
    tie = m & (t_c == t_tri)
    assert (ans["seen"][tie] == 0).all()
    assert set(np.unique(fam["N"])) == {2, 12}

    # both sides of each cull, from geom_dev.h's expressions in float64
    c1, ahead, beyond = G.cull_terms(fam, t_tri, ans["tri_hit"])
    kinds = fam["kinds"]
    groups = {"xy distance": (kinds >= 0) & (kinds < 8), "behind": (kinds >= 8) & (kinds < 12),
              "beyond": (kinds >= 12) & (kinds < 16)}
    culled = {"xy distance": c1 > 0, "behind": ahead < 0, "beyond": beyond > 0}
    for name, g in groups.items():
        a, b = int((culled[name] & g).sum()), int((~culled[name] & g).sum())
        print(f"cull {name}: culled {a}, kept {b}")
        assert a >= 1000 and b >= 1000, (name, a, b)
    # the xy cull's two margins straddle 1.01 r, and delta = 0 +- 1e-6 straddle
    # the capsule's own radius (hit or miss of the exact test)
    for k, want in ((5, False), (6, True), (7, True), (0, False), (3, False)):
        sel = kinds == k
        assert (c1[sel] > 0).mean() > 0.99 if want else (c1[sel] > 0).mean() < 0.01, k
    # origin inside a capsule, and on a capsule's axis with and without `self`
    assert (kinds == 16).sum() >= 1000 and (fam["self_"] >= 0).sum() >= 1000
    sj = fam["self_"]
    on = sj >= 0
    own = fam["caps"][np.flatnonzero(on), sj[on]]
    assert (own[:, :2] == fam["org"][on, :2]).all()
    up = fam["org"][on, 2] - own[:, 2] - G.F32(G.R)
    assert (up >= -1e-3).all() and (up <= G.SEG + 1e-3).all()
    # vertical and near-vertical rays
    vert = ~nudged
    dxy0 = (fam["d"][:, 0] == 0) & (fam["d"][:, 1] == 0)
    assert (vert & dxy0).sum() >= 100 and (vert & ~dxy0).sum() >= 100
    assert ans["seen"][vert].sum() >= 50 and (ans["seen"][vert] == 0).sum() >= 50


def test_families_hold_rays_whose_closest_hit_depends_on_the_tree():
    """The family rays include rays along zero-margin child box faces (rays
    aimed at vertices): the slot-order closest hit on the collision tree and
    the closest hit on the lidar tree are then different triangles, far
    apart -- the inputs on which line of sight depends on the tree walked
    (DESIGN.md section 2 definition 4)."""
    fam, ans = G.families(), G.family_answers()
    t_l, h_l = G.trace(fam["org"], fam["d"], 1)
    both = (h_l == 1) & (ans["tri_hit"] == 1)
    far = (h_l != ans["tri_hit"]) | (both & (np.abs(t_l - ans["t_tri"]) > 1e-3 * ans["t_tri"]))
    ulp = both & (t_l != ans["t_tri"]) & ~far
    occluded_l = (h_l == 1) & (t_l <= ans["t_c"])
    occluded_c = (ans["tri_hit"] == 1) & (ans["t_tri"] <= ans["t_c"])
    flips = (ans["t_c"] != 0) & (occluded_l != occluded_c)
    print(f"\nclosest hit, lidar tree vs collision tree: far apart on {far.sum()} queries of "
          f"{len(np.unique(fam['family'][far]))} families, an ulp or so apart on {ulp.sum()}; "
          f"'a triangle at or before t_c' differs on {flips.sum()} queries")
    assert far.sum() >= 10 and flips.sum() >= 10


def test_world_batch_equals_trace_ray_plus_capsule_loop():
    fam, ans = G.families(), G.family_answers()
    o = G.oracle()
    rng = np.random.default_rng(9)
    tie = np.flatnonzero((ans["t_c"] == ans["t_tri"]) & (ans["t_c"] != 0))
    idx = np.concatenate([rng.choice(len(fam["N"]), 3000, replace=False), tie[:500]])
    r, seg = G.F32(G.R), G.F32(G.SEG)
    for i in idx:
        org, d = fam["org"][i].copy(), fam["d"][i].copy()
        tt = C.c_float(0)
        hit = o.lib.oracle_trace_ray(o.h, T.fptr(org), T.fptr(d), C.byref(tt)) != 0
        min_t = np.float32(tt.value) if hit else G.KFLT_MAX
        ent = -1
        for j in range(int(fam["N"][i])):
            co = fam["caps"][i, j].copy()
            co[2] += r
            tr = (org - co).astype(np.float32)
            t = np.float32(o.lib.oracle_capsule(T.fptr(tr), T.fptr(d), r, seg))
            if t != 0 and t < min_t:
                min_t, hit, ent = t, True, j
        assert (int(hit), ent) == (ans["hit"][i], ans["entity"][i]), i
        assert np.float32(min_t).view(np.uint32) == ans["t"][i].view(np.uint32), i


def test_horizontal_sight_agrees_with_float64_restatement():
    """Families with d.z == 0: seen / not seen against Moller-Trumbore over
    every triangle plus an analytic vertical capsule, in float64.  Compared
    where the float64 answer is decisive: the target's t_c differs from the
    nearest triangle hit and from every other capsule's entry by more than
    1e-4 t, the nearest triangle hit is the same with every triangle widened
    or narrowed by 1e-6 (barycentric), and the answer is the same whether a
    grazed capsule counts as hit or as missed: a ray along a silhouette edge
    or a capsule's side has no margin in t to speak of."""
    fam, ans = G.families(), G.family_answers()
    sel = np.flatnonzero((fam["d"][:, 2] == 0) & (fam["family"] < fam["num_nudged_families"]))
    org, d = fam["org"][sel], fam["d"][sel]
    t64, wide, narrow, _ = G.family_tri64()
    f = fam["family"][sel]
    t_tri = t64.min(1)[f]
    stable = np.ones(len(sel), bool)
    for x in (wide[f], narrow[f]):
        stable &= (np.isfinite(x) == np.isfinite(t_tri)) & (
            ~np.isfinite(t_tri) | (np.abs(np.where(np.isfinite(x), x, 0) - np.where(np.isfinite(t_tri), t_tri, 0))
                                   <= 1e-6 * np.where(np.isfinite(t_tri), t_tri, 1)))
    n = len(sel)
    tcap = np.zeros((n, 12))
    for j in range(12):
        tcap[:, j] = G.capsule64(org, d, fam["caps"][sel, j])
    tcap[np.arange(12)[None, :] >= fam["N"][sel, None]] = 0
    tcap = np.where(tcap == 0, np.inf, tcap)
    t_c = tcap[np.arange(n), fam["target"][sel]]
    others = tcap.copy()
    others[np.arange(n), fam["target"][sel]] = np.inf
    # a capsule the ray's line grazes has no margin in t either: whether the
    # side is hit turns on r^2 - dist^2 (the quadratic's discriminant over
    # a), which float32 forms as b^2 - a c with an error of a few ulps of
    # b^2.  Such a capsule is taken both as missed and as hit as early as
    # that error allows.
    co = fam["caps"][sel].astype(np.float64)
    tr = org.astype(np.float64)[:, None, :2] - co[:, :, :2]
    dxy = d.astype(np.float64)[:, None, :2]
    b = (tr * dxy).sum(-1)
    dist2 = (tr * tr).sum(-1) - b * b
    tol = 1e-6 * (b * b + G.R * G.R)
    grazing = np.abs(G.R * G.R - dist2) < tol
    # the earliest a grazed capsule can be entered: its entry is -b - sqrt(r^2 - dist^2)
    entry = -b - np.sqrt(np.maximum(G.R * G.R - dist2, 0) + tol)
    decisive = stable & ~grazing[np.arange(n), fam["target"][sel]]
    seen64 = None
    for as_hit in (False, True):
        oth = np.where(grazing, np.where(as_hit & (entry > 0), entry, np.inf), others)
        rival = np.minimum(oth.min(1), t_tri)
        s64 = np.isfinite(t_c) & (t_c < rival)
        scale = np.where(np.isfinite(t_c), t_c, np.where(np.isfinite(rival), rival, 1.0))
        with np.errstate(invalid="ignore"):
            margin = np.where(np.isfinite(t_c) & np.isfinite(rival), np.abs(t_c - rival), np.inf)
        decisive &= margin > 1e-4 * scale
        if seen64 is not None:
            decisive &= s64 == seen64
        seen64 = s64
    agree = seen64 == (ans["seen"][sel] == 1)
    print(f"\nhorizontal queries {n}: decisive {decisive.sum()}, seen {seen64[decisive].sum()}, "
          f"disagreeing {(decisive & ~agree).sum()}")
    assert decisive.sum() >= 5000 and seen64[decisive].sum() >= 500
    assert agree[decisive].all(), sel[np.flatnonzero(decisive & ~agree)[:5]]


def test_hints_name_what_they_claim():
    fam, ans = G.families(), G.family_answers()
    _, verts, _ = T.scene_bvh()
    hs = G.hint_sets(fam, ans, verts)
    ntri = len(verts) // 9
    assert set(hs) == {"none", "closest", "beyond", "missed", "num_tris", "past_end"}
    assert (hs["closest"] < ntri).sum() >= 10000 and (hs["beyond"] < ntri).sum() >= 10000
    assert (hs["missed"] < ntri).all() and (hs["none"] == 0xffff).all()
    assert (hs["num_tris"] == ntri).all() and (hs["past_end"] == ntri + 7).all()
    # occluders and non-occluders both occur among the closest-hit hints
    t_hint = G.family_tri64()[0][fam["family"], np.minimum(hs["closest"], ntri - 1)]
    named = hs["closest"] < ntri
    assert (named & (t_hint <= ans["t_c"])).sum() >= 1000 and (named & (t_hint > ans["t_c"])).sum() >= 1000


def test_casts_reach_both_guard_branches_and_bounded_hits():
    c = G.casts()
    assert len(c["oh"]) == 10000 and len(c["ov"]) == 10000
    path, cell = G.cast_guards(c)
    t_h, _ = G.sphere_casts(c["oh"], c["dh"])
    t_v, _ = G.sphere_casts(c["ov"], c["dv"])
    hh, hv = int((t_h < c["bh"]).sum()), int((t_v < c["bv"]).sum())
    o1 = c["oh"].copy()
    o1[:, 2] = c["z1"]
    t_h1, _ = G.sphere_casts(o1, c["dh"])
    hh1 = int(((t_h1 < c["bh"]) & (c["act1"] == 1)).sum())
    print(f"\nhorizontal casts: path guard clear {path.mean():.3f}, full t < B on {hh} low and {hh1} high casts "
          f"({(path & (t_h < c['bh'])).sum()} of the low ones bounded); vertical casts: cell guard clear "
          f"{cell.mean():.3f}, full t < B on {hv} ({(cell & (t_v < c['bv'])).sum()} bounded)")
    for g in (path, cell):
        assert 0.1 <= g.mean() <= 0.9, g.mean()
    assert (path & (t_h < c["bh"])).sum() + (cell & (t_v < c["bv"])).sum() >= 1000
    assert (path & (t_h < c["bh"])).sum() >= 300 and (cell & (t_v < c["bv"])).sum() >= 300
    assert (c["act1"] == 1).sum() == 5000


def test_stuck_waves_cover_the_dealing_rounds():
    w = G.stuck_waves()
    n = len(w["flags"])
    assert n % 64 == 0 and 36 <= n // 64 <= 60
    f = w["flags"].reshape(-1, 64)
    act, need = (f & 1) != 0, (f & 3) == 3
    na, k = act.sum(1), need.sum(1)
    rounds = np.where(k > 0, -(-4 * k // np.maximum(na, 1)), 0)
    print(f"\nstuck waves {len(f)}: active lanes {sorted(set(na.tolist()))}, dealing rounds "
          f"{dict(zip(*np.unique(rounds, return_counts=True)))}")
    assert {0, 1, 2, 4} <= set(rounds.tolist())
    assert ((na == 1) & (k == 1)).any() and ((na == 64) & (k == 64)).any()
    assert (~act[:, 0]).any() and (na < 64).sum() > 20
    assert (k >= 2).sum() >= 20                      # two owners in one wave
    assert (need & ~np.roll(act, 1, axis=1)).any()   # a stuck lane next to a lane that has left
    hd = G.stuck_oracle(w["x"], w["v"], w["low_check"])
    assert hd.shape == (n, 4) and np.isfinite(hd[(w["flags"] & 3) == 3]).all()
