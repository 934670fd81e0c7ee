"""Scene residency without a GPU (include/mpenv_scene_residency.h, DESIGN.md
§3): what mpenv_scene_info says about simple_map and the generated pillar
scenes, that the generated scenes really leave the LDS path's limits, that the
oracle alone handles the big scene (BVH traversal against brute force on both
trees), the binding against the header, the Python names, and a refusal."""
import ctypes as C
import os
import re

import numpy as np

import big_scene
import mpenv_testlib as T
import scene_residency_testlib as R

HEADER = os.path.join(T.ROOT, "include", "mpenv_scene_residency.h")
LDS_BUDGET = 64 * 1024


def lds_bytes(info):
    return dict(k_move=info.lds_bytes_move, k_sim=info.lds_bytes_sim, k_vis=info.lds_bytes_vis,
                k_lidar=info.lds_bytes_lidar)


def test_scene_info_simple_map_is_lds_resident():
    rc, i = R.scene_info(T.SCENE)
    assert rc == 0
    assert i.supported == 1 and i.residency == R.LDS and i.reason == b""
    assert i.triangles == 252 and i.collision_nodes == 61 and i.lidar_nodes == 54
    assert i.lds_bytes_lidar == 63936 and i.lds_bytes_move == 31872
    assert max(lds_bytes(i).values()) <= LDS_BUDGET
    assert i.collision_stack <= 16 and i.lidar_stack <= 16
    assert i.global_bytes == i.lds_bytes_move + i.lds_bytes_lidar


def test_scene_info_pillars_40_is_global_because_of_lds_bytes():
    """Under every count limit of the LDS path, over its LDS budget: on the
    parent commit this scene was created and then could not launch."""
    rc, i = R.scene_info(R.pillars(40))
    assert rc == 0
    assert i.collision_nodes <= 256 and i.lidar_nodes <= 256
    assert i.collision_stack <= 16 and i.lidar_stack <= 16
    assert i.triangles > 252 + 12 * 30  # few pillars fall near a spawn
    assert i.lds_bytes_lidar > LDS_BUDGET and i.lds_bytes_move > LDS_BUDGET
    assert i.supported == 1 and i.residency == R.GLOBAL
    assert b"LDS" in i.reason  # why not LDS-resident


def test_scene_info_pillars_100_is_global_because_of_nodes_and_stack():
    rc, i = R.scene_info(R.pillars(100))
    assert rc == 0
    assert i.collision_nodes > 256 and i.lidar_stack > 16
    assert i.collision_stack <= 64 and i.lidar_stack <= 64
    assert i.supported == 1 and i.residency == R.GLOBAL
    assert b"nodes" in i.reason


def test_pillar_scene_follows_its_recipe(tmp_path):
    """12 outward-facing triangles per pillar inside the stated ranges, none
    within 40 units of a spawn region, the other files byte-equal, and the
    same seed gives the same bytes."""
    d = big_scene.pillar_scene(str(tmp_path / "a"), 100, 3)
    base = big_scene.read_collisions(os.path.join(big_scene.SIMPLE_MAP, "collisions.bin"))
    c = big_scene.read_collisions(os.path.join(d, "collisions.bin"))
    nb = len(base["minfo"])
    assert np.array_equal(c["verts"][:len(base["verts"])], base["verts"]) and np.array_equal(c["bounds"], base["bounds"])
    spawns = big_scene.read_spawn_regions(os.path.join(d, "spawns.bin"))
    b = c["bounds"]
    assert 80 <= len(c["minfo"]) - nb <= 100
    for voff, nv, toff, nt in c["minfo"][nb:]:
        assert (nv, nt) == (8, 12)
        v = c["verts"][voff:voff + 8]
        lo, hi = v.min(0), v.max(0)
        hw = (hi[:2] - lo[:2]) / 2
        assert abs(hw[0] - hw[1]) < 1e-3 and 4 - 1e-3 <= hw[0] <= 12 + 1e-3
        assert 20 - 1e-3 <= hi[2] - lo[2] <= 120 + 1e-3 and b[2] - 1e-3 <= lo[2] <= b[2] + 60
        ctr = (lo + hi) / 2
        assert (ctr[:2] >= b[:2] + 40 - 1e-3).all() and (ctr[:2] <= b[3:5] - 40 + 1e-3).all()
        gap_x = np.maximum(spawns[:, 0] - hi[0], lo[0] - spawns[:, 3])
        gap_y = np.maximum(spawns[:, 1] - hi[1], lo[1] - spawns[:, 4])
        assert (np.maximum(gap_x, gap_y) >= 40 - 1e-3).all()
        assert (c["tmat"][toff:toff + 12] == base["tmat"][0]).all()
        tri = v[c["idx"][toff:toff + 12]].astype(np.float64)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert (np.einsum("ij,ij->i", n, tri.mean(1) - ctr) > 0).all()  # outward
    for f in big_scene.COPIED:
        assert open(os.path.join(d, f), "rb").read() == open(os.path.join(big_scene.SIMPLE_MAP, f), "rb").read()
    d2 = big_scene.pillar_scene(str(tmp_path / "b"), 100, 3)
    assert open(os.path.join(d, "collisions.bin"), "rb").read() == open(os.path.join(d2, "collisions.bin"), "rb").read()


def _vertex_quirk_exposed(org, d, verts, r):
    """Casts on which the tree and brute force may differ by the reference's
    own definition: its vertex test (mesh_bvh.inl:1073-1104, the quirk
    tests/test_quirk_grid.py is about) intersects the ray from 2 * origin with
    a sphere around the vertex, so a triangle can report a hit far from its
    bounds.  The tree never visits that triangle; brute force does.  A cast
    is exposed when, in float64, the ray from 2 * origin passes within r
    (0.1% slack) of any vertex; every other cast must match bit for bit."""
    v = verts.reshape(-1, 3).astype(np.float64)
    p, dd = 2.0 * org.astype(np.float64), d.astype(np.float64)
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    out = np.zeros(len(org), bool)
    rr = (r * 1.001) ** 2
    for k in range(len(org)):
        w = v - p[k]
        s = w @ dd[k]
        w2 = np.einsum("ij,ij->i", w, w)
        out[k] = ((w2 <= rr) | ((s >= 0) & (w2 - s * s <= rr))).any()
    return out


def _bvh_vs_brute(lidar):
    """oracle_trace_ray against oracle_trace_ray_brute on 2,000 seeded rays
    plus edge_aimed_rays, and oracle_sphere_cast against
    oracle_sphere_cast_brute on 2,000 seeded casts, on one tree of
    pillar_scene(n=100).  Casts: see _vertex_quirk_exposed -- with this
    scene's 2,880 vertices a few of the 2,000 are exposed (cast 1564 on the
    collision tree: tree 834.640, brute force 453.706, a vertex-test hit on a
    triangle whose box the cast never enters); on those brute force may only
    be nearer.  Rays: the closest hit depends on the visiting order by an
    ulp where two hits are that close (seeded ray 1268 on the lidar tree:
    488.58737 in slot order, 488.58740 in triangle order), so t may differ by
    at most 2 ulp on at most 0.5% of the hits, and the order-free smallest-t
    rule (oracle_trace_ray_batch orders 2 and 3) must agree on every ray."""
    scene = R.pillars(100)
    o = R.TreeOracle(scene, lidar=lidar)
    assert len(o.nodes) // 64 > 256  # beyond the LDS path either way
    bounds = big_scene.read_collisions(os.path.join(scene, "collisions.bin"))["bounds"]
    ro, rd = R.seeded_rays(2000, 11, bounds)
    eo, ed = T.edge_aimed_rays(o.verts, 1, 12)
    lib = o.lib
    hits = ties = 0
    for org, d in ((ro, rd), (eo, ed)):
        for k in range(len(org)):
            t1, t2 = C.c_float(0), C.c_float(0)
            h1 = lib.oracle_trace_ray(o.h, T.fptr(org[k]), T.fptr(d[k]), C.byref(t1))
            h2 = lib.oracle_trace_ray_brute(o.h, T.fptr(org[k]), T.fptr(d[k]), C.byref(t2))
            assert h1 == h2, (lidar, k)
            if h1:
                hits += 1
                if t1.value != t2.value:
                    # visiting order: a hit is kept when T <= t_max * det in float32 (mesh_bvh.inl:433-554), so
                    # of two hits one ulp apart the one met second can be refused; never more than that apart
                    ties += 1
                    assert abs(t1.value - t2.value) <= 2.0 * np.spacing(np.float32(max(t1.value, t2.value))), \
                        (lidar, k, t1.value, t2.value)
        # the order-free rule, smallest t: the tree misses no triangle brute force finds (bit for bit)
        n = len(org)
        oo, dd = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(d, np.float32)
        tb, hb, tt, ht = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        lib.oracle_trace_ray_batch(o.h, n, T.fptr(oo), T.fptr(dd), 2, T.fptr(tt), ht.ctypes.data)
        lib.oracle_trace_ray_batch(o.h, n, T.fptr(oo), T.fptr(dd), 3, T.fptr(tb), hb.ctypes.data)
        T.compare(ht, hb, f"smallest-t hit, lidar={lidar}")
        T.compare(tt[hb == 1], tb[hb == 1], f"smallest-t t, lidar={lidar}")
    assert hits > 2000 and ties <= hits // 200, (hits, ties)
    nrm = np.zeros(3, np.float32)
    co, cd = R.seeded_rays(2000, 13, bounds)
    exposed = _vertex_quirk_exposed(co, cd, o.verts, 15.0)
    near = 0
    for k in range(len(co)):
        t1 = lib.oracle_sphere_cast(o.h, T.fptr(co[k]), T.fptr(cd[k]), 15.0, T.fptr(nrm))
        t2 = lib.oracle_sphere_cast_brute(o.h, T.fptr(co[k]), T.fptr(cd[k]), 15.0)
        if exposed[k]:
            assert t2 <= t1, (lidar, k, t1, t2)  # brute force visits every triangle the tree does
            continue
        assert np.float32(t1).view(np.uint32) == np.float32(t2).view(np.uint32), (lidar, k, t1, t2)
        near += t1 < 3.0e38
    assert (~exposed).sum() > 1500 and near > 300, ((~exposed).sum(), near)
    o.close()


def test_oracle_bvh_equals_brute_force_on_the_big_collision_tree():
    _bvh_vs_brute(False)


def test_oracle_bvh_equals_brute_force_on_the_big_lidar_tree():
    _bvh_vs_brute(True)


def test_binding_table_matches_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = dict((name, params) for name, params in re.findall(r"^int (mpenv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M))
    assert sorted(decl) == sorted(R.SIGNATURES)
    for name, params in decl.items():
        restype, argtypes = R.SIGNATURES[name]
        assert restype is C.c_int32 and len(argtypes) == len(params.split(",")), name
        for p, at in zip(params.split(","), argtypes):
            if "*" in p:
                assert at in (C.c_void_p, C.c_char_p) or issubclass(at, C._Pointer), (name, p)
            else:
                assert "int32_t" in p and at is C.c_int32, (name, p)
    assert re.search(r"#define MPENV_SCENE_AUTO 0\b", text) and re.search(r"#define MPENV_SCENE_LDS 1\b", text)
    assert re.search(r"#define MPENV_SCENE_GLOBAL 2\b", text)
    # the struct, field by field
    body = re.search(r"typedef struct mpenv_scene_info_t \{(.*?)\} mpenv_scene_info_t;", text, flags=re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(int32_t|int64_t|char)\s+([^;]+);", body):
        for nm in names.split(","):
            fields.append((nm.strip().split("[")[0], ctype))
    want = [(n, {C.c_int32: "int32_t", C.c_int64: "int64_t"}.get(t, "char")) for n, t in R.SceneInfo._fields_]
    assert fields == want
    assert '#include "mpenv_scene_residency.h"' in open(os.path.join(T.ROOT, "include", "mpenv.h")).read()
    l = R.lib()
    assert l.mpenv_set_scene_residency(None, R.GLOBAL) == R.ERR_INVALID
    assert l.mpenv_scene_residency(None, None) == R.ERR_INVALID
    assert l.mpenv_scene_info(None, None) == R.ERR_INVALID
    info = R.SceneInfo()
    assert l.mpenv_scene_info(b"/nonexistent/scene", C.byref(info)) == -2  # MPENV_ERR_IO


def test_python_names_and_scene_info_dict():
    import madrona_mp_env as m

    for name in ("set_scene_residency", "scene_residency"):
        assert hasattr(m.SimManager, name), name
    d = m.scene_info(T.SCENE)
    assert d["residency"] == "lds" and d["supported"] is True and d["reason"] == ""
    assert d["lds_bytes"] == dict(k_move=31872, k_sim=d["lds_bytes"]["k_sim"], k_vis=d["lds_bytes"]["k_vis"], k_lidar=63936)
    assert (d["triangles"], d["collision_nodes"], d["lidar_nodes"]) == (252, 61, 54)
    g = m.scene_info(R.pillars(100))
    assert g["residency"] == "global" and g["supported"] is True
    hpp = open(os.path.join(T.ROOT, "include", "mpenv_manager.hpp")).read()
    assert "setSceneResidency" in hpp and "sceneResidency" in hpp


def test_scene_info_refuses_a_scene_with_too_many_triangles_or_too_deep_a_tree():
    """Degenerate slivers along a line: a few thousand give a tree deeper
    than the traversal stack, 66,000 pass the triangle limit of k_vis's
    16-bit occluder hints.  Refused by name, and never LDS- or
    global-resident."""
    import madrona_mp_env as m

    rc, deep = R.scene_info(R.slivers(3000))
    assert rc == 0
    assert max(deep.collision_stack, deep.lidar_stack) > 64 and deep.triangles <= 0xfffe
    assert deep.supported == 0 and deep.residency == R.AUTO
    assert b"stack bound" in deep.reason and b"64" in deep.reason
    rc, many = R.scene_info(R.slivers(66000))
    assert rc == 0
    assert many.triangles == 252 + 66000
    assert many.supported == 0 and many.residency == R.AUTO
    assert b"triangles" in many.reason and b"65534" in many.reason
    d = m.scene_info(R.slivers(3000))
    assert d["supported"] is False and d["residency"] is None and "stack bound" in d["reason"]
