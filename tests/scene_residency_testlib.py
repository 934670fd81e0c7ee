"""Test infrastructure for scene residency (include/mpenv_scene_residency.h,
DESIGN.md §3 "Scene residency"): the ctypes binding of the header's
functions, cached big scenes (tests/big_scene.py), and an oracle handed one
tree as its collision tree.

Nothing here is imported by the product.
"""
import ctypes as C
import functools
import os
import tempfile

import numpy as np

import big_scene
import mpenv_testlib as T

AUTO, LDS, GLOBAL = 0, 1, 2  # MPENV_SCENE_*
ERR_INVALID, ERR_UNSUPPORTED = -1, -4

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


class SceneInfo(C.Structure):
    _fields_ = [("triangles", i32), ("collision_nodes", i32), ("collision_stack", i32), ("lidar_nodes", i32),
                ("lidar_stack", i32), ("lidar_triangles", i32), ("residency", i32), ("supported", i32),
                ("lds_bytes_move", i64), ("lds_bytes_sim", i64), ("lds_bytes_vis", i64), ("lds_bytes_lidar", i64),
                ("global_bytes", i64), ("reason", C.c_char * 128)]


SIGNATURES = {
    "mpenv_set_scene_residency": (i32, [vp, i32]),
    "mpenv_scene_residency": (i32, [vp, C.POINTER(i32)]),
    "mpenv_scene_info": (i32, [C.c_char_p, C.POINTER(SceneInfo)]),
}


def lib():
    l = T.lib_mpenv()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    return l


def scene_info(path):
    """(return code, SceneInfo)"""
    info = SceneInfo()
    rc = lib().mpenv_scene_info(path.encode(), C.byref(info))
    return rc, info


def set_residency(e, mode):
    """The status code: callers assert."""
    return lib().mpenv_set_scene_residency(e.h, mode)


def residency(e):
    m = i32(-1)
    assert lib().mpenv_scene_residency(e.h, C.byref(m)) == 0
    return m.value


_tmp = None


@functools.lru_cache(maxsize=None)
def pillars(n, seed=3):
    """pillar_scene(n, seed) under a directory that lives as long as the
    process; written once per (n, seed)."""
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="mpenv_big_scene_")
    return big_scene.pillar_scene(os.path.join(_tmp.name, f"pillars_{n}_{seed}"), n, seed)


@functools.lru_cache(maxsize=None)
def slivers(n):
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="mpenv_big_scene_")
    return big_scene.sliver_scene(os.path.join(_tmp.name, f"slivers_{n}"), n)


class TreeOracle:
    """An oracle (1 world, 1v1) whose collision tree is the scene's collision
    tree or (lidar=True) its lidar tree, for the per-tree geometry hooks
    (oracle_trace_ray and oracle_sphere_cast walk the collision tree)."""

    def __init__(self, scene, lidar=False):
        self.lib = T.lib_oracle()
        self.nodes, self.verts, self.max_stack = T.scene_bvh(scene, lidar=lidar)
        ln, lv, _ = T.scene_bvh(scene, lidar=True)
        self._keep = (ln, lv, scene.encode())
        cfg = T.OracleConfig(1, 5, 1, 0, 1, 0, self._keep[2], self.nodes.ctypes.data, len(self.nodes) // 64,
                             self.verts.ctypes.data, len(self.verts) // 3, T.TASK_ZONE, 0, 1, ln.ctypes.data,
                             len(ln) // 64, lv.ctypes.data, len(lv) // 3)
        self.h = self.lib.oracle_create(C.byref(cfg))
        assert self.h, "oracle_create failed"

    def close(self):
        if self.h:
            self.lib.oracle_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def seeded_rays(n, seed, bounds):
    rng = np.random.default_rng(seed)
    o = rng.uniform(bounds[:3], bounds[3:], (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)
