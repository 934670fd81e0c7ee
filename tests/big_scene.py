"""Scenes larger than simple_map, generated on the fly (never committed).

pillar_scene(dst, n, seed) writes under `dst` a copy of scenes/simple_map whose
collisions.bin holds up to `n` more meshes: axis-aligned boxes ("pillars") of
12 outward-facing triangles with the scene's first material.  navmesh.bin,
spawns.bin and zones.bin are copied unchanged (lidar_tree.txt is not: the
lidar tree of the bigger scene is the builder's own).  File formats: SURVEY.md
Appendix B; the reader mirrors tests/test_scene_bvh.py::parse_collisions.

sliver_scene(dst, n) adds `n` degenerate triangles in one mesh instead: a
scene for the engine to refuse (triangle limit).
"""
import os
import shutil
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIMPLE_MAP = os.path.join(os.path.dirname(HERE), "scenes", "simple_map")
COPIED = ("navmesh.bin", "spawns.bin", "zones.bin")

# corner k of a box: bit 0 = x, bit 1 = y, bit 2 = z; each face counter-clockwise seen from outside
_BOX_TRIS = np.array([[0, 2, 3], [0, 3, 1],   # z = lo (normal -z)
                      [4, 5, 7], [4, 7, 6],   # z = hi
                      [0, 1, 5], [0, 5, 4],   # y = lo
                      [2, 6, 7], [2, 7, 3],   # y = hi
                      [0, 4, 6], [0, 6, 2],   # x = lo
                      [1, 3, 7], [1, 7, 5]],  # x = hi
                     np.uint32)


def read_collisions(path):
    buf = open(path, "rb").read()
    off = 0

    def take(fmt, n=1):
        nonlocal off
        out = np.frombuffer(buf, dtype=np.dtype("<" + fmt), count=n, offset=off)
        off += out.nbytes
        return out

    c = {}
    c["bounds"] = take("f", 6)
    nmat = int(take("Q")[0])
    nname = int(take("Q")[0])
    c["names"] = take("B", nname)
    c["mflags"] = take("I", nmat)
    nmesh, nvert, ntri = (int(x) for x in take("Q", 3))
    c["verts"] = take("f", 3 * nvert).reshape(-1, 3)
    c["idx"] = take("I", 3 * ntri).reshape(-1, 3)
    c["tmat"] = take("I", ntri)
    c["minfo"] = take("I", 4 * nmesh).reshape(-1, 4)
    assert off == len(buf)
    return c


def write_collisions(path, c):
    verts = np.ascontiguousarray(c["verts"], "<f4")
    idx = np.ascontiguousarray(c["idx"], "<u4")
    tmat = np.ascontiguousarray(c["tmat"], "<u4")
    minfo = np.ascontiguousarray(c["minfo"], "<u4")
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(c["bounds"], "<f4").tobytes())
        f.write(struct.pack("<QQ", len(c["mflags"]), len(c["names"])))
        f.write(np.ascontiguousarray(c["names"], "u1").tobytes())
        f.write(np.ascontiguousarray(c["mflags"], "<u4").tobytes())
        f.write(struct.pack("<QQQ", len(minfo), len(verts), len(idx)))
        f.write(verts.tobytes())
        f.write(idx.tobytes())
        f.write(tmat.tobytes())
        f.write(minfo.tobytes())


def read_spawn_regions(path):
    """[n][6] AABBs of every A, B and common spawn."""
    buf = open(path, "rb").read()
    off, out = 0, []
    for _ in range(3):
        n = struct.unpack_from("<I", buf, off)[0]
        off += 4
        rec = np.frombuffer(buf, "<f4", count=8 * n, offset=off).reshape(n, 8)
        off += 32 * n
        out.append(rec[:, :6])
    assert off == len(buf)
    return np.concatenate(out)


def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    verts = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)], np.float32)
    return verts, _BOX_TRIS.copy()


def _copy_rest(dst):
    os.makedirs(dst, exist_ok=True)
    for name in COPIED:
        shutil.copy(os.path.join(SIMPLE_MAP, name), os.path.join(dst, name))


def _append_meshes(c, meshes):
    verts, idx, tmat, minfo = [c["verts"]], [c["idx"]], [c["tmat"]], [c["minfo"]]
    vo, to = len(c["verts"]), len(c["idx"])
    mat = c["tmat"][0]  # the scene's first material
    for v, t in meshes:
        verts.append(v)
        idx.append(t)
        tmat.append(np.full(len(t), mat, np.uint32))
        minfo.append(np.array([[vo, len(v), to, len(t)]], np.uint32))
        vo += len(v)
        to += len(t)
    out = dict(c)
    out["verts"], out["idx"] = np.concatenate(verts), np.concatenate(idx)
    out["tmat"], out["minfo"] = np.concatenate(tmat), np.concatenate(minfo)
    return out


def pillar_scene(dst, n, seed=3):
    """Returns dst.  `n` pillars are drawn; one whose footprint comes within
    40 units of a spawn region is skipped, so the scene may hold fewer."""
    c = read_collisions(os.path.join(SIMPLE_MAP, "collisions.bin"))
    spawns = read_spawn_regions(os.path.join(SIMPLE_MAP, "spawns.bin"))
    b = c["bounds"]
    rng = np.random.default_rng(seed)
    meshes = []
    for _ in range(n):
        cx = rng.uniform(b[0] + 40, b[3] - 40)
        cy = rng.uniform(b[1] + 40, b[4] - 40)
        hw = rng.uniform(4, 12)
        h = rng.uniform(20, 120)
        z0 = rng.uniform(b[2], b[2] + 60)
        near = ((cx + hw + 40 > spawns[:, 0]) & (cx - hw - 40 < spawns[:, 3]) &
                (cy + hw + 40 > spawns[:, 1]) & (cy - hw - 40 < spawns[:, 4]))
        if near.any():
            continue
        meshes.append(box_mesh((cx - hw, cy - hw, z0), (cx + hw, cy + hw, z0 + h)))
    _copy_rest(dst)
    write_collisions(os.path.join(dst, "collisions.bin"), _append_meshes(c, meshes))
    return dst


def sliver_scene(dst, n):
    """simple_map plus one mesh of `n` zero-area triangles (a, a, b) along a
    line under the floor: nothing to hit, only triangles to count."""
    c = read_collisions(os.path.join(SIMPLE_MAP, "collisions.bin"))
    b = c["bounds"]
    x = np.linspace(b[0] + 50, b[3] - 50, n + 1, dtype=np.float32)
    verts = np.stack([x, np.full_like(x, b[1] + 50), np.full_like(x, b[2] + 1)], 1)
    k = np.arange(n, dtype=np.uint32)
    tris = np.stack([k, k, k + 1], 1)
    _copy_rest(dst)
    write_collisions(os.path.join(dst, "collisions.bin"), _append_meshes(c, [(verts, tris)]))
    return dst
