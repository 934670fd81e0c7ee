"""Shared by tests/test_lidar_backface.py (CPU) and
tests/test_lidar_backface_gpu.py: seeded ray sets aimed at the cases where
dropping an octant's back-facing triangles from k_lidar's node images (scene.h
octantNodeImages, DESIGN.md section 2 definition 16) could change an answer,
the rule restated in numpy, and the host program tests/lidar_backface_host.cpp
that runs the product's scene.cpp."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import mpenv_testlib as T

F32 = np.float32
OFFSETS = (0.0, 1e-6, 1e-4, 1e-2, 1.0)

NODE = np.dtype([("min", "<f4", 3), ("exp", "i1", 3), ("internal", "u1"), ("triSize", "u1", 4),
                 ("qMinX", "u1", 4), ("qMinY", "u1", 4), ("qMinZ", "u1", 4),
                 ("qMaxX", "u1", 4), ("qMaxY", "u1", 4), ("qMaxZ", "u1", 4),
                 ("children", "<i4", 4), ("parent", "<i4")])
assert NODE.itemsize == 64
QBYTES = ("qMinX", "qMinY", "qMinZ", "qMaxX", "qMaxY", "qMaxZ")


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def octant(d):
    """rayOctant: sign bits, -0 counts as negative."""
    s = np.signbit(np.asarray(d, F32))
    return s[:, 0].astype(int) | (s[:, 1].astype(int) << 1) | (s[:, 2].astype(int) << 2)


def rule(verts):
    """dead[8][T]: the pruning rule on float32 vertices [T*9], in float64."""
    tri = np.asarray(verts, F32).reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    ln = np.linalg.norm(n, axis=1)
    dead = np.zeros((8, len(tri)), bool)
    for o in range(8):
        s = np.array([-1.0 if o >> i & 1 else 1.0 for i in range(3)])
        ok = (ln > 0) & (s * n >= 0).all(1) & ~((n != 0) & (np.abs(n) < 1e-6 * ln[:, None])).any(1)
        dead[o] = ok
    return dead


# ------------------------------------------------------------------- rays
def random_rays(n, seed):
    rng = np.random.default_rng(seed)
    org = rng.uniform([-1500, -1500, -50], [1500, 1500, 300], (n, 3))
    return org.astype(F32), _unit(rng.normal(size=(n, 3))).astype(F32)


def near_axis_rays(verts, n, seed):
    """Near-axis rays from on or near vertices (tests/test_lidar_order.py)."""
    rng = np.random.default_rng(seed)
    V = np.asarray(verts).reshape(-1, 3)
    org = V[rng.integers(0, len(V), n)] + rng.normal(size=(n, 3)) * rng.choice([0, 1e-3, 1, 30], size=(n, 1))
    d = np.zeros((n, 3))
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1, 1], n)
    d += rng.normal(size=(n, 3)) * rng.choice([0, 0, 1e-6, 1e-2], size=(n, 1))
    return org.astype(F32), _unit(d).astype(F32)


def skimming_rays(verts, per, seed, at_vertices):
    """Origins 0 / 1e-6 / 1e-4 / 1e-2 / 1 off a triangle's plane, on either
    side, with directions parallel to the plane aimed into that triangle
    (at_vertices: at one of its vertices).  Half of the rays carry their
    zero direction components as -0."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(verts, F32).reshape(-1, 3, 3).astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    keep = np.linalg.norm(nrm, axis=1) > 0
    tri, nrm = tri[keep], _unit(nrm[keep])
    u = _unit(tri[:, 1] - tri[:, 0])
    v = np.cross(nrm, u)
    T_ = len(tri)
    k = np.repeat(np.arange(T_), per * len(OFFSETS) * 2)
    off = np.tile(np.repeat(np.array(OFFSETS), 2) * np.tile([1.0, -1.0], len(OFFSETS)), T_ * per)
    m = len(k)
    th, r = rng.uniform(0, 2 * np.pi, m), rng.uniform(1, 800, m)
    p = tri[k].mean(1) + (r * np.cos(th))[:, None] * u[k] + (r * np.sin(th))[:, None] * v[k]
    if at_vertices:
        target = tri[k, rng.integers(0, 3, m)]
    else:
        w = rng.dirichlet([1, 1, 1], m)
        target = (w[:, :, None] * tri[k]).sum(1)
    d = _unit(target - p)
    d[np.abs(d) < 1e-12] = 0.0  # exactly parallel to an axis-aligned plane
    d = d.astype(F32)
    flip = rng.random(m) < 0.5
    d[flip] = np.where(d[flip] == 0, F32(-0.0), d[flip])
    return (p + off[:, None] * nrm[k]).astype(F32), d


# ------------------------------------------------------------ host program
@functools.lru_cache(maxsize=None)
def host_program():
    """tests/lidar_backface_host.cpp built against csrc/scene.cpp with the
    oracle's float flags."""
    d = tempfile.mkdtemp(prefix="lidar_backface_")
    exe = os.path.join(d, "host")
    csrc = os.path.join(T.PKG, "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                    "-I", csrc, "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "lidar_backface_host.cpp"), os.path.join(csrc, "scene.cpp"),
                    os.path.join(csrc, "navmesh.cpp"), "-o", exe, "-lpthread"], check=True)
    return exe


def run_host(mode, nodes, verts, org, d):
    """mode 0: (full images [8][n], pruned images [8][n], (t, hit) on the
    full images, (t, hit) on the pruned ones); mode 1: (dead [8][T],
    (t, hit) over every triangle, (t, hit) over the octant's live ones)."""
    nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    verts = np.ascontiguousarray(verts, F32).reshape(-1)
    org, d = np.ascontiguousarray(org, F32), np.ascontiguousarray(d, F32)
    n, nv, nr = len(nodes) // 64, len(verts) // 3, len(org)
    exe = host_program()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([mode, n, nv, nr], np.int32).tobytes())
            for a in (nodes, verts, org, d):
                f.write(a.tobytes())
        subprocess.run([exe, fin, fout], check=True)
        raw = np.fromfile(fout, np.uint8)
    head = 2 * 8 * n * 64 if mode == 0 else 8 * (nv // 3)
    assert len(raw) == head + 16 * nr
    res = raw[head:].reshape(4, nr * 4)
    ans = [(res[0].view(F32), res[1].view(np.int32)), (res[2].view(F32), res[3].view(np.int32))]
    if mode == 0:
        img = raw[:head].view(NODE).reshape(2, 8, n)
        return img[0], img[1], ans[0], ans[1]
    return raw[:head].reshape(8, nv // 3).astype(bool), ans[0], ans[1]
