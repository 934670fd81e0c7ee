"""k_lidar's octant node images without their back-facing triangles
(scene.h octantNodeImages with prune, DESIGN.md section 2 definition 16), on
the CPU: the structure of the pruned images of simple_map's lidar tree, the
equality of every answer with the unpruned images and with the oracle's octant
order, and the rule itself on a synthetic soup of triangles.  The product's
scene.cpp runs inside tests/lidar_backface_host.cpp."""
import numpy as np
import pytest

import lidar_backface_cases as B
import mpenv_testlib as T
from test_lidar_order import _rollout_rays


@pytest.fixture(scope="module")
def tree():
    nodes, verts, _ = T.scene_bvh(lidar=True)
    return nodes, verts


@pytest.fixture(scope="module")
def images(tree):
    nodes, verts = tree
    full, pruned, _, _ = B.run_host(0, nodes, verts, np.zeros((0, 3), B.F32), np.zeros((0, 3), B.F32))
    return full, pruned


def _slots(node):
    """A node's occupied slots in order: (child, first tri, count, box bytes)."""
    out = []
    for i in range(4):
        c = int(node["children"][i])
        if c == -1:
            continue
        box = bytes(int(node[q][i]) for q in B.QBYTES)
        out.append((c, c & 0x7fffffff if c < 0 else -1, int(node["triSize"][i]), box))
    return out


def _live_tris(img):
    t = []
    for node in img:
        for c, leaf, cnt, _ in _slots(node):
            if c < 0:
                t += list(range(leaf, leaf + cnt))
    return t


def test_each_octant_keeps_exactly_the_triangles_the_rule_spares(tree, images):
    _, verts = tree
    full, pruned = images
    dead = B.rule(verts)
    ntri = len(verts) // 9
    assert ntri == 252
    for o in range(8):
        all_t, live = _live_tris(full[o]), _live_tris(pruned[o])
        assert sorted(all_t) == list(range(ntri))
        assert len(live) == len(set(live)) == 126
        removed = sorted(set(all_t) - set(live))
        assert removed == list(np.flatnonzero(dead[o]))


def test_survivors_keep_their_bytes_and_order_and_empties_trail(tree, images):
    nodes, _ = tree
    full, pruned = images
    src = nodes.view(B.NODE)
    for o in range(8):
        for ni in range(len(src)):
            f, p = full[o][ni], pruned[o][ni]
            assert f.tobytes()[:16] == p.tobytes()[:16] == src[ni].tobytes()[:16]  # min, exp, internalNodes
            assert f["parent"] == p["parent"]
            kids = [int(c) for c in p["children"]]
            k = sum(c != -1 for c in kids)
            assert all(c != -1 for c in kids[:k]) and all(c == -1 for c in kids[k:])
            assert all(int(p["triSize"][i]) == 0 for i in range(k, 4))
            fs, ps = _slots(f), _slots(p)
            at = 0
            for c, leaf, cnt, box in ps:
                # the next full slot this survivor came from
                while at < len(fs):
                    fc, fleaf, fcnt, fbox = fs[at]
                    at += 1
                    if c >= 0 and fc == c:
                        assert cnt == fcnt == 0
                        break
                    if c < 0 and fc < 0 and fleaf <= leaf < fleaf + fcnt:
                        assert cnt >= 1 and leaf + cnt <= fleaf + fcnt
                        # whole leaf, its first triangle alone, or its second alone
                        assert (leaf, cnt) in ((fleaf, fcnt), (fleaf, 1), (fleaf + 1, 1))
                        break
                else:
                    raise AssertionError(f"octant {o} node {ni}: survivor {c:#x} out of order")
                assert box == fbox
            # leaves before internal children, as in the full image
            kinds = [c < 0 for c, *_ in ps]
            assert kinds == sorted(kinds, reverse=True)


def test_every_reachable_node_has_a_live_triangle_below(images):
    _, pruned = images
    for o in range(8):
        img = pruned[o]

        def below(ni):
            n = 0
            for c, _, cnt, _ in _slots(img[ni]):
                if c < 0:
                    assert cnt >= 1
                    n += cnt
                else:
                    sub = below(c)
                    assert sub > 0, f"octant {o}: node {ni} keeps the dead subtree {c}"
                    n += sub
            return n

        assert below(0) == 126


@pytest.fixture(scope="module")
def oracle():
    o = T.Oracle(1, 1)
    yield o
    o.close()


def _oracle_trace(o, org, d):
    n = len(org)
    t, h = np.zeros(n, np.float32), np.zeros(n, np.int32)
    o.lib.oracle_trace_ray_batch(o.h, n, T.fptr(org), T.fptr(d), 1, T.fptr(t), h.ctypes.data)
    return t, h


def _ray_sets(verts):
    yield "random", B.random_rays(100000, 21)
    yield "edge aimed", T.edge_aimed_rays(verts, 6, seed=11)
    yield "near axis", B.near_axis_rays(verts, 20000, 22)
    yield "skimming into", B.skimming_rays(verts, 10, 23, False)
    yield "skimming at vertices", B.skimming_rays(verts, 10, 24, True)
    for combat in (False, True):
        org, d = _rollout_rays(combat)
        yield "combat fans" if combat else "tape fans", (org.astype(B.F32), d.astype(B.F32))


def test_pruned_and_full_images_answer_like_the_oracle_bit_for_bit(tree, oracle):
    nodes, verts = tree
    for name, (org, d) in _ray_sets(verts):
        org, d = np.ascontiguousarray(org, B.F32), np.ascontiguousarray(d, B.F32)
        t_ref, h_ref = _oracle_trace(oracle, org, d)
        _, _, (t0, h0), (t1, h1) = B.run_host(0, nodes, verts, org, d)
        T.compare(h0, h_ref, f"{name}: full images hit")
        T.compare(t0, t_ref, f"{name}: full images t")
        T.compare(h1, h_ref, f"{name}: pruned images hit")
        T.compare(t1, t_ref, f"{name}: pruned images t")
        assert h_ref.sum() * 4 > len(org), (name, int(h_ref.sum()), len(org))
        assert len(set(B.octant(d))) >= 4, name


def _soup(seed, n=500):
    """Randomly oriented triangles; a tenth with normals tilted 1e-7 off an
    axis, a tenth axis-aligned, some degenerate (a repeated vertex, three
    collinear vertices)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-300, 300, (n, 1, 3))
    tri = c + rng.normal(size=(n, 3, 3)) * rng.uniform(5, 120, (n, 1, 1))
    k = n // 10
    for j in range(2 * k):
        ax = j % 3
        e = np.eye(3)
        nrm = e[ax] * rng.choice([-1, 1])
        if j < k:
            nrm = nrm + 1e-7 * rng.choice([-1, 1]) * e[(ax + 1 + j % 2) % 3]
        u = np.cross(nrm, e[(ax + 1) % 3])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        tri[j] = c[j] + rng.normal(size=(3, 2)) @ np.stack([u, v]) * 80
    tri[2 * k:2 * k + 5, 2] = tri[2 * k:2 * k + 5, 1]
    tri[2 * k + 5:2 * k + 10, 2] = 2 * tri[2 * k + 5:2 * k + 10, 1] - tri[2 * k + 5:2 * k + 10, 0]
    return tri.astype(B.F32).reshape(-1)


def test_rule_on_a_triangle_soup_never_changes_a_brute_force_answer():
    verts = _soup(31)
    rng = np.random.default_rng(32)
    n = 20000
    org = rng.uniform(-400, 400, (n, 3))
    d = rng.normal(size=(n, 3))
    # a fifth of the rays near an axis, a fifth with exact zero components of either sign
    d[:n // 5] = np.eye(3)[rng.integers(0, 3, n // 5)] * rng.choice([-1, 1], (n // 5, 1)) \
        + rng.normal(size=(n // 5, 3)) * rng.choice([1e-8, 1e-6, 1e-3], (n // 5, 1))
    d[n // 5:2 * n // 5][rng.random((n // 5, 3)) < 0.4] = 0.0
    d[(d == 0).all(1)] = [1.0, 0.0, 0.0]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(B.F32)
    flip = rng.random(n) < 0.5
    d[flip] = np.where(d[flip] == 0, B.F32(-0.0), d[flip])
    nodes = np.zeros(64, np.uint8)
    dead, (t0, h0), (t1, h1) = B.run_host(1, nodes, verts, org.astype(B.F32), d)
    assert np.array_equal(dead, B.rule(verts))
    per_oct = dead.sum(1)
    assert (per_oct > 20).all() and (per_oct < 250).all()
    assert not dead[:, 100:105].any()      # zero normal: stays (the collinear ones round to slivers)
    assert (dead[:, 50:100].sum(0) == 4).all()  # axis-aligned: dead in the four octants behind them
    assert dead[:, :50].sum(0).max() <= 4 and dead[:, :50].sum(0).min() < 4  # tilted: some are ambiguous
    T.compare(h1, h0, "soup hit")
    T.compare(t1, t0, "soup t")
    assert h0.sum() * 4 > n
