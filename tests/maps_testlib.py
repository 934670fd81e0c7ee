"""Test infrastructure for map sets (include/mpenv_maps.h, DESIGN.md §2
definition 19): the ctypes binding of the header's functions, the generated
maps A to E, an Engine made by mpenv_create_maps, and one oracle per range.

The maps are written under a directory that lives as long as the process;
none is committed.
  A  scenes/simple_map itself (LDS-resident)
  B  "blocks": one box per zone at the zone's xy centre, half-width 20, from
     the zone's min z to 200 above it (AUTO picks the global-resident path)
  C  "swapped": spawns.bin with the A and B lists exchanged
  D  four_zone_scene (4 zones)
  E  "nav-1": navmesh.bin without the face whose centroid is nearest the origin

Nothing here is imported by the product.
"""
import ctypes as C
import functools
import os
import shutil
import struct
import tempfile

import numpy as np

import big_scene
import mpenv_testlib as T

AUTO, LDS, GLOBAL = 0, 1, 2  # MPENV_SCENE_*
ERR_INVALID, ERR_IO, ERR_HIP, ERR_UNSUPPORTED = -1, -2, -3, -4
STATE_ERR_HEADER, STATE_ERR_MAP, STATE_ERR_CROSS_MAP = 1, 2, 4
MAX_MAP_RANGES = 32

vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32


class MapRange(C.Structure):
    _fields_ = [("scene_path", C.c_char_p), ("num_worlds", u32)]


class MapDesc(C.Structure):
    _fields_ = [("first_world", i32), ("num_worlds", i32), ("scene", i32), ("residency", i32), ("supported", i32),
                ("reason", C.c_char * 128)]


SIGNATURES = {
    "mpenv_create_maps": (i32, [C.POINTER(T.MpenvConfig), C.POINTER(MapRange), i32, C.POINTER(vp)]),
    "mpenv_num_maps": (i32, [vp, C.POINTER(i32)]),
    "mpenv_map_info": (i32, [vp, i32, C.POINTER(MapDesc), C.POINTER(C.c_char_p)]),
    "mpenv_map_of_world": (i32, [vp, C.POINTER(vp)]),
    "mpenv_maps_plan": (i32, [C.POINTER(T.MpenvConfig), C.POINTER(MapRange), i32, C.POINTER(MapDesc), C.POINTER(i32)]),
}


def lib():
    l = T.lib_mpenv()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    return l


# ------------------------------------------------------------------ the maps
_tmp = None


def _dir(name):
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="mpenv_maps_")
    return os.path.join(_tmp.name, name)


def _copy_scene(dst, skip=()):
    os.makedirs(dst, exist_ok=True)
    for f in ("collisions.bin", "navmesh.bin", "spawns.bin", "zones.bin"):
        if f not in skip:
            shutil.copy(os.path.join(T.SCENE, f), dst)
    return dst


def read_zones(path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[:4], np.uint32)[0])
    return np.frombuffer(raw[4:4 + 24 * n], np.float32).reshape(n, 6)


def _blocks(dst):
    c = big_scene.read_collisions(os.path.join(T.SCENE, "collisions.bin"))
    meshes = []
    for z in read_zones(os.path.join(T.SCENE, "zones.bin")):
        cx, cy = 0.5 * (z[0] + z[3]), 0.5 * (z[1] + z[4])
        meshes.append(big_scene.box_mesh((cx - 20, cy - 20, z[2]), (cx + 20, cy + 20, z[2] + 200.0)))
    _copy_scene(dst, skip=("collisions.bin",))
    big_scene.write_collisions(os.path.join(dst, "collisions.bin"), big_scene._append_meshes(c, meshes))
    return dst


def _swapped(dst):
    buf = open(os.path.join(T.SCENE, "spawns.bin"), "rb").read()
    off, lists = 0, []
    for _ in range(3):
        n = struct.unpack_from("<I", buf, off)[0]
        lists.append(buf[off:off + 4 + 32 * n])
        off += 4 + 32 * n
    assert off == len(buf)
    _copy_scene(dst, skip=("spawns.bin",))
    with open(os.path.join(dst, "spawns.bin"), "wb") as f:
        f.write(lists[1] + lists[0] + lists[2])
    return dst


def _nav_minus_one(dst):
    buf = open(os.path.join(T.SCENE, "navmesh.bin"), "rb").read()
    nv = struct.unpack_from("<I", buf, 0)[0]
    verts = np.frombuffer(buf, "<f4", 3 * nv, 4).reshape(nv, 3)
    off = 4 + 12 * nv
    nf = struct.unpack_from("<I", buf, off)[0]
    counts = np.frombuffer(buf, "<u4", nf, off + 4)
    off += 4 + 4 * nf
    ni = struct.unpack_from("<I", buf, off)[0]
    idx = np.frombuffer(buf, "<u4", ni, off + 4)
    assert off + 4 + 4 * ni == len(buf) and counts.sum() == ni
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cent = np.array([verts[idx[first[k]:first[k + 1]]].mean(0) for k in range(nf)])
    drop = int(np.argmin(np.linalg.norm(cent, axis=1)))
    keep = np.ones(nf, bool)
    keep[drop] = False
    new_idx = np.concatenate([idx[first[k]:first[k + 1]] for k in range(nf) if keep[k]])
    _copy_scene(dst, skip=("navmesh.bin",))
    with open(os.path.join(dst, "navmesh.bin"), "wb") as f:
        f.write(struct.pack("<I", nv) + verts.tobytes())
        f.write(struct.pack("<I", nf - 1) + counts[keep].astype("<u4").tobytes())
        f.write(struct.pack("<I", len(new_idx)) + new_idx.astype("<u4").tobytes())
    return dst


@functools.lru_cache(maxsize=None)
def scene(name):
    """The directory of map "A" .. "E", written on first use."""
    if name == "A":
        return T.SCENE
    d = T.four_zone_scene(_dir("D")) if name == "D" else {"B": _blocks, "C": _swapped, "E": _nav_minus_one}[name](_dir(name))
    if name != "B":
        # the same collisions.bin: simple_map's tuned lidar tree applies, and with it the LDS-resident path
        shutil.copy(os.path.join(T.SCENE, "lidar_tree.txt"), d)
    return d


def ranges_of(spec):
    """[("A", 2), ("B", 3)] -> [(directory, 2), (directory, 3)]"""
    return [(scene(k), n) for k, n in spec]


def _range_array(ranges):
    arr = (MapRange * max(len(ranges), 1))()
    for k, (path, n) in enumerate(ranges):
        arr[k].scene_path = path.encode() if path is not None else None
        arr[k].num_worlds = n
    return arr


def config(num_worlds, team_size, rand_seed=5, sim_flags=0, auto_reset=True, world_id_offset=0, task=T.TASK_ZONE,
           scene_path=None, replay=None, record=None, events=None, curriculum=None):
    e = [p.encode() if p else None for p in (scene_path, replay, record, events, curriculum)]
    return T.MpenvConfig(1, 0, num_worlds, rand_seed, int(auto_reset), sim_flags, task, team_size, 0, 0, e[0], 0,
                         e[1], e[2], e[3], e[4], world_id_offset)


def plan(ranges, team_size=3, num_worlds=None, **kw):
    """mpenv_maps_plan: (return code, [MapDesc per range], spawn_track_len, message)"""
    W = sum(n for _, n in ranges) if num_worlds is None else num_worlds
    cfg = config(W, team_size, **kw)
    desc = (MapDesc * max(len(ranges), 1))()
    track = i32(-1)
    rc = lib().mpenv_maps_plan(C.byref(cfg), _range_array(ranges), len(ranges), desc, C.byref(track))
    return rc, list(desc)[:min(len(ranges), MAX_MAP_RANGES)], track.value, lib().mpenv_last_error().decode()


def create(ranges, team_size=3, num_worlds=None, **kw):
    """mpenv_create_maps: (return code, handle or None, message)"""
    W = sum(n for _, n in ranges) if num_worlds is None else num_worlds
    cfg = config(W, team_size, **kw)
    h = vp()
    rc = lib().mpenv_create_maps(C.byref(cfg), _range_array(ranges), len(ranges), C.byref(h))
    return rc, (h if h.value else None), lib().mpenv_last_error().decode()


class MapEngine(T.Engine):
    """T.Engine over mpenv_create_maps: `ranges` is [(directory, worlds)]."""

    def __init__(self, ranges, team_size, **kw):
        self.lib = lib()
        self.mem = T.HipMem()
        self.ranges = list(ranges)
        rc, h, msg = create(self.ranges, team_size, **kw)
        assert rc == 0, msg
        self.h = h
        self.W, self.N = sum(n for _, n in ranges), 2 * team_size

    def num_maps(self):
        n = i32(-1)
        self._ok(self.lib.mpenv_num_maps(self.h, C.byref(n)))
        return n.value

    def map_info(self, r):
        d, p = MapDesc(), C.c_char_p()
        self._ok(self.lib.mpenv_map_info(self.h, r, C.byref(d), C.byref(p)))
        return dict(path=p.value.decode(), first_world=d.first_world, num_worlds=d.num_worlds, scene=d.scene,
                    residency=d.residency)

    def map_of_world(self):
        p = vp()
        self._ok(self.lib.mpenv_map_of_world(self.h, C.byref(p)))
        out = np.empty(self.W, np.int32)
        self.mem.d2h(p.value, out.nbytes, out)
        return out


@functools.lru_cache(maxsize=None)
def _trees(scene):
    return T.scene_bvh(scene), T.scene_bvh(scene, lidar=True)


class Oracle(T.Oracle):
    """T.Oracle with the scene's two trees built once per directory (they are
    most of an oracle's construction time, and these tests make dozens)."""

    def __init__(self, num_worlds, team_size, rand_seed=5, sim_flags=0, world_id_offset=0, scene=T.SCENE,
                 task=T.TASK_ZONE):
        self.lib = T.lib_oracle()
        (self.nodes, self.verts, _), (self.lnodes, self.lverts, _) = _trees(scene)
        cfg = T.OracleConfig(num_worlds, rand_seed, 1, sim_flags, team_size, world_id_offset, scene.encode(),
                             self.nodes.ctypes.data, len(self.nodes) // 64, self.verts.ctypes.data,
                             len(self.verts) // 3, task, 0, 1, self.lnodes.ctypes.data, len(self.lnodes) // 64,
                             self.lverts.ctypes.data, len(self.lverts) // 3)
        self.h = self.lib.oracle_create(C.byref(cfg))
        assert self.h, "oracle_create failed"
        self.W, self.N = num_worlds, 2 * team_size


class RangeOracles:
    """One oracle per range, as DESIGN.md §2 definition 19 states the
    contract: scene dir_r, n_r worlds, world_id_offset advanced by the range's
    first world; get() concatenates their exports in range order."""

    def __init__(self, ranges, team_size, world_id_offset=0, **kw):
        self.o, w0 = [], 0
        for path, n in ranges:
            self.o.append(Oracle(n, team_size, world_id_offset=world_id_offset + w0, scene=path, **kw))
            w0 += n
        self.W, self.N = w0, 2 * team_size

    def close(self):
        for o in self.o:
            o.close()

    def each(self, fn):
        return [fn(o) for o in self.o]

    def put_ctrl(self, ctrl):
        self.each(lambda o: o.put_ctrl(ctrl))

    def init(self):
        self.each(lambda o: o.init())

    def step(self):
        self.each(lambda o: o.step())

    def get(self, name):
        return np.concatenate(self.each(lambda o: o.get(name)))

    def explore(self):
        return np.concatenate(self.each(T.explore_visited))

    def seek_actions(self, step, seed=1234):
        """seek_combat_actions on each oracle's rows, concatenated (the tape
        rows of an oracle start at agent 0 of its range, as a single-map
        manager's would)."""
        acts = self.each(lambda o: T.seek_combat_actions(o, step, seed))
        for o, a in zip(self.o, acts):
            o.set_actions(a)
        return np.concatenate(acts)

    def set_policy(self, col):
        """AGENT_POLICY [A, 1] over the batch, cut by range"""
        a0 = 0
        for o in self.o:
            o.view("AGENT_POLICY")[:] = col[a0:a0 + o.W * o.N]
            a0 += o.W * o.N


COMPARED = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS


def compare_all(e, ref, tag):
    """Every STEP_OUTPUTS and DEBUG_OUTPUTS export and the explore cells."""
    for name in COMPARED:
        T.compare(e.get(name), ref.get(name), f"{tag} {name}")
    T.compare(T.explore_visited(e), ref.explore() if isinstance(ref, RangeOracles) else T.explore_visited(ref),
              f"{tag} explore")


def scenes_differ_by(path_a, path_b, team_size, n, world_id_offset, steps=5, bots=False, **kw):
    """The parity tests' precondition, from oracles alone: the first step
    (0 = init) by which oracles on the two scenes over the same world range
    and offset differ in a compared output, or None."""
    pair = [Oracle(n, team_size, world_id_offset=world_id_offset, scene=p, **kw) for p in (path_a, path_b)]
    try:
        for o in pair:
            o.put_ctrl([0, 1, 1])
            if bots:
                pol = o.view("AGENT_POLICY")
                pol.reshape(n, 2 * team_size)[:, team_size:] = -1
            o.init()
        for step in range(steps + 1):
            if any(not np.array_equal(pair[0].get(nm).view(np.uint32), pair[1].get(nm).view(np.uint32))
                   for nm in COMPARED):
                return step
            for o in pair:
                o.set_actions(T.seek_combat_actions(o, step))
                o.step()
        return None
    finally:
        for o in pair:
            o.close()
