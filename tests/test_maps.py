"""Map sets without a GPU (include/mpenv_maps.h; DESIGN.md §2 definition 19):
what mpenv_maps_plan makes of a list, every refusal by its words, the
library's exports, the Python module's surface and a C++ caller.  The list is
checked before mpenv_create_maps touches a device, so its refusals are
asserted here too."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import maps_testlib as M
import mpenv_testlib as T
import scene_residency_testlib as R

HEADER = os.path.join(T.ROOT, "include", "mpenv_maps.h")


def test_generated_maps_are_what_the_tests_assume():
    rc, info = R.scene_info(M.scene("B"))
    assert rc == 0 and info.supported == 1
    assert info.collision_nodes == 70 and info.lds_bytes_lidar == 77312 and info.residency == R.GLOBAL
    for k in "ACDE":
        rc, info = R.scene_info(M.scene(k))
        assert rc == 0 and info.supported == 1 and info.residency == R.LDS, k
    assert len(M.read_zones(os.path.join(M.scene("D"), "zones.bin"))) == 4
    assert T.scene_navmesh(M.scene("A"))[0].shape[0] == 155
    assert T.scene_navmesh(M.scene("E"))[0].shape[0] == 154


def test_plan_of_a_mixed_set():
    spec = [("A", 2), ("B", 3), ("C", 1), ("D", 2), ("B", 4)]
    rc, desc, track, msg = M.plan(M.ranges_of(spec))
    assert rc == 0, msg
    assert [d.first_world for d in desc] == [0, 2, 5, 6, 8]
    assert [d.num_worlds for d in desc] == [2, 3, 1, 2, 4]
    assert [d.residency for d in desc] == [M.LDS, M.GLOBAL, M.LDS, M.LDS, M.GLOBAL]
    assert [d.scene for d in desc] == [0, 1, 2, 3, 1]  # equal paths share one loaded scene
    assert all(d.supported == 1 for d in desc)
    assert b"k_lidar" in desc[1].reason  # why B is not LDS-resident
    # the common row shape: the largest of the scenes' own, each what a single-map manager would use
    own = []
    for k, _ in spec:
        rc, _, t, msg = M.plan(M.ranges_of([(k, 1)]))
        assert rc == 0, msg
        own.append(t)
    assert track == max(own) and track >= 128


def _refused(ranges, code, *needles, **kw):
    """By mpenv_maps_plan and, before any device is touched, by mpenv_create_maps."""
    rc, _, _, msg = M.plan(ranges, **kw)
    assert rc == code, (rc, msg)
    for n in needles:
        assert n in msg, (n, msg)
    rc, h, msg2 = M.create(ranges, **kw)
    assert rc == code and h is None and msg2 == msg, (rc, msg2)


def test_refusals_name_the_range(tmp_path):
    A, B = M.scene("A"), M.scene("B")
    _refused([(A, 2), (B, 3)], M.ERR_INVALID, "hold 5 worlds", "num_worlds is 6", num_worlds=6)
    _refused([(A, 2), (B, 0)], M.ERR_INVALID, "map range 1", B, "at least one world", num_worlds=2)
    _refused([(A, 1)] * 33, M.ERR_INVALID, "33 ranges", "32")
    _refused([], M.ERR_INVALID, "0 ranges", num_worlds=1)
    missing = str(tmp_path / "no_such_map")
    _refused([(A, 1), (missing, 1)], M.ERR_IO, "map range 1", missing, "open")
    sliver = R.slivers(70000)
    _refused([(A, 1), (B, 1), (sliver, 2)], M.ERR_INVALID, "map range 2", sliver, "collision triangles")
    D = M.scene("D")
    _refused([(D, 1), (A, 2), (D, 1)], M.ERR_INVALID, "map range 1", A, ">= 4 zones", task=T.TASK_ZONE_CAPTURE_DEFEND)
    rc, _, _, msg = M.plan([(D, 1), (D, 3)], task=T.TASK_ZONE_CAPTURE_DEFEND)
    assert rc == 0, msg
    _refused([(A, 2)], M.ERR_INVALID, "scene_path must be null", scene_path=A)


def test_plan_marks_the_refused_map():
    rc, desc, _, _ = M.plan(M.ranges_of([("D", 1), ("A", 2)]), task=T.TASK_ZONE_CAPTURE_DEFEND)
    assert rc == M.ERR_INVALID
    assert desc[0].supported == 1 and desc[1].supported == 0 and b">= 4 zones" in desc[1].reason


def test_logs_and_curricula_are_unsupported(tmp_path):
    for key in ("replay", "record", "events", "curriculum"):
        rc, h, msg = M.create(M.ranges_of([("A", 1), ("B", 1)]), **{key: str(tmp_path / "x")})
        assert rc == M.ERR_UNSUPPORTED and h is None and "not supported" in msg and "one map" in msg, (key, rc, msg)


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.findall(r"^int\s+(mpenv_\w+)\s*\(", src, flags=re.M)


def test_library_exports_every_declared_function():
    names = declared_functions()
    assert sorted(names) == sorted(M.SIGNATURES), names
    out = subprocess.run(["nm", "-D", "--defined-only", T.build_native.LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (mpenv_\w+)", out))
    assert set(names) <= exported
    assert '#include "mpenv_maps.h"' in open(os.path.join(T.ROOT, "include", "mpenv.h")).read()
    src = open(HEADER).read()
    assert "#define MPENV_MAX_MAP_RANGES 32" in src and "#define MPENV_STATE_ERR_CROSS_MAP 4u" in src


def test_null_arguments_are_refused():
    l = M.lib()
    n, p, d = C.c_int32(), C.c_void_p(), M.MapDesc()
    assert l.mpenv_num_maps(None, C.byref(n)) == M.ERR_INVALID
    assert l.mpenv_map_info(None, 0, C.byref(d), None) == M.ERR_INVALID
    assert l.mpenv_map_of_world(None, C.byref(p)) == M.ERR_INVALID
    assert l.mpenv_maps_plan(None, None, 1, None, None) == M.ERR_INVALID
    assert l.mpenv_create_maps(None, None, 1, C.byref(p)) == M.ERR_INVALID


def test_python_module_surface():
    import madrona_mp_env as m

    for name in ("maps", "world_map_tensor"):
        assert hasattr(m.SimManager, name), name
    doc = m.SimManager.__init__.__doc__
    assert "scene_path: object" in doc  # a str or a list of (directory, worlds)
    spec = M.ranges_of([("A", 8), ("B", 4), ("A", 4)])
    out = m.maps_plan(spec, team_size=6)
    assert out["spawn_track_len"] >= 128
    assert [(d["path"], d["first_world"], d["num_worlds"], d["residency"], d["scene"]) for d in out["maps"]] == [
        (spec[0][0], 0, 8, "lds", 0), (spec[1][0], 8, 4, "global", 1), (spec[0][0], 12, 4, "lds", 0)]
    assert "task_type" in m.maps_plan.__doc__ and "sim_flags" in m.maps_plan.__doc__
    with pytest.raises(RuntimeError, match="map range 0 .*>= 4 zones"):
        m.maps_plan(spec, 6, task_type=m.Task.ZoneCaptureDefend)
    with pytest.raises(RuntimeError, match="at least one world"):
        m.maps_plan([(spec[0][0], 0)], 6)


def test_python_manager_refuses_a_bad_list_before_the_gpu():
    import madrona_mp_env as m

    with pytest.raises(RuntimeError, match="hold 3 worlds, num_worlds is 4"):
        m.SimManager(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=4, rand_seed=5, auto_reset=True,
                     sim_flags=m.SimFlags.Default, task_type=m.Task.Zone, team_size=1, num_pbt_policies=0,
                     policy_history_size=0, scene_path=[(M.scene("A"), 1), (M.scene("B"), 2)])


def test_cpp_caller_compiles_against_config_maps(tmp_path):
    exe = str(tmp_path / "maps_caller")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "maps_caller.cpp"), "-o", exe, "-L", T.PKG, "-lmpenv",
                    f"-Wl,-rpath,{T.PKG}"], check=True)
    r = subprocess.run([exe, T.SCENE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "maps caller ok" in r.stdout


def test_headless_takes_map_options():
    r = subprocess.run([T.build_native.HEADLESS, "CUDA", "4", "1", T.SCENE, "--map", T.SCENE + ":1", "--map",
                        M.scene("B") + ":2"], capture_output=True, text=True)
    assert r.returncode != 0 and "hold 3 worlds, num_worlds is 4" in r.stderr, r.stderr
    r = subprocess.run([T.build_native.HEADLESS, "CUDA", "4", "1", T.SCENE, "--map", T.SCENE], capture_output=True,
                       text=True)
    assert r.returncode != 0 and "DIR:N" in r.stderr, r.stderr
