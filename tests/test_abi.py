"""The drop-in boundary without a GPU: library load, exported symbols,
Python module surface (src/bindings.cpp:11-160) and loud failure modes."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

import mpenv_testlib as T

HEADER = os.path.join(T.ROOT, "include", "mpenv.h")
HERE = os.path.dirname(os.path.abspath(__file__))


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mpenv_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_manager_surface():
    fns = declared_functions()
    for f in ("mpenv_create", "mpenv_destroy", "mpenv_init", "mpenv_step", "mpenv_step_async",
              "mpenv_gpu_stream_init", "mpenv_gpu_stream_step", "mpenv_export_tensor",
              "mpenv_trigger_reset", "mpenv_set_pvp_action", "mpenv_set_hp",
              "mpenv_train_interface_size", "mpenv_train_interface_entry", "mpenv_copy_actions"):
        assert f in fns, f


def declarations():
    """{function: (return type, [parameter types])} as the header spells
    them, a pointer or array parameter reduced to "*"."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    pattern = r"^([A-Za-z_][\w ]*?[ *]+)(mpenv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;"  # type name(params); over 1-3 lines
    for ret, name, params in re.findall(pattern, text, flags=re.M):
        kinds = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = p.replace("const", " ").split()
            kinds.append("*" if "*" in p or "[" in p else " ".join(words[:-1]))
        out[name] = (" ".join(ret.replace("*", " * ").split()), kinds)
    return out


def test_binding_table_matches_header():
    """tests/mpenv_abi.py SIGNATURES, the one ctypes binding every test and
    tool calls through, against include/mpenv.h: the same functions, the same
    number of parameters, every pointer pointer-sized and every integer of the
    declared width (ctypes would otherwise pass a 64-bit address as a C int)."""
    from mpenv_abi import SIGNATURES

    decl = declarations()
    assert sorted(decl) == declared_functions()  # the parser saw every declaration
    assert sorted(SIGNATURES) == sorted(decl), set(SIGNATURES) ^ set(decl)
    returns = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "void": None, "const char *": C.c_char_p}
    values = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "size_t": C.c_size_t}
    for name, (ret, kinds) in decl.items():
        restype, argtypes = SIGNATURES[name]
        assert restype is returns[ret], (name, ret, restype)
        assert len(argtypes) == len(kinds), (name, kinds, argtypes)
        for k, (kind, at) in enumerate(zip(kinds, argtypes)):
            if kind == "*":
                assert at in (C.c_void_p, C.c_char_p) or issubclass(at, C._Pointer), (name, k, at)
            else:
                assert at is values[kind], (name, k, kind, at)


def test_library_exports_every_declared_symbol():
    lib = T.lib_mpenv()
    missing = [f for f in declared_functions() if not hasattr(lib, f)]
    assert not missing, missing
    out = subprocess.run(["nm", "-D", "--defined-only", T.build_native.LIB], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mpenv_\w+)", out))
    assert set(declared_functions()) <= exported
    assert lib.mpenv_abi_version() == 1


def test_library_has_gfx950_code_object():
    sections = subprocess.run(["readelf", "-S", T.build_native.LIB], capture_output=True, text=True,
                              check=True).stdout
    assert ".hip_fatbin" in sections
    assert b"amdgcn-amd-amdhsa--gfx950" in open(T.build_native.LIB, "rb").read()


def test_oracle_is_not_linked_into_the_product():
    for so in (T.build_native.LIB, T.build_native.EXT):
        out = subprocess.run(["ldd", so], capture_output=True, text=True).stdout
        assert "oracle" not in out
        assert b"oracle_" not in open(so, "rb").read()


def test_scene_bvh_query_needs_no_gpu():
    nodes, verts, max_stack = T.scene_bvh()
    assert len(nodes) // 64 == 61 and len(verts) // 9 == 252 and max_stack <= 16


def _cfg(**kw):
    c = T.MpenvConfig(1, 0, 4, 5, 1, 0, 2, 3, 0, 0, T.SCENE.encode(), 0, None, None, None, None, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("kw,needle", [
    (dict(exec_mode=0), "CPU"),
    (dict(task_type=1), "Zone"),
    (dict(team_size=7), "team"),
    (dict(num_worlds=0), "world"),
    (dict(sim_flags=1 << 12), "sim_flags"),
    (dict(scene_path=b"/nonexistent"), ""),
])
def test_create_rejects_unsupported_configs(kw, needle):
    lib = T.lib_mpenv()
    h = C.c_void_p()
    rc = lib.mpenv_create(C.byref(_cfg(**kw)), C.byref(h))
    assert rc != 0 and not h.value
    msg = lib.mpenv_last_error().decode()
    assert needle.lower() in msg.lower(), msg


@pytest.mark.gpu
def test_create_error_codes(tmp_path):
    """What mpenv_create returns once a device is there (without one it stops
    at "no HIP device available"): a scene or curriculum file that cannot be
    opened or a collisions.bin with a mesh range past its arrays is
    MPENV_ERR_IO, a scene the task cannot use MPENV_ERR_HIP."""
    lib = T.lib_mpenv()

    def create(**kw):
        h = C.c_void_p()
        rc = lib.mpenv_create(C.byref(_cfg(**kw)), C.byref(h))
        assert not h.value
        return rc, lib.mpenv_last_error().decode()

    rc, msg = create(scene_path=str(tmp_path / "no_such_scene").encode())
    assert rc == -2 and "open" in msg, (rc, msg)  # MPENV_ERR_IO
    rc, msg = create(curriculum_data_path=str(tmp_path / "no_such_file").encode())
    assert rc == -2 and "open" in msg, (rc, msg)
    rc, msg = create(task_type=T.TASK_ZONE_CAPTURE_DEFEND)  # simple_map has three zones
    assert rc == -3 and ">= 4 zones" in msg, (rc, msg)  # MPENV_ERR_HIP
    # a collisions.bin whose last mesh claims more triangles than the file holds: the file's last
    # 16 bytes are that mesh's (vertexOffset, numVertices, triOffset, numTris)
    bad = tmp_path / "bad_mesh_range"
    bad.mkdir()
    for f in ("collisions.bin", "navmesh.bin", "spawns.bin", "zones.bin"):
        shutil.copy(os.path.join(T.SCENE, f), bad)
    raw = bytearray((bad / "collisions.bin").read_bytes())
    raw[-4:] = struct.pack("<I", 0x7FFFFFFF)
    (bad / "collisions.bin").write_bytes(bytes(raw))
    rc, msg = create(scene_path=str(bad).encode())
    assert rc == -2 and "range outside" in msg and "truncated or malformed" in msg, (rc, msg)


def test_every_manager_call_refuses_a_null_handle():
    """Each function that takes the manager handle first and returns a code,
    called with a null handle and zero or null for the rest."""
    from mpenv_abi import SIGNATURES

    lib = T.lib_mpenv()
    calls = [n for n, (ret, args) in SIGNATURES.items() if ret is C.c_int32 and args and args[0] is C.c_void_p]
    assert len(calls) >= 44  # the selection finds them
    for name in calls:
        args = [None if a is C.c_void_p or a is C.c_char_p or issubclass(a, C._Pointer) else 0
                for a in SIGNATURES[name][1]]
        # the error text is per thread and stays: put a known other one there first
        assert lib.mpenv_scene_quirk_grid(None, None, None, None) == -1
        assert lib.mpenv_last_error() == b"num_words is null"
        assert getattr(lib, name)(*args) == -1, name  # MPENV_ERR_INVALID
        msg = lib.mpenv_last_error().decode()
        assert msg != "num_words is null" and ("null" in msg or "argument" in msg), (name, msg)


def test_python_module_surface():
    import madrona_mp_env as m

    assert m.madrona.ExecMode.CUDA is not None and m.madrona.ExecMode.CPU is not None
    assert int(m.Task.Zone) == 2
    flags = m.SimFlags.SpawnInMiddle | m.SimFlags.RandomizeHPMagazine
    assert int(flags) == 3
    # every getter src/bindings.cpp:110-158 defines, plus the extensions
    for name in ("init", "step", "fwd_lidar", "rear_lidar", "hp", "magazine", "alive", "self_obs",
                 "filters_state", "teammates", "opponents", "opponents_last_known", "self_pos",
                 "teammate_positions", "opponent_positions", "opponent_last_known_positions",
                 "opponent_masks", "agent_map", "unmasked_agent_map", "reward_coefs",
                 "explore_action_tensor", "pvp_action_tensor", "aim_action_tensor", "reward_tensor",
                 "done_tensor", "reset_tensor", "self_observation_tensor", "jax",
                 "step_async", "train_interface", "copy_actions", "kernel_timings"):
        assert hasattr(m.SimManager, name), name


def test_python_module_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import madrona_mp_env as m

    with pytest.raises(Exception) as ei:
        m.SimManager(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=2, rand_seed=5,
                     auto_reset=True, sim_flags=m.SimFlags.Default, task_type=m.Task.Zone,
                     team_size=1, num_pbt_policies=0, policy_history_size=0,
                     scene_path=T.SCENE)
    assert "device" in str(ei.value).lower() or "hip" in str(ei.value).lower()


def test_cpp_manager_headless_builds_and_fails_loudly_without_gpu():
    """include/mpenv_manager.hpp (the mgr.hpp Manager class) compiles into the
    headless driver; without a device it exits non-zero with a message."""
    import torch

    exe = T.build_native.HEADLESS
    assert os.path.exists(exe)
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([exe, "CUDA", "2", "1", T.SCENE], capture_output=True, text=True)
    assert r.returncode != 0 and "device" in r.stderr.lower()


def test_caller_written_against_mgr_hpp_compiles_and_out_of_scope_parts_throw(tmp_path):
    """tests/mgr_hpp_caller.cpp names every public Manager method with the
    reference's signature (src/mgr.hpp:54-157, incl. Manager(cfg, VizState*),
    vizStep, getWorldContext, setExploreAction, setCoarsePvPAction) and runs
    without a GPU: a non-null VizState and ExecMode::CPU are refused."""
    exe = str(tmp_path / "mgr_caller")
    pkg = T.PKG
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "mgr_hpp_caller.cpp"), "-o", exe, "-L", pkg, "-lmpenv",
                    f"-Wl,-rpath,{pkg}"], check=True)
    r = subprocess.run([exe, T.SCENE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "mgr.hpp caller ok" in r.stdout


def test_product_kernels_carry_no_lab_switches_and_lab_patches_apply(tmp_path):
    """Only the shipped configuration is in csrc/ (no lab hooks or dropped
    variants behind compile-time switches); any lab overlay under tools/lab/
    still applies to it, so kernel_lab variants keep building.  (Round 6
    retired the round-1..5 lab_hooks.patch: it is in git history before
    commit "retire lab_hooks.patch".)"""
    import shutil

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "madrona-mp-env_amd", "csrc")
    switch = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b.*\bMPENV_", re.M)
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".cpp")):
            text = open(os.path.join(csrc, f)).read()
            assert not switch.search(text), f"compile-time MPENV_ switch left in {f}"
            assert "MPENV_LAB" not in text and "MP_LAB_" not in text, f"lab hook left in {f}"
    lab = os.path.join(root, "tools", "lab")
    patches = sorted(p for p in os.listdir(lab) if p.endswith(".patch")) if os.path.isdir(lab) else []
    for p in patches:
        work = tmp_path / p
        shutil.copytree(csrc, work)
        # a patch may build on others ("# requires: a.patch b.patch" first line)
        first = open(os.path.join(lab, p)).readline()
        chain = first.split(":", 1)[1].split() if first.startswith("# requires:") else []
        for q in chain + [p]:
            r = subprocess.run(["patch", "-p1", "-d", str(work), "-i", os.path.join(lab, q)],
                               capture_output=True, text=True)
            assert r.returncode == 0 and "fuzz" not in r.stdout, (p, q, r.stdout, r.stderr)


CSRC = os.path.join(T.ROOT, "madrona-mp-env_amd", "csrc")


def test_every_source_file_is_built():
    """Every .hip / .cpp of csrc/ is a unit of libmpenv.so or one of the two
    separately built programs: a new file cannot be forgotten."""
    built = set(T.build_native.LIB_SOURCES) | {"pybind_module.cpp", "headless.cpp"}
    found = {f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp"))}
    assert found == built, (sorted(found - built), sorted(built - found))
    assert len(T.build_native.LIB_SOURCES) == len(set(T.build_native.LIB_SOURCES))


def _kernel_lab():
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_lab", os.path.join(T.ROOT, "tools", "kernel_lab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ksim_body(text, head):
    a = text.index(head) + len(head)
    depth, k = 1, a
    while depth:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
    return text[a:k - 1]


def test_ksim_lab_hooks_apply(tmp_path):
    """kernel_lab's k_sim hooks land in k_sim's body where it now is: one
    phase timer per block barrier, every KSIM_SKIP phase behind its switch,
    and the hooked file still compiles (device side, syntax only)."""
    lab = _kernel_lab()
    work = tmp_path / "src"
    shutil.copytree(CSRC, work)
    path = os.path.join(work, lab.KSIM_FILE)
    before = _ksim_body(open(path).read(), lab.KSIM_HEAD)
    barriers = before.count("__syncthreads();")
    assert barriers > 0
    lab.ksim_hooks(path)
    hooked = open(path).read()
    # "MP_PT()" also stands in the two #define lines of the prelude
    assert hooked.count("MP_PT();") == barriers and hooked.count("__syncthreads(); MP_PT();") == barriers
    for name, bit in lab.KSIM_SKIP:
        calls = before.count(name)
        assert calls >= 1, name
        assert hooked.count(f"(MPENV_LAB_SIM_SKIP & {bit}) ? (void)0 : (void){name}") == calls, name
    assert hooked.count("MPENV_LAB_SIM_SKIP &") == sum(before.count(name) for name, _ in lab.KSIM_SKIP)
    B = T.build_native
    cmd = B.compile_cmd(path, None, str(work), extra=["-DMPENV_LAB_PHASE_T", "-DMPENV_LAB_SIM_SKIP=1"],
                        mode=("--cuda-device-only", "-fsyntax-only"))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_ksim_lab_hooks_refuse_a_missing_anchor(tmp_path):
    """With k_sim's body head gone from the copy the hooks raise instead of
    leaving the kernel as it was."""
    lab = _kernel_lab()
    work = tmp_path / "src"
    shutil.copytree(CSRC, work)
    path = os.path.join(work, lab.KSIM_FILE)
    text = open(path).read()
    assert lab.KSIM_HEAD in text
    open(path, "w").write(text.replace(lab.KSIM_HEAD, lab.KSIM_HEAD.replace("simBody", "simBodyMoved")))
    with pytest.raises(ValueError, match="body head"):
        lab.ksim_hooks(path)


_XLA_CALL = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[3])
import mpenv_abi
fake = sys.argv[2]
if fake:
    C.CDLL(fake, mode=C.RTLD_GLOBAL)
lib = mpenv_abi.bind(C.CDLL(sys.argv[1]))
Fn = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t)
FnS = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t, C.c_void_p)
bad = bytes(24)
if fake:
    f = FnS(C.cast(lib.mpenv_xla_gpu_stream_step_status, C.c_void_p).value)
    status = C.create_string_buffer(8)
    f(None, None, bad, len(bad), C.cast(status, C.c_void_p))
    got = C.CDLL(fake).fake_status_message
    got.restype = C.c_char_p
    print("status:", got().decode(), "errors:", lib.mpenv_xla_errors())
else:
    f = Fn(C.cast(lib.mpenv_xla_gpu_stream_step, C.c_void_p).value)
    f(None, None, bad, len(bad))
    print("returned")
"""


def test_xla_v1_target_aborts_on_a_foreign_opaque():
    """The API-v1 custom call has no error channel: like the reference's
    REQ_CUDA / FATAL (src/mgr.cpp:514-531, 620-638) a bad opaque prints why
    and aborts instead of leaving XLA with unwritten result buffers.  Run in a
    subprocess that never touches a GPU (the opaque check fails first)."""
    import sys

    r = subprocess.run([sys.executable, "-c", _XLA_CALL, T.build_native.LIB, "", HERE], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout
    assert "mpenv: XLA custom call gpuStreamStep failed: bad XLA opaque" in r.stderr, r.stderr


def test_xla_status_target_reports_failure_through_xla(tmp_path):
    """The status-returning twin hands the failure to XLA's
    XlaCustomCallStatusSetFailure (resolved at run time; here a stand-in
    library exports it) and returns; the failure is counted."""
    import sys

    src = tmp_path / "fake_xla.c"
    src.write_text('#include <string.h>\n#include <stddef.h>\nstatic char msg[512];\n'
                   'void XlaCustomCallStatusSetFailure(void *s, const char *m, size_t n)\n'
                   '{ (void)s; if (n > 511) n = 511; memcpy(msg, m, n); msg[n] = 0; }\n'
                   'const char *fake_status_message(void) { return msg; }\n')
    so = tmp_path / "libfake_xla.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    r = subprocess.run([sys.executable, "-c", _XLA_CALL, T.build_native.LIB, str(so), HERE], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "status: mpenv: gpuStreamStep: bad XLA opaque" in r.stdout and "errors: 1" in r.stdout, r.stdout
