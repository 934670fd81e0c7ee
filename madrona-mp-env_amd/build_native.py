"""Builds the native parts of the engine in-tree (no JIT cache, no pip).

Outputs (git-ignored, shipped to the GPU box with the snapshot):
  madrona-mp-env_amd/libmpenv.so                     HIP kernels + C ABI (gfx950)
  madrona-mp-env_amd/madrona_mp_env<ext-suffix>.so   Python module (pybind11)
  oracle/_build/liboracle.so                         CPU parity oracle (tests only)

Every float translation unit is compiled with -ffp-contract=off so the host
oracle and the gfx950 kernels round identically (see csrc/mpenv_core.h).
"""
import os
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
ORACLE = os.path.join(ROOT, "oracle")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("MPENV_OFFLOAD_ARCH", "gfx950")

LIB = os.path.join(PKG, "libmpenv.so")
EXT = os.path.join(PKG, "madrona_mp_env" + sysconfig.get_config_var("EXT_SUFFIX"))
ORACLE_LIB = os.path.join(ORACLE, "_build", "liboracle.so")

LIB_SOURCES = ["kernels.hip", "move.hip", "vis.hip", "obs.hip", "lidar.hip", "hooks.hip", "wire.hip", "state.hip",
               "policy.hip", "camera.hip", "league.hip", "curriculum.hip", "manager.cpp", "manager_scene.cpp",
               "camera.cpp", "league.cpp", "curriculum.cpp", "policy.cpp", "scene.cpp", "navmesh.cpp"]
API_HEADERS = [os.path.join(INCLUDE, h) for h in ("mpenv.h", "mpenv_policy_slots.h", "mpenv_policy_precision.h",
                                                     "mpenv_scene_residency.h", "mpenv_camera.h", "mpenv_maps.h",
                                                     "mpenv_league.h", "mpenv_curriculum.h")]
MAX_PARALLEL = 16  # what one command may use on the GPU machines, whatever the machine's CPU count


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    # stderr: callers such as bench.py own stdout (one JSON line)
    print("[build]", " ".join(cmd), file=sys.stderr, flush=True)
    subprocess.run(cmd, check=True, stdout=sys.stderr)


def compile_flags(src_dir, extra=()):
    """The flags every translation unit of libmpenv.so is compiled with."""
    return ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", f"-I{src_dir}", f"-I{INCLUDE}",
            "-Wall", "-Wno-unused-variable", "-Wno-unused-function"] + list(extra)


def compile_cmd(src, out, src_dir, extra=(), mode=("-c",)):
    """hipcc line for one of LIB_SOURCES; `mode` is what to emit (-c, -S, -fsyntax-only ...),
    `out` None for a mode that writes no file."""
    to = ["-o", out] if out else []
    if src.endswith(".hip"):
        return [HIPCC, "-x", "hip", f"--offload-arch={ARCH}", *mode, src] + to + compile_flags(src_dir, extra)
    return ([HIPCC, "-x", "c++", *mode, src] + to + compile_flags(src_dir, extra) +
            ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"])


def _compile(cmd):
    # one print per unit, command and compiler output together, so concurrent units do not interleave
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print("[build] " + " ".join(cmd) + "\n" + r.stdout, end="", file=sys.stderr, flush=True)
    return r.returncode


def compile_and_link(src_dir, objdir, out, extra=(), force=True):
    """The one compile recipe: LIB_SOURCES of `src_dir` into objects under
    `objdir`, concurrently, then linked into the shared library `out`.
    force=False recompiles only the objects older than their source or any
    header, and relinks when an object is newer than the library."""
    headers = [os.path.join(src_dir, h) for h in sorted(os.listdir(src_dir)) if h.endswith(".h")] + API_HEADERS
    srcs = [os.path.join(src_dir, s) for s in LIB_SOURCES]
    objs = [os.path.join(objdir, s + ".o") for s in LIB_SOURCES]
    if not force and not _stale(out, srcs + headers + [o for o in objs if os.path.exists(o)]):
        return out  # up to date, with or without its objects (a tree may travel without them)
    os.makedirs(objdir, exist_ok=True)
    todo = [compile_cmd(src, o, src_dir, extra) for src, o in zip(srcs, objs)
            if force or _stale(o, [src] + headers)]
    if todo:
        jobs = max(1, min(MAX_PARALLEL, int(os.environ.get("MAX_JOBS") or MAX_PARALLEL), len(todo)))
        with ThreadPoolExecutor(jobs) as pool:
            codes = list(pool.map(_compile, todo))
        failed = [cmd for cmd, rc in zip(todo, codes) if rc]
        if failed:
            # last, below every unit's output: which units failed
            for cmd in failed:
                print("[build] FAILED:", next(a for a in cmd if a.endswith((".hip", ".cpp"))), file=sys.stderr, flush=True)
            raise subprocess.CalledProcessError(1, failed[0])
    if todo or _stale(out, objs):
        _run([HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", out] + objs + ["-Wl,-soname,libmpenv.so"])
    return out


def build_lib(force=False):
    return compile_and_link(CSRC, os.path.join(PKG, "build"), LIB, force=force)


def build_ext(force=False):
    src = os.path.join(CSRC, "pybind_module.cpp")
    if not os.path.exists(src):
        return None
    if not force and not _stale(EXT, [src, LIB] + API_HEADERS):
        return EXT
    import pybind11
    py_inc = sysconfig.get_paths()["include"]
    _run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{pybind11.get_include()}",
          f"-I{py_inc}", f"-I{INCLUDE}", src, "-o", EXT, f"-L{PKG}", "-lmpenv",
          "-Wl,-rpath,$ORIGIN"])
    return EXT


HEADLESS = os.path.join(PKG, "headless")


def build_headless(force=False):
    """C++ driver over include/mpenv_manager.hpp (reference src/headless.cpp role)."""
    src = os.path.join(CSRC, "headless.cpp")
    deps = [src, LIB, os.path.join(INCLUDE, "mpenv_manager.hpp"), os.path.join(CSRC, "mpenv_core.h")] + API_HEADERS
    if not force and not _stale(HEADLESS, deps):
        return HEADLESS
    _run([HIPCC, "-x", "c++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
          f"-I{INCLUDE}", f"-I{CSRC}", src, "-o", HEADLESS, f"-L{PKG}", "-lmpenv",
          "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"])
    return HEADLESS


def build_oracle(force=False):
    src = os.path.join(ORACLE, "oracle.cpp")
    deps = [src, os.path.join(ORACLE, "oracle.h"), os.path.join(CSRC, "mpenv_core.h"),
            os.path.join(INCLUDE, "mpenv.h")]
    if not force and not _stale(ORACLE_LIB, deps):
        return ORACLE_LIB
    os.makedirs(os.path.dirname(ORACLE_LIB), exist_ok=True)
    _run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
          "-Wall", "-Wno-invalid-offsetof", f"-I{INCLUDE}", f"-I{CSRC}", src, "-o", ORACLE_LIB,
          "-lpthread"])
    return ORACLE_LIB


def build_all(force=True):
    """Every artefact, recompiled from source by default (build() must never
    ship binaries it did not compile); force=False is the incremental mode
    the test harness uses when a build already ran in this tree."""
    build_lib(force)
    build_ext(force)
    build_headless(force)
    build_oracle(force)


if __name__ == "__main__":
    build_all(force="--incremental" not in sys.argv)
