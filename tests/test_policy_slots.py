"""The per-slot policy calls at the ABI boundary, without a GPU:
include/mpenv_policy_slots.h against tests/policy_slots_abi.py and the
library, and include/mpenv.h still declaring exactly what tests/mpenv_abi.py
binds (a declaration that strays into the wrong header shows here too)."""
import ctypes as C
import os
import re
import subprocess

import mpenv_testlib as T

INCLUDE = os.path.join(T.ROOT, "include")
SLOTS_HEADER = os.path.join(INCLUDE, "mpenv_policy_slots.h")
MAIN_HEADER = os.path.join(INCLUDE, "mpenv.h")


def header_text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def named_functions(path):
    """every mpenv_* name followed by "(" outside comments"""
    return sorted(set(re.findall(r"\b(mpenv_[a-z0-9_]+)\s*\(", header_text(path))))


def declarations(path):
    """{function: (return type, [parameter types])} as the header spells
    them, a pointer or array parameter reduced to "*"."""
    out = {}
    pattern = r"^([A-Za-z_][\w ]*?[ *]+)(mpenv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;"  # type name(params); over 1-3 lines
    for ret, name, params in re.findall(pattern, header_text(path), flags=re.M):
        kinds = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = p.replace("const", " ").split()
            kinds.append("*" if "*" in p or "[" in p else " ".join(words[:-1]))
        out[name] = (" ".join(ret.replace("*", " * ").split()), kinds)
    return out


def check_table(signatures, decl):
    returns = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "void": None, "const char *": C.c_char_p}
    values = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "size_t": C.c_size_t}
    assert sorted(signatures) == sorted(decl), set(signatures) ^ set(decl)
    for name, (ret, kinds) in decl.items():
        restype, argtypes = signatures[name]
        assert restype is returns[ret], (name, ret, restype)
        assert len(argtypes) == len(kinds), (name, kinds, argtypes)
        for k, (kind, at) in enumerate(zip(kinds, argtypes)):
            if kind == "*":
                assert at in (C.c_void_p, C.c_char_p) or issubclass(at, C._Pointer), (name, k, at)
            else:
                assert at is values[kind], (name, k, kind, at)


def test_slot_binding_table_matches_its_header():
    import policy_slots_abi

    decl = declarations(SLOTS_HEADER)
    assert sorted(decl) == named_functions(SLOTS_HEADER)  # the parser saw every declaration
    assert sorted(decl) == ["mpenv_policy_forward_slot", "mpenv_policy_load_slot", "mpenv_policy_slots",
                            "mpenv_policy_unload_slot"]
    check_table(policy_slots_abi.SIGNATURES, decl)
    m = re.search(r"^#define\s+MPENV_POLICY_SLOTS\s+(\d+)\s*$", header_text(SLOTS_HEADER), flags=re.M)
    assert m and int(m.group(1)) == policy_slots_abi.POLICY_SLOTS == 32


def test_main_header_includes_the_slot_header_and_declares_what_mpenv_abi_binds():
    import mpenv_abi
    import policy_slots_abi

    text = header_text(MAIN_HEADER)
    assert re.search(r'^#include\s+"mpenv_policy_slots\.h"\s*$', text, flags=re.M)
    decl = declarations(MAIN_HEADER)
    assert sorted(decl) == named_functions(MAIN_HEADER)
    check_table(mpenv_abi.SIGNATURES, decl)
    assert not set(decl) & set(policy_slots_abi.SIGNATURES)


def test_library_exports_every_slot_function():
    import policy_slots_abi

    lib = policy_slots_abi.bind(T.lib_mpenv())
    out = subprocess.run(["nm", "-D", "--defined-only", T.build_native.LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (mpenv_\w+)", out))
    for f in named_functions(SLOTS_HEADER):
        assert hasattr(lib, f) and f in exported, f


def test_slot_calls_refuse_a_null_manager_without_a_gpu():
    import policy_slots_abi

    lib = policy_slots_abi.bind(T.lib_mpenv())
    mask = C.c_uint32(7)
    assert lib.mpenv_policy_load_slot(None, 0, b"/nowhere") == -1
    assert lib.mpenv_policy_unload_slot(None, 0) == -1
    assert lib.mpenv_policy_slots(None, C.byref(mask)) == -1
    assert lib.mpenv_policy_forward_slot(None, 0, None, None, None) == -1
    assert "null" in lib.mpenv_last_error().decode()


def test_one_header_serves_a_c_and_a_cpp_caller(tmp_path):
    """Users include mpenv.h alone, from C and from C++, and get the slot calls."""
    src = ('#include "mpenv.h"\n'
           "int main(void) { uint32_t m = 0; return mpenv_policy_slots(0, &m) == MPENV_ERR_INVALID && "
           "MPENV_POLICY_SLOTS == 32 ? 0 : 1; }\n")
    for ext, cc in ((".c", "gcc"), (".cpp", "g++")):
        f = tmp_path / ("caller" + ext)
        f.write_text(src)
        exe = str(tmp_path / ("caller_" + cc))
        subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, str(f), "-o", exe, "-L", T.PKG, "-lmpenv",
                        f"-Wl,-rpath,{T.PKG}"], check=True)
        assert subprocess.run([exe]).returncode == 0
