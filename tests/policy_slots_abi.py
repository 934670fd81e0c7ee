"""The ctypes binding of include/mpenv_policy_slots.h (the per-slot policy
calls that mpenv.h includes): SIGNATURES, {function: (restype, [argtypes])},
for every function that header declares, by the rules of mpenv_abi.py -- one
type per parameter kind: c_void_p for the manager handle, streams and device
pointers, POINTER(c_xxx) for host out-parameters passed with byref, c_char_p
for host strings.  tests/test_policy_slots.py pins the table to the header.
Imports nothing but ctypes."""
import ctypes as C

vp, cstr = C.c_void_p, C.c_char_p
i32, u32 = C.c_int32, C.c_uint32
P = C.POINTER

POLICY_SLOTS = 32  # MPENV_POLICY_SLOTS

SIGNATURES = {
    "mpenv_policy_load_slot": (i32, [vp, i32, cstr]),
    "mpenv_policy_unload_slot": (i32, [vp, i32]),
    "mpenv_policy_slots": (i32, [vp, P(u32)]),
    "mpenv_policy_forward_slot": (i32, [vp, i32, vp, vp, vp]),
}


def bind(lib):
    """Install every signature on a CDLL handle of the library; returns it."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib
