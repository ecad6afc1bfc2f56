"""Shared by tests/test_adam_rows_host.py and __graft_entry__.build() (test infrastructure): the g++ build of the CPU harness around
the row-index helpers of lg_adam_rows_kernel (lightgaussian_amd/csrc/lg_adam_rows.h)."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
_HARNESS = {}


def harness():
    """g++ build of tests/cpu_harness/lg_adam_rows_harness.cpp (the product's lg_adam_rows.h compiled for the CPU)."""
    if "lib" not in _HARNESS:
        d = os.path.join(HERE, "cpu_harness")
        root = os.path.dirname(HERE)
        so = os.path.join(d, "liblg_adam_rows_harness.so")
        srcs = [os.path.join(d, "lg_adam_rows_harness.cpp"), os.path.join(root, "lightgaussian_amd", "csrc", "lg_adam_rows.h"),
                os.path.join(root, "include", "lightgaussian.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", srcs[0], "-o", so])
        lib = C.CDLL(so)
        lib.h_adam_span.restype = C.c_int
        lib.h_adam_span.argtypes = []
        lib.h_adam_local_rows.restype = C.c_int64
        lib.h_adam_local_rows.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.h_adam_first_row.restype = C.c_int64
        lib.h_adam_first_row.argtypes = [C.c_int64, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.h_adam_row_of.restype = C.c_int64
        lib.h_adam_row_of.argtypes = [C.c_int64, C.c_uint32, C.c_uint32]
        _HARNESS["lib"] = lib
    return _HARNESS["lib"]
