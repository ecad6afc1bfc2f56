"""Shared by tests/test_adam_rows_host.py and __graft_entry__.build() (test infrastructure): the g++ build of the CPU harness around
the row-index helpers of lg_adam_rows_kernel (lightgaussian_amd/csrc/lg_adam_rows.h)."""
import ctypes as C
import os

import common


def harness():
    """The product's lg_adam_rows.h compiled for the CPU."""
    I64, U32, U64 = C.c_int64, C.c_uint32, C.c_uint64
    return common.build_harness("adam_rows", headers=(os.path.join("lightgaussian_amd", "csrc", "lg_adam_rows.h"), common.LG_API_H),
                                flags=common.PLAIN, signatures={
        "h_adam_span": (C.c_int, []), "h_adam_local_rows": (I64, [U32, U64, U64, C.POINTER(U64)]),
        "h_adam_first_row": (I64, [I64, U32, C.POINTER(U32)]), "h_adam_row_of": (I64, [I64, U32, U32])})
