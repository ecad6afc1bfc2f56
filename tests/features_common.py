"""g++ build of tests/cpu_harness/lg_features_harness.cpp: lg_feature_step of the product's lg_math.h over whole images (test infrastructure)."""
import ctypes as C
import os
import subprocess

import numpy as np

import common

_HARNESS = None


def harness():
    global _HARNESS
    if _HARNESS is not None:
        return _HARNESS
    d = os.path.join(common.ROOT, "tests", "cpu_harness")
    so = os.path.join(d, "liblg_features_harness.so")
    srcs = [os.path.join(d, "lg_features_harness.cpp"), os.path.join(common.ROOT, "lightgaussian_amd", "csrc", "lg_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2",
                               srcs[0], "-o", so])
    lib = C.CDLL(so)
    P = C.c_void_p
    lib.h_feature_step.restype = C.c_int
    lib.h_feature_step.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.h_blend_features.restype = C.c_longlong
    lib.h_blend_features.argtypes = [C.c_int] * 4 + [P] * 6 + [C.c_float, C.c_float] + [P] * 7
    _HARNESS = lib
    return lib


def blend_features(kw, features, bg=None, dL_dout=None):
    """kw: common.scene_kwargs(...) (numpy, scales / rotations); features [N, C].  Returns (out [C,H,W], alpha [H,W], radii, instances),
    and with dL_dout [C,H,W] also dF [N, C] = sum over pixels of w dL_dout in float64."""
    lib = harness()
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    means3D = f32(kw["means3D"]); N = means3D.shape[0]
    feats = f32(features); Cn = feats.shape[1]
    W, H = kw["W"], kw["H"]
    op = f32(kw["opacities"]).reshape(-1); sc = f32(kw["scales"]); rot = f32(kw["rotations"])
    vm = f32(kw["viewmatrix"]); pm = f32(kw["projmatrix"])
    bgc = None if bg is None else f32(bg)
    out = np.zeros((Cn, H, W), np.float32); alpha = np.zeros((H, W), np.float32); radii = np.zeros(N, np.int32)
    g = None if dL_dout is None else f32(dL_dout)
    dF = None if g is None else np.zeros((N, Cn), np.float64)
    n = lib.h_blend_features(N, Cn, W, H, p(means3D), p(op), p(sc), p(rot), p(vm), p(pm), float(kw["tanfovx"]), float(kw["tanfovy"]),
                             p(feats), p(bgc), p(out), p(alpha), p(radii), p(g), p(dF))
    if g is not None:
        return out, alpha, radii, int(n), dF
    return out, alpha, radii, int(n)
