"""g++ build of tests/cpu_harness/lg_features_harness.cpp: lg_feature_step of the product's lg_math.h over whole images (test infrastructure)."""
import ctypes as C

import numpy as np

import common
from common import f32, ptr


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("features", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_feature_step": (I, [F, F, C.POINTER(F), C.POINTER(F)]),
        "h_blend_features": (C.c_longlong, [I] * 4 + [P] * 6 + [F, F] + [P] * 7)})


def blend_features(kw, features, bg=None, dL_dout=None):
    """kw: common.scene_kwargs(...) (numpy, scales / rotations); features [N, C].  Returns (out [C,H,W], alpha [H,W], radii, instances),
    and with dL_dout [C,H,W] also dF [N, C] = sum over pixels of w dL_dout in float64."""
    lib = harness()
    means3D = f32(kw["means3D"]); N = means3D.shape[0]
    feats = f32(features); Cn = feats.shape[1]
    W, H = kw["W"], kw["H"]
    op = f32(kw["opacities"]).reshape(-1); sc = f32(kw["scales"]); rot = f32(kw["rotations"])
    vm = f32(kw["viewmatrix"]); pm = f32(kw["projmatrix"])
    bgc = f32(bg)
    out = np.zeros((Cn, H, W), np.float32); alpha = np.zeros((H, W), np.float32); radii = np.zeros(N, np.int32)
    g = f32(dL_dout)
    dF = None if g is None else np.zeros((N, Cn), np.float64)
    n = lib.h_blend_features(N, Cn, W, H, ptr(means3D), ptr(op), ptr(sc), ptr(rot), ptr(vm), ptr(pm), float(kw["tanfovx"]), float(kw["tanfovy"]),
                             ptr(feats), ptr(bgc), ptr(out), ptr(alpha), ptr(radii), ptr(g), ptr(dF))
    if g is not None:
        return out, alpha, radii, int(n), dF
    return out, alpha, radii, int(n)
