"""g++ build of tests/cpu_harness/lg_scoremax_harness.cpp: the per-hit significance weights of the product's lg_math.h, reduced by a maximum
and by the Q24.40 sum, over whole views (test infrastructure).  The reference of score_reduce="max" -- the oracle has no maximum;
tests/test_scoremax_host.py ties the harness to the oracle through the sums."""
import ctypes as C
import math

import numpy as np

import common
from common import f32, ptr, syn

POLICIES = ("alpha", "alpha_t")
THRESHOLD = 0.01        # RadSplat's pruning threshold: every scene of the tests has Gaussians on both sides of it


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("scoremax", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_fix40_to_score": (F, [C.c_uint64]),
        "h_score_max": (C.c_longlong, [I] * 4 + [P] * 6 + [F, F] + [P] * 6)})


def score_max(kw, antialias=False):
    """kw: common.scene_kwargs(...) (numpy or CPU tensors; scales / rotations).  Returns a dict of per-Gaussian arrays: count (int32),
    max {policy: float32}, sum {policy: uint64 Q24.40}, score_sum {policy: float32 = lg_fix40_score(sum)}, radii, and `instances`."""
    lib = harness()
    means3D = f32(kw["means3D"]); N = means3D.shape[0]
    W, H = int(kw["W"]), int(kw["H"])
    op = f32(kw["opacities"]).reshape(-1); sc = f32(kw["scales"]); rot = f32(kw["rotations"])
    vm = f32(kw["viewmatrix"]); pm = f32(kw["projmatrix"])
    count = np.zeros(N, np.int32); radii = np.zeros(N, np.int32)
    mx = {p: np.zeros(N, np.float32) for p in POLICIES}
    sm = {p: np.zeros(N, np.uint64) for p in POLICIES}
    n = lib.h_score_max(N, W, H, int(bool(antialias)), ptr(means3D), ptr(op), ptr(sc), ptr(rot), ptr(vm), ptr(pm), float(kw["tanfovx"]),
                        float(kw["tanfovy"]), ptr(count), ptr(mx["alpha"]), ptr(mx["alpha_t"]), ptr(sm["alpha"]), ptr(sm["alpha_t"]), ptr(radii))
    score_sum = {p: np.array([lib.h_fix40_to_score(int(q)) for q in sm[p]], np.float32).reshape(N) for p in POLICIES}
    return dict(count=count, max=mx, sum=sm, score_sum=score_sum, radii=radii, instances=int(n))


# ---- the scenes of tests/test_scoremax_host.py and tests/test_gpu_score_max.py ---------------------------------------------------
def _parity_case(k):
    from test_gpu_parity import CASES, _scene
    return _scene(CASES[k])


def _small_partial_tile():
    # (faint splats: some never reach alpha >= 1/255 on the 13 x 9 pixels, some stay below the threshold)
    g = syn.make_gaussians(64, seed=11, log_scale_mean=math.log(0.1), opacity_mean=-3.0, extent=(0.6, 0.4, 0.6))
    return common.scene_kwargs(g, syn.orbit_camera(0, 4, 13, 9, radius=3.0), 13, 9, deg=1, as_torch=True)


def _long_lists():
    """The scene of tests/test_gpu_weight_policies.py's long-list test: lists of several hundred entries with saturating pixels."""
    g = syn.make_gaussians(6000, seed=21, log_scale_mean=math.log(0.08), opacity_mean=1.5, extent=(1.0, 0.6, 1.0), log_scale_std=0.7)
    return common.scene_kwargs(g, syn.orbit_camera(2, 9, 208, 144, radius=4.0), 208, 144, deg=1, bg=(0.0, 0.0, 0.0), as_torch=True)


SCENES = {"saturating": lambda: _parity_case(1), "early_stop": lambda: _parity_case(2), "ragged": lambda: _parity_case(3),
          "screen_filling": lambda: _parity_case(6), "partial_tile": _small_partial_tile, "long_lists": _long_lists}
_CACHE = {}


def scene(name, antialias=False):
    """(kw as CPU tensors, the harness's result for it), computed once per process and never modified."""
    key = (name, bool(antialias))
    if key not in _CACHE:
        kw = SCENES[name]()
        ref = score_max(kw, antialias)
        for a in [ref["count"], ref["radii"], *ref["max"].values(), *ref["sum"].values(), *ref["score_sum"].values()]:
            a.setflags(write=False)
        _CACHE[key] = (kw, ref)
    return _CACHE[key]


# the 9-view scene of the sharded per-hit test (tests/test_gpu_weight_policies.py)
SHARD_N, SHARD_W, SHARD_H, SHARD_V = 4000, 160, 96, 9


def shard_scene():
    g = syn.make_gaussians(SHARD_N, seed=13, log_scale_mean=math.log(0.04), opacity_mean=0.5, extent=(2, 1.2, 2))
    cams = [syn.orbit_camera(k, SHARD_V, SHARD_W, SHARD_H, radius=5.0) for k in range(SHARD_V)]
    return g, cams
