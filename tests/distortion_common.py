"""Shared by tests/test_distortion_host.py and tests/test_gpu_distortion.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_distortion_harness.cpp, float64 references of one ray, and the rays of the thin-slab accuracy check."""
import ctypes as C

import numpy as np

import common
from common import f32, ptr

SLAB_SEEDS, SLAB_HITS, SLAB_HALF = 200, 20, 0.02


def harness():
    P, F, I, U = C.c_void_p, C.c_float, C.c_int, C.c_uint32
    return common.build_harness("distortion", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_distortion_step": (None, [F, F, F, U, P, P]),
        "h_distortion_ray": (I, [I, P, P, F, F, P, P, P, P, P]),
        "h_distortion_view": (C.c_longlong, [I] * 3 + [P] * 6 + [F, F, P, I] + [P] * 12)})


def ray(alpha, m, gD=1.0, gM=0.0):
    """The harness's walk of one ray: dict(D, median, T, med_pos, w [n], dalpha [n], dm [n], n)."""
    alpha, m = f32(alpha), f32(m)
    n = alpha.shape[0]
    out = np.zeros(3, np.float32); pos = np.zeros(1, np.uint32)
    w, da, dm = (np.zeros(n, np.float32) for _ in range(3))
    cnt = harness().h_distortion_ray(n, ptr(alpha), ptr(m), float(gD), float(gM), ptr(out), ptr(pos), ptr(w), ptr(da), ptr(dm))
    return dict(D=float(out[0]), median=float(out[1]), T=float(out[2]), med_pos=int(pos[0]), w=w, dalpha=da, dm=dm, n=cnt)


def ray64(alpha, m):
    """float64 on the same float32 inputs: (D by the pairwise definition, median, 0-based index of the median entry or -1, w [n],
    number of contributors).  The decisions are the contract's: alpha >= 1/255, T (1 - alpha) >= 1e-4 or the ray ends, Tin > 0.5."""
    alpha, m = np.asarray(f32(alpha), np.float64), np.asarray(f32(m), np.float64)
    T, w, sel = 1.0, np.zeros(len(alpha)), -1
    for k, a in enumerate(alpha):
        if a < 1.0 / 255.0:
            continue
        if T * (1.0 - a) < 1e-4:
            break
        if T > 0.5:
            sel = k
        w[k] = a * T
        T *= 1.0 - a
    d = m[:, None] - m[None, :]
    D = float((np.triu(w[:, None] * w[None, :], 1) * d * d).sum())
    return D, (float(m[sel]) if sel >= 0 else 0.0), sel, w, int((w > 0).sum())


def shifted32(w, m):
    """An independent float32 evaluation of the shifted recurrence (numpy scalars, one rounding per operation): the float32 floor."""
    w, m = f32(w), f32(m)
    one = np.float32
    A = P1 = P2 = D = one(0)
    c = None
    for wk, mk in zip(w, m):
        if wk == 0:
            continue
        if c is None:
            c = mk
        u = one(mk - c)
        uu = one(u * u)
        t = one(one(one(uu * A) + P2) - one(one(one(2) * u) * P1))
        D = one(D + one(wk * t))
        A = one(A + wk); P1 = one(P1 + one(wk * u)); P2 = one(P2 + one(wk * uu))
    return float(D)


def composed32(w, m):
    """A M2 - M1^2 with float32 running sums: what a feature blend of the columns [1, m, m m] gives."""
    w, m = f32(w), f32(m)
    one = np.float32
    A = M1 = M2 = one(0)
    for wk, mk in zip(w, m):
        A = one(A + wk); M1 = one(M1 + one(wk * mk)); M2 = one(M2 + one(wk * one(mk * mk)))
    return float(one(one(A * M2) - one(M1 * M1)))


def slab_ray(depth, seed):
    """(alpha [20], m [20]) float32: a thin slab at `depth` +- 0.02, every entry a contributor (alpha in [0.05, 0.3]: T stays above
    0.7^20 = 8e-4)."""
    rs = np.random.RandomState(1000 + seed)
    return rs.uniform(0.05, 0.3, SLAB_HITS).astype(np.float32), (depth + rs.uniform(-SLAB_HALF, SLAB_HALF, SLAB_HITS)).astype(np.float32)


def view(kw, m, gD=None, gM=None):
    """The harness's full-view walk.  kw: common.scene_kwargs(...) (numpy, scales / rotations); m [N] or a column view with its stride.
    Returns dict(D, median [H,W], radii, dm [N], means2D, means3D, opacities, scales, rotations, instances, longest, early, mid)."""
    means3D = f32(kw["means3D"]); N = means3D.shape[0]
    W, H = kw["W"], kw["H"]
    op = f32(kw["opacities"]).reshape(-1); sc = f32(kw["scales"]); rot = f32(kw["rotations"])
    vm = f32(kw["viewmatrix"]); pm = f32(kw["projmatrix"])
    m = f32(m).reshape(-1)
    gD, gM = f32(gD), f32(gM)
    o = dict(D=np.zeros((H, W), np.float32), median=np.zeros((H, W), np.float32), radii=np.zeros(N, np.int32), dm=np.zeros(N, np.float32),
             means2D=np.zeros((N, 3), np.float32), means3D=np.zeros((N, 3), np.float32), opacities=np.zeros((N, 1), np.float32),
             scales=np.zeros((N, 3), np.float32), rotations=np.zeros((N, 4), np.float32))
    info = np.zeros(3, np.int64)
    o["instances"] = int(harness().h_distortion_view(
        N, W, H, ptr(means3D), ptr(op), ptr(sc), ptr(rot), ptr(vm), ptr(pm), float(kw["tanfovx"]), float(kw["tanfovy"]), ptr(m), 1, ptr(gD), ptr(gM),
        ptr(o["D"]), ptr(o["median"]), ptr(o["radii"]), ptr(o["dm"]), ptr(o["means2D"]), ptr(o["means3D"]), ptr(o["opacities"]), ptr(o["scales"]),
        ptr(o["rotations"]), ptr(info)))
    o["longest"], o["early"], o["mid"] = (int(x) for x in info)
    return o
