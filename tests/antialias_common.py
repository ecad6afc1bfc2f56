"""Shared by tests/test_antialias_host.py and tests/test_gpu_antialias.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_antialias_harness.cpp, the scenes, and the dense twin of the antialiased render.

The twin is oracle/torch_dense.py::render_dense called with opacities = sigma rho, rho recomputed in torch -- differentiably -- from
means3D, scales and rotations (or cov3D_precomp) and the view matrix, by render_dense's own projection lines and its detached clamp:
    rho = sqrt(clamp(det0 / det1, min=0.000025)),  det0 = a0 c0 - b b,  det1 = (a0 + 0.3)(c0 + 0.3) - b b.
Scenes and the tolerance rule are tests/camera_grad_common.py's, unchanged: per tensor in the max norm
    rel_err(got, d64) <= max(1e-4, 3 rel_err(d32, d64)).
"N300_70x45" gets six hand-placed Gaussians appended (EXTRA below); every reference is computed once per key and shared."""
import ctypes as C
import math

import numpy as np
import torch

import camera_grad_common as cg
import common
import dense_twin
import tolerance
from common import f32, ptr  # noqa: F401  (the tests of this feature take them from here)
from tolerance import TOL, rel_err  # noqa: F401

FLOOR = 0.000025


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("antialias", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_aa_rho": (None, [I, P, P, P, P]),
        "h_aa_rho_scene": (None, [I, I, I, I, P, P, P, P, P, F, F, P]),
        "h_aa_project": (None, [I, I, I, I, P, P, P, P, P, P, F, F, P]),
        "h_aa_backward": (None, [I, I, I, I, I] + [P] * 8 + [F, F] + [P] * 6),
        "h_aa_camera_terms": (None, [I, I, I, I] + [P] * 7 + [F, F, P])})


# ---- scenes ----------------------------------------------------------------------------------------------------------------
# Six Gaussians appended to "N300_70x45", placed in VIEW space (x, y right / down of the optical axis, z along it) and mapped to the world
# by the camera's own matrix:  (view position, log-scales, opacity logit)
#   0  log-scale -11 on all axes: det0 / det1 ~ 1e-7, rho sits at the floor
#   1  rank-one covariance (two axes at log-scale -40: exactly zero in float32 products): det0 <= 0 up to rounding
#   2  behind the camera
#   3  far off-axis: |x / z| > 1.3 tanfovx, the clamp of the EWA Jacobian is active (its rectangle still reaches the image)
#   4  sigma just above 1/255 with rho < 0.5: only the compensation removes it
#   5  ten times the mean size: rho > 0.99
_EXTRA = (((0.05, 0.02, 4.0), (-11.0, -11.0, -11.0), 2.0),
          ((-0.3, 0.1, 4.5), (math.log(0.05), -40.0, -40.0), 2.0),
          ((0.1, 0.1, -3.0), (math.log(0.05),) * 3, 2.0),
          (None, (math.log(0.6),) * 3, 2.0),
          ((0.2, -0.1, 4.2), (math.log(0.012),) * 3, math.log(0.0042 / (1 - 0.0042))),
          ((-0.2, 0.15, 5.0), (math.log(0.5),) * 3, 0.0))
N_EXTRA = len(_EXTRA)


def small_scene(name):
    """cg.small_scene(name); "N300_70x45" with the six hand-placed Gaussians appended (306 in all).  (gaussians, camera, W, H)"""
    g, cam, W, H = cg.small_scene(name)
    if name != "N300_70x45":
        return g, cam, W, H
    far_off_axis = (1.45 * math.tan(cam.FoVx * 0.5) * 4.0, 0.0, 4.0)
    return common.append_view_space(g, cam, [(pos or far_off_axis, ls, logit) for pos, ls, logit in _EXTRA]), cam, W, H


def combo_kwargs(name, combo):
    g, cam, W, H = small_scene(name)
    return cg.combo_kwargs(g, cam, W, H, combo)


# ---- rho in torch ----------------------------------------------------------------------------------------------------------
def cov2d(means3D, vm, W, H, tanfovx, tanfovy, scales=None, rotations=None, cov3D_precomp=None):
    """(a0, b, c0, tz): the 2D covariance before the blur, by render_dense's own lines (the clamp detached)."""
    dt = means3D.dtype
    N = means3D.shape[0]
    ph = torch.cat([means3D, torch.ones(N, 1, dtype=dt)], 1)
    pview = ph @ vm
    tz = pview[:, 2]
    if cov3D_precomp is None:
        r, x, y, z = rotations[:, 0], rotations[:, 1], rotations[:, 2], rotations[:, 3]
        Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                          2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                          2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(N, 3, 3)
        L = Rm * scales[:, None, :]
        Sig = L @ L.transpose(1, 2)
    else:
        c = cov3D_precomp
        Sig = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).view(N, 3, 3)
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = pview[:, 0] / tz, pview[:, 1] / tz
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz).detach(), pview[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz).detach(), pview[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], 1).view(N, 2, 3)
    T2 = J @ vm[:3, :3].t()
    cov = T2 @ Sig @ T2.transpose(1, 2)
    return cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1], tz


def rho_of(a0, b, c0):
    det0 = a0 * c0 - b * b
    det1 = (a0 + 0.3) * (c0 + 0.3) - b * b
    return torch.sqrt(torch.clamp(det0 / det1, min=FLOOR))


def rho_torch(t, vm, W, H, tanfovx, tanfovy):
    """rho [N] of the tensors t (means3D and scales + rotations or cov3D_precomp, of one dtype); 1 behind z_view = 0.19 (cg.dense_render
    drops those Gaussians)."""
    a0, b, c0, tz = cov2d(t["means3D"], vm, W, H, tanfovx, tanfovy, t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"))
    return torch.where(tz > 0.19, rho_of(a0, b, c0), torch.ones_like(tz))


def rho32_harness(kw, raw=False):
    """The float32 rho of every Gaussian of kw (scene kwargs, torch or numpy), by the harness -- K1's own operations."""
    lib = harness()
    m = f32(kw["means3D"])
    rho = np.ones(m.shape[0], np.float32)
    sc, rot, cov, vm = f32(kw.get("scales")), f32(kw.get("rotations")), f32(kw.get("cov3D_precomp")), f32(kw["viewmatrix"])
    lib.h_aa_rho_scene(m.shape[0], int(raw), kw["W"], kw["H"], ptr(m), ptr(sc), ptr(rot), ptr(cov), ptr(vm), float(kw["tanfovx"]),
                       float(kw["tanfovy"]), ptr(rho))
    return rho


# ---- the dense twin --------------------------------------------------------------------------------------------------------
def compensated_opacities(t, vm, kw):
    """sigma rho of the per-Gaussian tensors t (one dtype) under the view matrix vm: what dense_twin.render(antialias=True) renders."""
    return t["opacities"] * rho_torch(t, vm, kw["W"], kw["H"], kw["tanfovx"], kw["tanfovy"])[:, None]


def dense_image(kw, dd, antialias=True):
    """(image [3,H,W], count [N], rho [N]) of the twin in dtype dd, no gradients."""
    with torch.no_grad():
        color, _radii, count = dense_twin.render(kw, dd, antialias=antialias)
        rho = rho_torch(dense_twin.leaves(kw, dd, grad=False), kw["viewmatrix"].to(dd), kw["W"], kw["H"], kw["tanfovx"], kw["tanfovy"])
    return color, count, rho


def dense_reference(key, kw, gimg, camera=False):
    """{"float64": {tensor name: gradient}, "float32": {...}} of sum(image * gimg) by the antialiased twin, with respect to the
    per-Gaussian inputs of kw (and, camera=True, to viewmatrix / projmatrix / campos).  Computed once per key."""
    return dense_twin.gradients(key, kw, gimg, camera=camera, antialias=True)


def assert_rule(got, ref, names, what=""):
    """Rule 3 per tensor."""
    for n in names:
        tolerance.assert_rule3(got[n], ref["float64"][n], ref["float32"][n], f"{what} d/d{n}")


_CHECKED = []


def assert_scene_conditions():
    """What the issue asks of the float64 twin on "N300_70x45" (with the six extra Gaussians); checked once per process."""
    if _CHECKED:
        return _CHECKED[0]
    kw = combo_kwargs("N300_70x45", "sh3")
    _img_on, cnt_on, rho = dense_image(kw, torch.float64, True)
    _img_off, cnt_off, _ = dense_image(kw, torch.float64, False)
    sig = kw["opacities"].double().reshape(-1)
    front = (kw["means3D"].double() @ kw["viewmatrix"].double()[:3, 2] + kw["viewmatrix"].double()[3, 2]) > 0.2
    facts = dict(below_half=int(((rho < 0.5) & front).sum()), above_075=int(((rho > 0.75) & front).sum()),
                 at_floor=int(((rho == math.sqrt(FLOOR)) & front).sum()),
                 removed=int(((sig >= 1 / 255) & (sig * rho < 1 / 255) & front).sum()), hits_on=int(cnt_on.sum()), hits_off=int(cnt_off.sum()))
    print("N300_70x45 + 6:", facts)
    assert facts["below_half"] >= 100 and facts["above_075"] >= 25
    assert facts["at_floor"] >= 1 and facts["removed"] >= 1
    assert facts["hits_on"] < facts["hits_off"]
    _CHECKED.append(facts)
    return facts
