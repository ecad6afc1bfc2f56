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
import os
import subprocess

import numpy as np
import torch

import camera_grad_common as cg
import common
from common import syn
from oracle import torch_dense

FLOOR = 0.000025
TOL = cg.TOL
rel_err = cg.rel_err

_HARNESS = None


def harness():
    global _HARNESS
    if _HARNESS is not None:
        return _HARNESS
    d = os.path.join(common.ROOT, "tests", "cpu_harness")
    so = os.path.join(d, "liblg_antialias_harness.so")
    srcs = [os.path.join(d, "lg_antialias_harness.cpp"), os.path.join(common.ROOT, "lightgaussian_amd", "csrc", "lg_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2",
                               srcs[0], "-o", so])
    lib = C.CDLL(so)
    P, F, I = C.c_void_p, C.c_float, C.c_int
    lib.h_aa_rho.restype = None
    lib.h_aa_rho.argtypes = [I, P, P, P, P]
    lib.h_aa_rho_scene.restype = None
    lib.h_aa_rho_scene.argtypes = [I, I, I, I, P, P, P, P, P, F, F, P]
    lib.h_aa_project.restype = None
    lib.h_aa_project.argtypes = [I, I, I, I, P, P, P, P, P, P, F, F, P]
    lib.h_aa_backward.restype = None
    lib.h_aa_backward.argtypes = [I, I, I, I, I] + [P] * 8 + [F, F] + [P] * 6
    lib.h_aa_camera_terms.restype = None
    lib.h_aa_camera_terms.argtypes = [I, I, I, I] + [P] * 7 + [F, F, P]
    _HARNESS = lib
    return lib


def f32(t):
    return None if t is None else np.ascontiguousarray(t.detach().numpy() if torch.is_tensor(t) else t, np.float32)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


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
    vm = cam.world_view_transform.double()
    inv = torch.linalg.inv(vm)
    tanx = math.tan(cam.FoVx * 0.5)
    xyz, sc, op = [], [], []
    for pos, ls, logit in _EXTRA:
        if pos is None:
            pos = (1.45 * tanx * 4.0, 0.0, 4.0)
        xyz.append((torch.tensor(pos + (1.0,), dtype=torch.float64) @ inv)[:3].float())
        sc.append(torch.tensor(ls)); op.append(torch.tensor([logit]))
    n = len(_EXTRA)
    gen = torch.Generator().manual_seed(5)
    cat = lambda a, b: torch.cat([a.detach(), b.to(a.dtype)], 0)  # noqa: E731
    g2 = syn.SyntheticGaussians(cat(g._xyz, torch.stack(xyz)), cat(g._features_dc, g._features_dc[:n]), cat(g._features_rest, g._features_rest[:n]),
                                cat(g._scaling, torch.stack(sc)), cat(g._rotation, torch.randn(n, 4, generator=gen)),
                                cat(g._opacity, torch.stack(op)), g.max_sh_degree, g.active_sh_degree)
    return g2, cam, W, H


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
_GEOM = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


def twin_leaves(kw, dd, grad=True):
    return {k: kw[k].to(dd).detach().clone().requires_grad_(grad) for k in _GEOM if k in kw}


def twin_kwargs(kw, leaves, dd, camera=None, antialias=True):
    """kw with the leaves in place of its per-Gaussian tensors and opacities = sigma rho (rho from the leaves and the camera)."""
    vm = camera[0] if camera is not None else kw["viewmatrix"].to(dd)
    out = dict(kw)
    out.update(leaves)
    if antialias:
        out["opacities"] = leaves["opacities"] * rho_torch(leaves, vm, kw["W"], kw["H"], kw["tanfovx"], kw["tanfovy"])[:, None]
    return out


def dense_image(kw, dd, antialias=True):
    """(image [3,H,W], count [N] over the Gaussians cg.dense_render keeps, rho [N]) of the twin in dtype dd, no gradients."""
    with torch.no_grad():
        leaves = twin_leaves(kw, dd, grad=False)
        k2 = twin_kwargs(kw, leaves, dd, antialias=antialias)
        vm32 = kw["viewmatrix"].float()
        keep = (kw["means3D"].float() @ vm32[:3, 2] + vm32[3, 2]) > 0.19
        t = {k: k2[k][keep] for k in _GEOM if k in k2}
        color, _radii, cnt = torch_dense.render_dense(means2D=torch.zeros(int(keep.sum()), 3, dtype=dd), W=kw["W"], H=kw["H"], tanfovx=kw["tanfovx"],
                                                      tanfovy=kw["tanfovy"], bg=kw["bg"].to(dd), viewmatrix=kw["viewmatrix"].to(dd),
                                                      projmatrix=kw["projmatrix"].to(dd), campos=kw["campos"].to(dd), sh_degree=kw["sh_degree"], **t)
        count = torch.zeros(kw["means3D"].shape[0], dtype=torch.int64)
        count[keep] = cnt
        rho = rho_torch(leaves, kw["viewmatrix"].to(dd), kw["W"], kw["H"], kw["tanfovx"], kw["tanfovy"])
    return color, count, rho


_REF = {}


def dense_reference(key, kw, gimg, camera=False):
    """{"float64": {tensor name: gradient}, "float32": {...}} of sum(image * gimg) by the antialiased twin, with respect to the
    per-Gaussian inputs of kw (and, camera=True, to viewmatrix / projmatrix / campos).  Computed once per key."""
    if key in _REF:
        return _REF[key]
    out = {}
    for dd in (torch.float64, torch.float32):
        leaves = twin_leaves(kw, dd)
        cam = tuple(kw[n].to(dd).detach().clone().requires_grad_() for n in cg.NAMES) if camera else None
        (cg.dense_render(twin_kwargs(kw, leaves, dd, cam), dd, cam) * gimg.to(dd)).sum().backward()
        g = {k: v.grad.numpy().astype(np.float64) for k, v in leaves.items()}
        if camera:
            g.update({n: (np.zeros(tuple(c.shape)) if c.grad is None else c.grad.numpy().astype(np.float64)) for n, c in zip(cg.NAMES, cam)})
        out["float64" if dd == torch.float64 else "float32"] = g
    _REF[key] = out
    return out


def assert_rule(got, ref, names, what=""):
    """The rule of camera_grad_common, per tensor; every figure is printed before it is asserted."""
    for n in names:
        r64, r32 = ref["float64"][n], ref["float32"][n]
        g = np.asarray(got[n], np.float64).reshape(r64.shape)
        floor, err = rel_err(r32, r64), rel_err(g, r64)
        print(f"{what} d/d{n}: rel_err {err:.3e} (float32 twin {floor:.3e}, max |d64| {np.abs(r64).max():.3e})")
        assert np.isfinite(g).all(), f"{what} {n}: not finite"
        assert np.abs(r64).max() > 0, f"{what} {n}: the reference is zero"
        assert err <= max(TOL, 3.0 * floor), f"{what} d/d{n}: rel err {err:.3e} (float32 twin floor {floor:.3e})"


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
