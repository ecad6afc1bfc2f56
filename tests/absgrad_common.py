"""Shared by tests/test_absgrad_host.py and tests/test_gpu_absgrad.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_absgrad_harness.cpp, the scenes, and the dense-twin reference of the absolute mean gradients.

Reference: oracle/torch_dense.py::render_dense in float64 (d64) and float32 (d32).  For the loss sum(gimg * image), per pixel p
    s_p = sum_c gimg[c, p] image[c, p],        absgrad = sum_p |d s_p / d means2D|
by one autograd.grad per pixel with a non-zero gimg (pixels where gimg is zero contribute exactly zero), which is why every scene's gimg
has at most ~600 non-zero pixels.  means2D enters render_dense additively in NDC: the units of the rasterizer's dL_dmeans2D.  Every
reference is computed once per key and shared.  The rule is tests/camera_grad_common.py's, in the max norm over [N, 2]:
    rel_err(got, d64) <= max(1e-4, 3 rel_err(d32, d64)).

Scenes (the smallest that reach each path of K7's ABS variants and of lg_absgrad_rows):
    a  64 Gaussians at 33 x 17                     partial tiles on both edges, N a multiple of 64; gimg on all 561 pixels
    b  300 + 2 Gaussians at 70 x 45                one behind the camera, one off screen, N no multiple of 64; gimg on every fifth pixel (630)
    c  200 Gaussians stacked over one 16 x 16 tile segment_length 64: a list of several batches and >= 3 segments, started from checkpoints
    d  24 Gaussians at 112 x 112 (7 x 7 tiles)     one Gaussian covering the whole image: 49 instances > LG_COOP_ROWS = 48, the cooperative
                                                   gather; gimg on 3 pixels of every tile (147)"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import torch

import antialias_common as aa
import camera_grad_common as cg
import common
from common import syn
from oracle import torch_dense

TOL = cg.TOL
rel_err = cg.rel_err
SCENES = ("a", "b", "c", "d")

_HARNESS = None


def harness():
    global _HARNESS
    if _HARNESS is not None:
        return _HARNESS
    d = os.path.join(common.ROOT, "tests", "cpu_harness")
    so = os.path.join(d, "liblg_absgrad_harness.so")
    srcs = [os.path.join(d, "lg_absgrad_harness.cpp"), os.path.join(common.ROOT, "lightgaussian_amd", "csrc", "lg_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2",
                               srcs[0], "-o", so])
    lib = C.CDLL(so)
    P, F, I = C.c_void_p, C.c_float, C.c_int
    lib.h_abs_pair.restype = None
    lib.h_abs_pair.argtypes = [I] + [P] * 7
    lib.h_abs_pair_sum.restype = None
    lib.h_abs_pair_sum.argtypes = [I, P, P, P, F, F, F, P]
    lib.h_abs_rows_to_grad.restype = None
    lib.h_abs_rows_to_grad.argtypes = [I, P, P, P, I, I, P]
    lib.h_pair_signed.restype = None
    lib.h_pair_signed.argtypes = [I] + [P] * 8
    _HARNESS = lib
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _append(g, cam, extra):
    """g with Gaussians appended that are placed in VIEW space, as antialias_common.small_scene does: (view position, log-scales, logit)."""
    inv = torch.linalg.inv(cam.world_view_transform.double())
    n = len(extra)
    xyz = torch.stack([(torch.tensor(tuple(pos) + (1.0,), dtype=torch.float64) @ inv)[:3].float() for pos, _ls, _lo in extra])
    sc = torch.tensor([ls for _p, ls, _lo in extra], dtype=torch.float32)
    op = torch.tensor([[lo] for _p, _ls, lo in extra], dtype=torch.float32)
    cat = lambda a, b: torch.cat([a.detach(), b.to(a.dtype)], 0)  # noqa: E731
    return syn.SyntheticGaussians(cat(g._xyz, xyz), cat(g._features_dc, g._features_dc[:n]), cat(g._features_rest, g._features_rest[:n]),
                                  cat(g._scaling, sc), cat(g._rotation, torch.randn(n, 4, generator=torch.Generator().manual_seed(5))),
                                  cat(g._opacity, op), g.max_sh_degree, g.active_sh_degree)


_SCENE = {}


def scene(name):
    """(gaussians, camera, W, H, rasterizer options of the scene, gimg [3,H,W]) -- built once per name."""
    if name in _SCENE:
        return _SCENE[name]
    opts = {}
    if name == "a":
        g, cam, W, H = cg.small_scene("N64_33x17")
        mask = torch.ones(H, W, dtype=torch.bool)
    elif name == "b":
        g, cam, W, H = cg.small_scene("N300_70x45")
        tanx = math.tan(cam.FoVx * 0.5)
        g = _append(g, cam, (((0.1, 0.1, -3.0), (math.log(0.05),) * 3, 2.0),                    # behind the camera
                             ((3.0 * tanx * 4.0, 0.0, 4.0), (math.log(0.02),) * 3, 2.0)))       # off screen: three half-widths to the right
        mask = (torch.arange(H * W) % 5 == 0).reshape(H, W)
    elif name == "c":
        W = H = 16
        g = syn.make_gaussians(200, seed=11, extent=(0.5, 0.5, 0.5), log_scale_mean=math.log(0.8), log_scale_std=0.2, opacity_mean=-3.5,
                               opacity_std=0.3)
        cam = syn.look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), W, H)
        opts = {"segment_length": 64}
        mask = torch.ones(H, W, dtype=torch.bool)
    elif name == "d":
        W = H = 112
        g = syn.make_gaussians(23, seed=13, extent=(1.5, 1.5, 1.0), log_scale_mean=math.log(0.08), opacity_mean=0.0)
        cam = syn.look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), W, H)
        g = _append(g, cam, (((0.0, 0.0, 4.5), (math.log(2.0),) * 3, 0.0),))                    # sigma ~ 43 pixels: every tile of the image
        gen = torch.Generator().manual_seed(17)
        mask = torch.zeros(H, W, dtype=torch.bool)
        for ty in range(7):
            for tx in range(7):
                for k in torch.randperm(256, generator=gen)[:3].tolist():
                    mask[ty * 16 + k // 16, tx * 16 + k % 16] = True
    else:
        raise KeyError(name)
    gimg = cg.image_gradient(H, W, seed=1) * mask[None].float()
    _SCENE[name] = (g, cam, W, H, opts, gimg)
    return _SCENE[name]


def scene_kwargs(name):
    """The activated rasterizer inputs of the scene (CPU torch tensors, SH degree 3) and its gimg."""
    g, cam, W, H, opts, gimg = scene(name)
    return cg.combo_kwargs(g, cam, W, H, "sh3"), opts, gimg


# ---- the dense twin ----------------------------------------------------------------------------------------------------------------
_PER_GAUSSIAN = ("means3D", "opacities", "shs", "scales", "rotations")
_REF = {}


def abs_reference(name, antialias=False):
    """{"float64": {"absgrad": [N,2], "grad": [N,2]}, "float32": {...}} (numpy float64) of the scene's loss by the dense twin: per pixel
    with a non-zero gimg one autograd.grad(s_p, means2D); absgrad = sum_p |.|, grad = sum_p (.) (the signed gradient, for the
    tests' own sanity).  antialias: the twin of antialias_common (opacities = sigma rho).  Computed once per (name, antialias)."""
    key = (name, bool(antialias))
    if key in _REF:
        return _REF[key]
    kw, _opts, gimg = scene_kwargs(name)
    N = kw["means3D"].shape[0]
    vm32 = kw["viewmatrix"].float()
    keep = (kw["means3D"].float() @ vm32[:3, 2] + vm32[3, 2]) > 0.19       # cg.dense_render's superset of what the near plane lets through
    pix = torch.nonzero(gimg.abs().sum(0).reshape(-1) > 0).reshape(-1).tolist()
    out = {}
    for dd in (torch.float64, torch.float32):
        with torch.no_grad():
            k2 = aa.twin_kwargs(kw, aa.twin_leaves(kw, dd, grad=False), dd, antialias=antialias)
        t = {k: k2[k][keep].to(dd) for k in _PER_GAUSSIAN}
        m2 = torch.zeros(int(keep.sum()), 3, dtype=dd, requires_grad=True)
        color, _radii, _cnt = torch_dense.render_dense(means2D=m2, W=kw["W"], H=kw["H"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"],
                                                       bg=kw["bg"].to(dd), viewmatrix=kw["viewmatrix"].to(dd), projmatrix=kw["projmatrix"].to(dd),
                                                       campos=kw["campos"].to(dd), sh_degree=kw["sh_degree"], **t)
        s = (color * gimg.to(dd)).sum(0).reshape(-1)
        a = torch.zeros(m2.shape[0], 2, dtype=torch.float64)
        sg = torch.zeros(m2.shape[0], 2, dtype=torch.float64)
        for p in pix:
            gp, = torch.autograd.grad(s[p], m2, retain_graph=True)
            a += gp[:, :2].abs().double()
            sg += gp[:, :2].double()
        full_a, full_s = np.zeros((N, 2)), np.zeros((N, 2))
        full_a[keep.numpy()] = a.numpy()
        full_s[keep.numpy()] = sg.numpy()
        out["float64" if dd == torch.float64 else "float32"] = {"absgrad": full_a, "grad": full_s}
    _REF[key] = out
    return out


def assert_rule(got, ref, what=""):
    """got [N,3] (or [N,2]) against ref = abs_reference(...); the figures are printed before they are asserted."""
    r64, r32 = ref["float64"]["absgrad"], ref["float32"]["absgrad"]
    g = np.asarray(got, np.float64)[:, :2]
    floor, err = rel_err(r32, r64), rel_err(g, r64)
    print(f"{what} absgrad: rel_err {err:.3e} (float32 twin {floor:.3e}, max |d64| {np.abs(r64).max():.3e})")
    assert np.isfinite(g).all(), f"{what}: not finite"
    assert np.abs(r64).max() > 0, f"{what}: the reference is zero"
    assert err <= max(TOL, 3.0 * floor), f"{what} absgrad: rel err {err:.3e} (float32 twin floor {floor:.3e})"


# ---- GPU runs (tests/test_gpu_absgrad.py, tools) ------------------------------------------------------------------------------------
DEV = "cuda:0"
PER_GAUSSIAN = ("means3D", "opacities", "shs", "scales", "rotations")
RAW = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")


def run_activated(name, options, camera_grad=False, backwards=1):
    """Forward + `backwards` backward passes of the scene's loss through GaussianRasterizer (activated inputs).  Returns a dict: image,
    radii, grads {name: tensor} (means2D among them), camera {name: array} or None, means2D (the leaf: .absgrad is read from it)."""
    from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    kw, opts, gimg = scene_kwargs(name)
    dev = torch.device(DEV)
    t = {k: (v.detach().to(dev).clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
    for n in PER_GAUSSIAN:
        t[n].requires_grad_(True)
    cam = {n: t[n].requires_grad_(camera_grad) for n in cg.NAMES}
    rs = GaussianRasterizationSettings(image_height=t["H"], image_width=t["W"], tanfovx=t["tanfovx"], tanfovy=t["tanfovy"], bg=t["bg"],
                                       scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], sh_degree=t["sh_degree"],
                                       campos=cam["campos"], prefiltered=False, debug=False, f_count=False)
    means2D = torch.zeros((t["means3D"].shape[0], 3), device=dev, requires_grad=True)
    color, radii = GaussianRasterizer(rs, options=dict(opts, **options, camera_grad=camera_grad))(
        means3D=t["means3D"], means2D=means2D, opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    loss = (color * gimg.to(dev)).sum()
    for k in range(backwards):
        loss.backward(retain_graph=k + 1 < backwards)
    torch.cuda.synchronize()
    grads = {n: t[n].grad for n in PER_GAUSSIAN}
    grads["means2D"] = means2D.grad
    camera = {n: cam[n].grad.detach().cpu().numpy().copy() for n in cg.NAMES} if camera_grad else None
    return dict(image=color.detach(), radii=radii, grads=grads, camera=camera, means2D=means2D)


def gpu_model(name):
    """The scene's Gaussians on the device as a model with the reference's getters and fresh raw leaves (the fused path of render())."""
    g = scene(name)[0]
    model = g.to(DEV)
    for n in RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    return model


def run_render(name, options, model=None):
    """Forward + backward of the scene's loss through gaussian_renderer.render (raw parameters, getters fused into the kernels).  Returns a
    dict: image, radii, grads {raw name: tensor, "means2D"}, means2D (= pkg["viewspace_points"]), pkg, model."""
    from lightgaussian_amd import gaussian_renderer
    _g, cam, _W, _H, opts, gimg = scene(name)
    model = model if model is not None else gpu_model(name)
    bg = torch.tensor(cg.BG, device=DEV)
    pkg = gaussian_renderer.render(cam.to(DEV), model, syn.PipelineParams(), bg, options=dict(opts, **options))
    assert "Raw" in type(pkg["render"].grad_fn).__name__           # the fused getters
    (pkg["render"] * gimg.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {n: getattr(model, n).grad for n in RAW}
    grads["means2D"] = pkg["viewspace_points"].grad
    return dict(image=pkg["render"].detach(), radii=pkg["radii"], grads=grads, means2D=pkg["viewspace_points"], pkg=pkg, model=model)
