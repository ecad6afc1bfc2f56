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

import numpy as np
import torch

import camera_grad_common as cg
import common
import dense_twin
import tolerance
from common import ptr, syn  # noqa: F401  (the tests of this feature take ptr from here)
from tolerance import TOL, rel_err  # noqa: F401

SCENES = ("a", "b", "c", "d")


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("absgrad", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_abs_pair": (None, [I] + [P] * 7), "h_abs_pair_sum": (None, [I, P, P, P, F, F, F, P]),
        "h_abs_rows_to_grad": (None, [I, P, P, P, I, I, P]), "h_pair_signed": (None, [I] + [P] * 8)})


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
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
        g = common.append_view_space(g, cam, (((0.1, 0.1, -3.0), (math.log(0.05),) * 3, 2.0),           # behind the camera
                                              ((3.0 * tanx * 4.0, 0.0, 4.0), (math.log(0.02),) * 3, 2.0)))  # off screen: three half-widths to the right
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
        g = common.append_view_space(g, cam, (((0.0, 0.0, 4.5), (math.log(2.0),) * 3, 0.0),))     # sigma ~ 43 pixels: every tile of the image
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
_REF = {}


def abs_reference(name, antialias=False):
    """{"float64": {"absgrad": [N,2], "grad": [N,2]}, "float32": {...}} (numpy float64) of the scene's loss by the dense twin: per pixel
    with a non-zero gimg one autograd.grad(s_p, means2D); absgrad = sum_p |.|, grad = sum_p (.) (the signed gradient, for the
    tests' own sanity).  antialias: the twin of antialias_common (opacities = sigma rho).  Computed once per (name, antialias)."""
    key = (name, bool(antialias))
    if key in _REF:
        return _REF[key]
    kw, _opts, gimg = scene_kwargs(name)
    pix = torch.nonzero(gimg.abs().sum(0).reshape(-1) > 0).reshape(-1).tolist()
    out = {}
    for dd, dname in dense_twin.DTYPES:
        m2 = torch.zeros(kw["means3D"].shape[0], 3, dtype=dd, requires_grad=True)
        s = (dense_twin.render(kw, dd, means2D=m2, antialias=antialias)[0] * gimg.to(dd)).sum(0).reshape(-1)
        a, sg = torch.zeros(m2.shape[0], 2, dtype=torch.float64), torch.zeros(m2.shape[0], 2, dtype=torch.float64)
        for p in pix:
            gp, = torch.autograd.grad(s[p], m2, retain_graph=True)
            a += gp[:, :2].abs().double()
            sg += gp[:, :2].double()
        out[dname] = {"absgrad": a.numpy(), "grad": sg.numpy()}
    _REF[key] = out
    return out


def assert_rule(got, ref, what=""):
    """got [N,3] (or [N,2]) against ref = abs_reference(...)."""
    tolerance.assert_rule3(np.asarray(got)[:, :2], ref["float64"]["absgrad"], ref["float32"]["absgrad"], f"{what} absgrad")


# ---- GPU runs (tests/test_gpu_absgrad.py, tools) ------------------------------------------------------------------------------------
DEV = "cuda:0"
RAW = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")


def run_activated(name, options, camera_grad=False, backwards=1):
    """gpu_common.run_rasterizer on the scene, its own rasterizer options underneath `options`."""
    import gpu_common
    kw, opts, gimg = scene_kwargs(name)
    return gpu_common.run_rasterizer(kw, gimg, dict(opts, **options), camera_grad=camera_grad, backwards=backwards)


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
