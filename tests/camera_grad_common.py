"""Shared by tests/test_camera_host.py and tests/test_gpu_camera.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_camera_harness.cpp, the scenes, the dense-twin reference of the camera gradients and the tolerance rule.

Reference: oracle/torch_dense.py::render_dense differentiated with respect to viewmatrix, projmatrix and campos (they enter through
plain torch ops), in float64 (d64) and in float32 (d32), with the same image gradient.  Rule 3 of the project, per output tensor in
the max norm:   rel_err(g, d64) <= max(1e-4, 3 rel_err(d32, d64)).

The rule itself is tests/tolerance.py's, the twin's call and its keep mask tests/dense_twin.py's; every reference is computed once per
key and shared."""
import ctypes as C
import math

import numpy as np
import torch

import common
import dense_twin
import tolerance
from common import syn
from tolerance import TOL, rel_err  # noqa: F401  (the modules built on this one take them from here)

BG = (0.1, 0.2, 0.3)
NAMES = dense_twin.CAMERA


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("camera", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_camera_terms": (I, [I] * 4 + [P] * 9 + [F, F] + [P] * 3)})


def unpack(sums27):
    """The packed 27 sums (LG_CAM_TERMS: vm columns 0..2, pm columns 0, 1, 3, campos) -> ([4,4], [4,4], [3]) float64."""
    s = np.asarray(sums27, np.float64)
    vm, pm = np.zeros((4, 4)), np.zeros((4, 4))
    vm[:, :3] = s[:12].reshape(4, 3)
    pm[:, [0, 1, 3]] = s[12:24].reshape(4, 3)
    return vm, pm, s[24:27].copy()


def assert_rule3(got, ref, what=""):
    """got: {name: array}; ref: {"float64": {...}, "float32": {...}}.  Rule 3 per camera tensor; with colours as inputs the camera centre
    takes no part in the render (autograd hands the twin no gradient at all): exact zeros are asked for then."""
    for n in NAMES:
        tolerance.assert_rule3(got[n], ref["float64"][n], ref["float32"][n], f"{what} d/d{n}", zero_means_zero=(n == "campos"))


def assert_unused_columns_zero(got, what=""):
    vm, pm = np.asarray(got["viewmatrix"]).reshape(4, 4), np.asarray(got["projmatrix"]).reshape(4, 4)
    assert not vm[:, 3].any() and not pm[:, 2].any(), f"{what}: column 3 of d/dviewmatrix and column 2 of d/dprojmatrix must be exact zeros"


# ---- scenes --------------------------------------------------------------------------------------------------------------
def small_scene(name):
    """"N300_70x45": the issue's scene (300 Gaussians, look_at_camera((2.5, -1, -4), (0.1, 0, 0), roll 20), scale mean log 0.05);
    "N64_33x17": 64 Gaussians at 33 x 17 under the same camera.  Returns (gaussians, camera, W, H)."""
    N, W, H = {"N300_70x45": (300, 70, 45), "N64_33x17": (64, 33, 17)}[name]
    g = syn.make_gaussians(N, seed=3, extent=(1.5, 1.0, 1.5), log_scale_mean=math.log(0.05), opacity_mean=0.0)
    cam = syn.look_at_camera((2.5, -1.0, -4.0), (0.1, 0.0, 0.0), W, H, roll_deg=20.0)
    return g, cam, W, H


COMBOS = ("sh3", "sh1", "precolor", "precov")


def combo_kwargs(g, cam, W, H, combo, n=None):
    """scene_kwargs (CPU torch tensors) of one input combination: SH degree 3, SH degree 1, colors_precomp, or cov3D_precomp (with SH
    degree 3).  n: use only the first n Gaussians."""
    N = g.num
    pre = torch.rand(N, 3, generator=torch.Generator().manual_seed(7)) if combo == "precolor" else None
    kw = common.scene_kwargs(g, cam, W, H, deg=1 if combo == "sh1" else 3, precolor=pre, precov=(combo == "precov"), bg=BG, as_torch=True)
    kw = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
    if n is not None:
        for k in dense_twin.PER_GAUSSIAN:
            if k in kw:
                kw[k] = kw[k][:n].contiguous()
    return kw


def image_gradient(H, W, seed=0):
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed))


def dense_render(kw, dd, camera=None):
    """The twin's [3,H,W] image of kw in dtype dd.  camera: (vm, pm, campos) tensors to use instead of kw's (already of dtype dd, possibly
    requiring grad)."""
    return dense_twin.render(kw, dd, camera=camera)[0]


def dense_camera_reference(key, kw, gimg):
    """{"float64": {viewmatrix, projmatrix, campos}, "float32": {...}} (numpy float64 arrays) of sum(image * gimg) by the dense twin."""
    return dense_twin.gradients(key, kw, gimg, camera=True, per_gaussian=False)
