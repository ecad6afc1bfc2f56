"""Sensitivity pruning score (PUP 3D-GS): per Gaussian the log-determinant of its 6 x 6 block of the Gauss-Newton Hessian of the L2
reconstruction error, over the spatial parameters theta = (mean, scale), summed over the training views:

    H_i   = sum_views sum_pixels sum_channels (dI/dtheta_i)(dI/dtheta_i)^T
    score = log det H_i

    H = sensitivity_list(gaussians, scene_or_cameras, pipe, background)     # one forward + two launches per view
    s = score(H, gaussians, scale_space="log")                              # [N] float64; -inf: never seen, or not enough views
    prune.prune_gaussians(model, 0.9, s)                                    # -inf ranks first

A Hessian block needs the outer product of the per-pixel Jacobian -- render().backward() would have to run once per pixel and channel.
The kernels (csrc/lg_sensitivity.h) use that a pixel sees theta_i only through the Gaussian's 2D mean and conic: per (tile, Gaussian)
instance twelve pixel-offset moments are accumulated in one back-to-front walk of the lists the view's ordinary forward left, and one
lane per Gaussian turns them into A^T M A through the one copy of the backward chain.  No atomics: bit-identical run to run, and the
views add in float64.

The parameterisation is this project's reading of the paper: theta holds the ACTIVATED scales the rasterizer
receives and the colours are held constant (no view-direction term of the SH colours, no opacity or rotation column).  Every convention
of the backward applies: straight through the 0.99 clamp, pairs with alpha < 1/255 take no part, no gradient through the 1.3 tanfov
clamp.  scale_space="log" gives the block with respect to the raw log-scales, D H D with D = diag(1, 1, 1, s): the score gains
2 sum_k log s_k, applied at scoring time.

A model carrying `filter_3D` (filter3d.compute_filter_3d) is scored with respect to the FILTERED scales it is rendered with, and
scale_space="log" takes the logarithm of those: the score ranks what the renderer draws, not the raw parameters behind the filter
(options={"filter_3d": False} scores the unfiltered model)."""
import ctypes as C

import torch

from . import _lib
from . import filter3d as _filter3d
from . import rasterizer as _rasterizer
from .gaussian_renderer import _inputs, _pipe_options, _settings
from .rasterizer import _Call, _native_forward
from .vectree import CompressedGaussians, TrainableCompressed

H_WIDTH = 21        # LG_SENS_H: the upper triangle of a 6 x 6 block, row-major

# The C ABI of include/lightgaussian_sensitivity.h, in header order: name -> (restype, argtypes).  tests/test_sensitivity_host.py holds
# every entry against the header.
i32, i64, sz, vp = C.c_int32, C.c_int64, C.c_size_t, C.c_void_p
PROTOTYPES = {
    "lg_sensitivity_scratch_bytes": (sz, (i32, i64)),
    "lg_sensitivity_accumulate": (C.c_int, (vp, vp, vp, vp, vp, vp, i64, vp, vp, vp)),
    "lg_sensitivity_score": (C.c_int, (i32, vp, vp, vp, vp)),
}
def load():
    """The library object of _lib.load() with the prototypes of include/lightgaussian_sensitivity.h set on it."""
    return _lib.bind(_lib.load(), PROTOTYPES)


def _check_H(H, n, dev):
    if not (torch.is_tensor(H) and H.dtype == torch.float64 and tuple(H.shape) == (n, H_WIDTH) and H.is_contiguous() and H.device == dev):
        raise ValueError(f"H must be a contiguous float64 [{n}, {H_WIDTH}] tensor on the Gaussians' device")


def new_accumulator(n, device):
    """A zeroed H [n, 21] float64."""
    return torch.zeros((int(n), H_WIDTH), dtype=torch.float64, device=device)


def _forward(camera, model, pipe, bg, options, override_color):
    """The ordinary colour forward of the view without autograd: (call, radii, geom, binning, img, num_rendered)."""
    options = _pipe_options(pipe, options)
    opts = _rasterizer.resolve_options(options)
    if opts["antialiasing"]:
        raise NotImplementedError("sensitivity is not implemented with antialiasing: the compensated opacity depends on the covariance, "
                                  "which needs an opacity column")
    if isinstance(model, (CompressedGaussians, TrainableCompressed)):
        raise NotImplementedError("sensitivity needs the dense tensors: pass model.to_dense() instead")
    if pipe.compute_cov3D_python:
        raise NotImplementedError("sensitivity needs scales and rotations: compute_cov3D_python hands the renderer covariances only")
    with torch.no_grad():
        means3D, opacity, scales, rotations, _cov, shs, colors_precomp = _inputs(camera, model, pipe, 1.0, override_color, options)
        rs = _settings(camera, model, pipe, bg, 1.0, False)
        call = _Call(rs, means3D, shs, colors_precomp, opacity, scales, rotations, None, exact=False, opts=opts, differentiated=False)
        with torch.cuda.device(call.dev):
            _color, radii, _gc, _sc, geom, binning, img, num_rendered = _native_forward(load(), call, rs, False)
    return call, radii, geom, binning, img, num_rendered


def _accumulate_view(state, H):
    """lg_sensitivity_accumulate on what _forward left."""
    lib = load()
    call, radii, geom, binning, img, num_rendered = state
    if call.N == 0:
        return H
    with torch.cuda.device(call.dev):
        scratch = _lib.scratch(lib.lg_sensitivity_scratch_bytes(call.N, num_rendered), call.dev)
        _lib.check(lib.lg_sensitivity_accumulate(C.byref(call.view), C.byref(call.g), _lib.ptr(radii), _lib.ptr(geom),
                                                 _lib.ptr(binning) if binning is not None and binning.numel() else None, _lib.ptr(img),
                                                 C.c_int64(num_rendered), _lib.ptr(H), _lib.ptr(scratch), _lib.stream()))
    return H


def accumulate(camera, model, pipe, bg, H=None, *, options=None, override_color=None):
    """Adds the view's blocks into H [N, 21] float64 (the upper triangle of every Gaussian's 6 x 6 block over (xyz, activated scale),
    row-major; None: a zeroed accumulator is made) and returns it.  One ordinary forward of the view without autograd, then
    lg_sensitivity_accumulate on the buffers it left.  A Gaussian the view does not see keeps its block.  options: the rasterizer's, as
    for render(); override_color: [N, 3] colours in place of the model's SH colours, as for render().  `antialiasing` (option or
    pipe.antialiasing) raises NotImplementedError, as do compressed models and pipe.compute_cov3D_python."""
    state = _forward(camera, model, pipe, bg, options, override_color)
    call = state[0]
    if H is None:
        H = new_accumulator(call.N, call.dev)
    _check_H(H, call.N, call.dev)
    return _accumulate_view(state, H)


def _rendered_scales(model, options=None):
    """The activated scales the rasterizer receives: the model's, with its filter_3D applied when it carries one."""
    with torch.no_grad():
        scales = model.get_scaling
        f = _filter3d.model_filter(model, options)
        if f is not None:
            scales, _op = _filter3d.apply_filter_3d_activated(scales, model.get_opacity, f)
        return scales.detach().float().contiguous()


def score(H, model=None, scale_space="linear", *, options=None):
    """[N] float64: log det of every block of H (Cholesky in float64 on the device); -inf for a block that is not positive definite -- a
    Gaussian no view saw, or whose views do not span six directions -- which every prune ranks first.  scale_space="log": with respect
    to the log-scales, the linear score plus 2 sum_k log s_k of the scales `model` is rendered with (model required)."""
    if scale_space not in ("linear", "log"):
        raise ValueError(f"scale_space must be 'linear' or 'log', not {scale_space!r}")
    if not torch.is_tensor(H) or H.dim() != 2:
        raise ValueError(f"H must be a float64 [N, {H_WIDTH}] tensor")
    if H.device.type != "cuda":
        raise RuntimeError("sensitivity.score needs H on a HIP device (torch 'cuda'); there is no CPU path")
    n = int(H.shape[0])
    _check_H(H, n, H.device)
    scales = None
    if scale_space == "log":
        if model is None:
            raise ValueError("scale_space='log' needs the model (its scales)")
        scales = _rendered_scales(model, options).to(H.device)
        if tuple(scales.shape) != (n, 3):
            raise ValueError(f"the model has {int(scales.shape[0])} Gaussians, H has {n} rows")
    lib = load()
    with torch.cuda.device(H.device):
        out = torch.empty(n, dtype=torch.float64, device=H.device)
        _lib.check(lib.lg_sensitivity_score(n, _lib.ptr(H), _lib.ptr(scales) if n else None, _lib.ptr(out), _lib.stream()))
    return out


def sensitivity_list(gaussians, scene_or_cameras, pipe, background, *, options=None):
    """H [N, 21] float64 summed over the training cameras (a Scene, or a list of cameras), as prune.prune_list does for the significance
    score: the getters are evaluated once, the views are taken from the end of the list.  score(H, gaussians, ...) ranks it."""
    from .prune import _FrozenGetters, _train_cameras
    frozen = _FrozenGetters(gaussians)
    if getattr(gaussians, "filter_3D", None) is not None:
        frozen.filter_3D = gaussians.filter_3D
    stack = _train_cameras(scene_or_cameras)
    H = None
    while stack:
        H = accumulate(stack.pop(), frozen, pipe, background, H, options=options)
    if H is None:
        H = new_accumulator(int(gaussians.get_xyz.shape[0]), gaussians.get_xyz.device)
    return H
