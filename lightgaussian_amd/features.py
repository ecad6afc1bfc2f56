"""Blend per-Gaussian feature channels over a view's tile lists.

The blend kernels composite three channels.  Any other per-pixel quantity under the same blending weights w = alpha T -- an
accumulated-opacity map, expected depth, normals, a feature vector learnt on a frozen scene -- used to cost one full
render(..., override_color=...) per three channels: K1, the scan, the duplication, both sort stages again, and a K7 + K9 backward
for a gradient that is linear in the weights.  blend_features runs the ordinary forward ONCE and then lg_blend_features
(csrc/lg_features.h) on the lists that forward left: up to 64 channels per call, `alpha` for free, and a backward
(lg_blend_features_backward) that walks the lists once more and gathers one row per Gaussian -- no float atomics, bit-identical
run to run.
"""
import ctypes as C
import warnings

import torch

from . import _lib
from . import rasterizer as _rasterizer
from .rasterizer import _Call, _native_forward, _prep, _ptr

FEATURES_MAX = _lib.FEATURES_MAX
_warned = [False]


def _check_features(features, bg_features):
    """Everything that can be refused without touching the device, in that order: type, dtype, rank, layout, channel count,
    background length, and last the device (there is no CPU path)."""
    if not torch.is_tensor(features):
        raise TypeError("features must be a torch tensor [N, C]")
    if features.dtype != torch.float32:
        raise TypeError(f"features must be float32, not {features.dtype}")
    if features.dim() != 2:
        raise ValueError(f"features must be [N, C], not {tuple(features.shape)}")
    if not features.is_contiguous():
        raise ValueError("features must be contiguous (call .contiguous() on a sliced or transposed tensor)")
    c = int(features.shape[1])
    if c < 1 or c > FEATURES_MAX:
        raise ValueError(f"features has {c} channels: 1 .. {FEATURES_MAX} per call (split wider tensors)")
    if bg_features is not None:
        if not torch.is_tensor(bg_features) or bg_features.dtype != torch.float32 or tuple(bg_features.shape) != (c,):
            raise ValueError(f"bg_features must be a float32 tensor of {c} values, one per channel")
    if features.device.type != "cuda":
        raise RuntimeError("blend_features needs tensors on a HIP device (torch 'cuda'); there is no CPU path")


class _BlendFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options):
        lib = _lib.load()
        opts = _rasterizer.resolve_options(options)
        call = _Call(rs, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, exact=False, opts=opts,
                     differentiated=False)
        if features.device != call.dev or features.shape[0] != call.N:
            raise ValueError("features must hold one row per Gaussian, on the Gaussians' device")
        dev, n, c = call.dev, call.N, int(features.shape[1])
        h, w = int(rs.image_height), int(rs.image_width)
        bg = _prep(bg_features, dev)
        with torch.cuda.device(dev):
            color, radii, _gc, _sc, geom, binning, _img, num_rendered = _native_forward(lib, call, rs, False)
            out = torch.empty((c, h, w), dtype=torch.float32, device=dev)
            alpha = torch.empty((h, w), dtype=torch.float32, device=dev)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.lg_blend_features(C.byref(call.view), n, _ptr(geom), _ptr(binning), C.c_int64(num_rendered), _ptr(features), c,
                                             _ptr(bg), _ptr(out), _ptr(alpha), stream))
        ctx.view_args = (h, w, float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier), int(rs.sh_degree), int(call.view.flags),
                         int(call.view.segment_length))
        ctx.shape = (n, c)
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(geom, binning if binning is not None else torch.empty(0, dtype=torch.uint8, device=dev))
        ctx.mark_non_differentiable(alpha, color, radii)       # functions of the geometry, which is a constant here
        ctx.set_materialize_grads(False)
        return out, alpha, color, radii

    @staticmethod
    def backward(ctx, grad_out, *_unused):
        none = (None,) * 10
        if grad_out is None or not ctx.needs_input_grad[0]:
            return (None,) + none
        lib = _lib.load()
        geom, binning = ctx.saved_tensors
        n, c = ctx.shape
        h, w, tanx, tany, mod, deg, flags, seg = ctx.view_args
        dev = geom.device
        grad_out = _prep(grad_out, dev)
        # only the image size, the flags and the segment length of the forward's view are read
        view = _lib.lg_view(h, w, tanx, tany, None, mod, None, None, deg, None, 0, flags, seg)
        with torch.cuda.device(dev):
            d_feat = torch.empty((n, c), dtype=torch.float32, device=dev)
            scratch = torch.empty(max(int(lib.lg_features_scratch_bytes(n, ctx.num_rendered, c)), 1), dtype=torch.uint8, device=dev)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.lg_blend_features_backward(C.byref(view), n, _ptr(geom), _ptr(binning) if binning.numel() else None,
                                                      C.c_int64(ctx.num_rendered), _ptr(grad_out), c, _ptr(d_feat), _ptr(scratch), stream))
        return (d_feat,) + none


def blend_features(raster_settings, features, *, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, shs=None,
                   colors_precomp=None, bg_features=None, options=None):
    """(features_image [C,H,W], alpha [H,W], color [3,H,W], radii [N]) of one view.

    Runs the ordinary forward (the colour image is a by-product; the rasterizer options -- fast_exp, segment_length, sync_free,
    ... -- apply unchanged, as `options=` or through rasterizer.options) and then blends `features` [N, C] float32 contiguous,
    1 <= C <= 64, over the same tile lists with the same weights:  features_image_c = sum_j f[j, c] alpha_j T_j + T_final bg_features[c],
    alpha = sum_j alpha_j T_j (= 1 - T_final up to rounding; bit for bit the blend of a column of ones).  With fast_exp=False a triple of
    channels equals the colour image of the same colours bit for bit.

    Differentiable with respect to `features` ONLY: the geometry inputs (means3D, opacities, scales, rotations, cov3D_precomp, shs,
    colors_precomp) and bg_features are constants of this function -- its backward returns None for them, and alpha / color carry no
    gradient.  A loss on feature maps that should move the geometry needs a second, ordinary render.  A warning is issued once when a
    geometry input requires grad.  The gradient is summed in a fixed order: two backward calls give identical bits."""
    if raster_settings.f_count:
        raise ValueError("blend_features runs on a colour forward: raster_settings.f_count must be False")
    _check_features(features, bg_features)
    _rasterizer._check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
    geometry = (means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp)
    if not _warned[0] and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in geometry):
        _warned[0] = True
        warnings.warn("blend_features: the geometry inputs are constants of this function -- no gradient reaches means3D, opacities, "
                      "scales, rotations, cov3D_precomp, shs or colors_precomp (use an ordinary render for those)", stacklevel=2)
    return _BlendFeatures.apply(features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp,
                                raster_settings, options)
