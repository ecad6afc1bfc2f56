"""Blend per-Gaussian feature channels over a view's tile lists.

The blend kernels composite three channels.  Any other per-pixel quantity under the same blending weights w = alpha T -- an
accumulated-opacity map, expected depth, normals, a feature vector learnt on a frozen scene -- used to cost one full
render(..., override_color=...) per three channels: K1, the scan, the duplication, both sort stages again, and a K7 + K9 backward
for a gradient that is linear in the weights.  blend_features runs the ordinary forward ONCE and then lg_blend_features
(csrc/lg_features.h) on the lists that forward left: up to 64 channels per call, `alpha` for free, and a backward
(lg_blend_features_backward) that walks the lists once more and gathers one row per Gaussian -- no float atomics, bit-identical
run to run.

blend_features(..., geometry_grad=True) makes the maps differentiable with respect to the GEOMETRY as well: the backward
(lg_backward_features) runs K7 for a colour loss, adds the pixel-offset moments of the feature / alpha loss to the same per-instance
rows with one more back-to-front walk of the lists per group of channels (lg_features_bwd_geom), and K9 once -- a joint photometric +
depth + alpha loss costs one forward and one backward.
"""
import ctypes as C
import warnings

import torch

from . import _lib
from . import rasterizer as _rasterizer
from .rasterizer import _bare_view, _Call, _finish_forward, _GradSet, _native_forward, _prep

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


def _forward_then_blend(features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options,
                        differentiated):
    """The ordinary forward of the view, then lg_blend_features over the lists it left.  Returns (opts, call, bg, the outputs
    (out, alpha, color, radii), the buffers (geom, binning, img), num_rendered)."""
    lib = _lib.load()
    opts = _rasterizer.resolve_options(options)
    call = _Call(rs, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, exact=False, opts=opts,
                 differentiated=differentiated)
    if features.device != call.dev or features.shape[0] != call.N:
        raise ValueError("features must hold one row per Gaussian, on the Gaussians' device")
    dev, c = call.dev, int(features.shape[1])
    h, w = int(rs.image_height), int(rs.image_width)
    bg = _prep(bg_features, dev)
    with torch.cuda.device(dev):
        color, radii, _gc, _sc, geom, binning, img, num_rendered = _native_forward(lib, call, rs, False)
        out = torch.empty((c, h, w), dtype=torch.float32, device=dev)
        alpha = torch.empty((h, w), dtype=torch.float32, device=dev)
        _lib.check(lib.lg_blend_features(C.byref(call.view), call.N, _lib.ptr(geom), _lib.ptr(binning), C.c_int64(num_rendered), _lib.ptr(features), c,
                                         _lib.ptr(bg), _lib.ptr(out), _lib.ptr(alpha), _lib.stream()))
    if binning is None:     # (an empty tensor stands in for it among the saved ones)
        binning = torch.empty(0, dtype=torch.uint8, device=dev)
    return opts, call, bg, (out, alpha, color, radii), (geom, binning, img), num_rendered


class _BlendFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options):
        _opts, call, _bg, outputs, (geom, binning, _img), num_rendered = _forward_then_blend(
            features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options, differentiated=False)
        ctx.raster_settings = rs
        ctx.view_flags = (int(call.view.flags), int(call.view.segment_length))
        ctx.shape = tuple(features.shape)
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(geom, binning)
        ctx.mark_non_differentiable(*outputs[1:])       # alpha, color, radii: functions of the geometry, which is a constant here
        ctx.set_materialize_grads(False)
        return outputs

    @staticmethod
    def backward(ctx, grad_out, *_unused):
        none = (None,) * 10
        if grad_out is None or not ctx.needs_input_grad[0]:
            return (None,) + none
        lib = _lib.load()
        geom, binning = ctx.saved_tensors
        n, c = ctx.shape
        dev = geom.device
        grad_out = _prep(grad_out, dev)
        view = _bare_view(ctx.raster_settings, *ctx.view_flags)
        with torch.cuda.device(dev):
            d_feat = torch.empty((n, c), dtype=torch.float32, device=dev)
            scratch = _lib.scratch(lib.lg_features_scratch_bytes(n, ctx.num_rendered, c), dev)
            _lib.check(lib.lg_blend_features_backward(C.byref(view), n, _lib.ptr(geom), _lib.ptr(binning) if binning.numel() else None,
                                                      C.c_int64(ctx.num_rendered), _lib.ptr(grad_out), c, _lib.ptr(d_feat), _lib.ptr(scratch), _lib.stream()))
        return (d_feat,) + none


def _geometry_backward(ctx, grads, launch, *, trailing, feat_zeros):
    """The backward of _BlendFeaturesGeom and of distortion._BlendGeometry around their library call.  grads: the incoming gradients of
    the feature image, alpha and colour, then the function's own.  trailing: the inputs behind the ten tensors, a None each.  feat_zeros:
    dL/dfeatures is wanted (zeros) also without a gradient on the feature image.  launch(head, n, c, dev, grads, g_feat) runs when there
    is something to walk: head holds the arguments lg_backward_features and lg_backward_distortion share (view .. dL_dshs_rest)."""
    features, bg, means3D, sh, colors, opac, scales, rots, cov, radii, geom, binning, img = ctx.saved_tensors[:13]
    if features.shape[0] == 0:          # an empty model: nothing was rendered, and the empty inputs were not kept
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=features.device)  # noqa: E731
        return (z(0, features.shape[1]), None, z(0, 3), z(0, 3), z(0, 1)) + (None,) * (5 + trailing)
    call = _Call(ctx.raster_settings, means3D, sh, colors, opac, scales, rots, cov, exact=False, opts=ctx.opts, differentiated=True)
    dev, n, c = call.dev, call.N, int(features.shape[1])
    grads = [_prep(t, dev) for t in grads]
    grad_out, grad_alpha, grad_color = grads[:3]
    with torch.cuda.device(dev):
        run = n > 0 and binning.numel() > 0       # (no Gaussians, or a forward that left no binning buffer: zero gradients)
        new = torch.empty if run else torch.zeros
        g = _GradSet(call, new=new)
        g_feat = None
        if ctx.needs_input_grad[0] and (grad_out is not None or feat_zeros):
            g_feat = (new if grad_out is not None else torch.zeros)((n, c), dtype=torch.float32, device=dev)
        if run:
            head = (C.byref(call.view), C.byref(call.g), _lib.ptr(radii), _lib.ptr(geom), _lib.ptr(binning), _lib.ptr(img),
                    C.c_int64(ctx.num_rendered), _lib.ptr(grad_color), _lib.ptr(features), c, _lib.ptr(bg) if bg.numel() else None,
                    _lib.ptr(grad_out), _lib.ptr(grad_alpha), *g.ptrs())
            launch(head, n, c, dev, grads, g_feat)
    return (g_feat, None, g["means3D"], g["means2D"], g["opacity"], g["scales"], g["rotations"], g["cov3D"], g["shs"],
            g["colors"]) + (None,) * trailing


class _BlendFeaturesGeom(torch.autograd.Function):
    """blend_features(geometry_grad=True): a DIFFERENTIATED forward that keeps the img buffer, as _RasterizeGaussians does; out, alpha
    and color are differentiable, radii is not.  The backward is one lg_backward_features call."""

    @staticmethod
    def forward(ctx, features, bg_features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options):
        opts, call, bg, outputs, (geom, binning, img), num_rendered = _forward_then_blend(
            features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options, differentiated=True)
        _finish_forward(ctx, rs, num_rendered, opts)
        ctx.save_for_backward(features, bg if bg is not None else binning.new_empty(0), call.means3D, call.sh, call.colors, call.opac,
                              call.scales, call.rots, call.cov, outputs[3], geom, binning, img)
        ctx.mark_non_differentiable(outputs[3])        # radii
        return outputs

    @staticmethod
    def backward(ctx, grad_out, grad_alpha, grad_color, _grad_radii=None):
        lib = _lib.load()

        def launch(head, n, c, dev, _grads, g_feat):
            scratch = _lib.scratch(lib.lg_backward_features_scratch_bytes(n, ctx.num_rendered, c), dev)
            _lib.check(lib.lg_backward_features(*head, _lib.ptr(g_feat), _lib.ptr(scratch), _lib.stream()))

        return _geometry_backward(ctx, (grad_out, grad_alpha, grad_color), launch, trailing=2, feat_zeros=False)


def blend_features(raster_settings, features, *, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, shs=None,
                   colors_precomp=None, bg_features=None, options=None, geometry_grad=False, means2D=None):
    """(features_image [C,H,W], alpha [H,W], color [3,H,W], radii [N]) of one view.

    Runs the ordinary forward (the colour image is a by-product; the rasterizer options -- fast_exp, segment_length, sync_free,
    ... -- apply unchanged, as `options=` or through rasterizer.options) and then blends `features` [N, C] float32 contiguous,
    1 <= C <= 64, over the same tile lists with the same weights:  features_image_c = sum_j f[j, c] alpha_j T_j + T_final bg_features[c],
    alpha = sum_j alpha_j T_j (= 1 - T_final up to rounding; bit for bit the blend of a column of ones).  With fast_exp=False a triple of
    channels equals the colour image of the same colours bit for bit.

    Differentiable with respect to `features` ONLY: the geometry inputs (means3D, opacities, scales, rotations, cov3D_precomp, shs,
    colors_precomp) and bg_features are constants of this function -- its backward returns None for them, and alpha / color carry no
    gradient.  A loss on feature maps that should move the geometry needs a second, ordinary render.  A warning is issued once when a
    geometry input requires grad.  The gradient is summed in a fixed order: two backward calls give identical bits.

    geometry_grad=True: the forward is a differentiated one and features_image, alpha and color are all differentiable -- with respect
    to `features` as above (the same bits) and to means3D, opacities, scales / rotations or cov3D_precomp, shs or colors_precomp, and
    means2D ([N, 3], optional: its gradient is the view-space one densification statistics read).  Any subset of the three maps may
    enter the loss; one backward call (lg_backward_features) serves them all, deterministic like the rasterizer's.  No warning."""
    if raster_settings.f_count:
        raise ValueError("blend_features runs on a colour forward: raster_settings.f_count must be False")
    if means2D is not None and not geometry_grad:
        raise ValueError("means2D receives the view-space gradient: it needs geometry_grad=True")
    if _rasterizer.option_value("camera_grad", options):
        raise NotImplementedError("camera_grad is not implemented for feature blending: use render() for the pose gradient")
    _check_features(features, bg_features)
    _rasterizer._check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
    if geometry_grad:
        if means2D is None:
            means2D = torch.zeros(0, dtype=torch.float32, device=means3D.device)
        return _BlendFeaturesGeom.apply(features, bg_features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, shs,
                                        colors_precomp, raster_settings, options)
    geometry = (means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp)
    if not _warned[0] and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in geometry):
        _warned[0] = True
        warnings.warn("blend_features: the geometry inputs are constants of this function -- no gradient reaches means3D, opacities, "
                      "scales, rotations, cov3D_precomp, shs or colors_precomp (use an ordinary render for those)", stacklevel=2)
    return _BlendFeatures.apply(features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp,
                                raster_settings, options)
