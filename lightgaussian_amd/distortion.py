"""Depth distortion and median depth of a view (2DGS, GOF, PGSR, RaDe-GS), next to the feature blend of the same forward.

Per pixel, with the blending weights w_i = alpha_i T_i and a per-Gaussian scalar m_i (one column of the feature tensor):

    distortion = sum_{i<j} w_i w_j (m_i - m_j)^2
    median     = the m of the entry that carries T across one half (the last contributor when T never gets there; 0 without one)

    blend_geometry(raster_settings, features, m_column=..., ...) -> (features_image, alpha, color, radii, distortion, median)

is features.blend_features(geometry_grad=True) with the two maps added: ONE ordinary forward, lg_blend_features and
lg_blend_distortion (csrc/lg_distortion.h) over the tile lists it left, and ONE backward call, lg_backward_distortion: K7 for the colour
loss, the feature walks, the distortion walk into the same moment rows, K9 once.  Every map is differentiable with respect to the
geometry and to `features`; the gradient of the two maps with respect to m is added into column m_column of dL/dfeatures.  The
median's selection is piecewise constant: its gradient reaches the selected Gaussian's m only.

distortion equals A M2 - M1^2 of the blended columns [1, m, m m] in exact arithmetic; in float32 that difference cancels where the loss
matters (a thin surface far from the camera: the composed form is wrong by several times the value at depth 30 +- 0.02), so the kernel
accumulates about the pixel's first contributor (lg_math.h: lg_distortion_step).

For unbounded scenes 2DGS measures the distortion in NDC depth: put ndc_depth(z, near, far) in a further feature column and name it
as m_column."""
import ctypes as C

import torch

from . import _lib
from . import rasterizer as _rasterizer
from .features import _check_features, _forward_then_blend, _geometry_backward
from .rasterizer import _finish_forward

# The C ABI of include/lightgaussian_distortion.h, in header order: name -> (restype, argtypes).  tests/test_distortion_host.py holds
# every entry against the header.
i32, i64, sz, vp = C.c_int32, C.c_int64, C.c_size_t, C.c_void_p
PROTOTYPES = {
    "lg_distortion_state_bytes": (sz, (i32, i32)),
    "lg_blend_distortion": (C.c_int, (vp, i32, vp, vp, i64, vp, i32, vp, vp, vp, vp)),
    "lg_backward_distortion_scratch_bytes": (sz, (i32, i64, i32)),
    "lg_backward_distortion": (C.c_int, (vp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp) + (vp,) * 9 + (vp, vp, i32, vp, vp, vp, vp, vp, vp)),
}
def load():
    """The library object of _lib.load() with the prototypes of include/lightgaussian_distortion.h set on it."""
    return _lib.bind(_lib.load(), PROTOTYPES)


def ndc_depth(z, near, far):
    """2DGS's mapping of view-space depth z [N] to NDC depth, far / (far - near) - far near / ((far - near) z): the m of the distortion
    term for unbounded scenes (differentiable torch ops)."""
    if not (far > near > 0):
        raise ValueError(f"ndc_depth needs 0 < near < far, not near={near}, far={far}")
    return far / (far - near) - (far * near) / ((far - near) * z)


def _column_ptr(features, m_column):
    """Column m_column of a contiguous [N, C] float32 tensor as a pointer (stride C floats); NULL for an empty tensor."""
    return C.c_void_p(features.data_ptr() + 4 * m_column) if features.numel() else None


class _BlendGeometry(torch.autograd.Function):
    """features._BlendFeaturesGeom with the distortion and median maps of the same differentiated forward; the backward is one
    lg_backward_distortion call."""

    @staticmethod
    def forward(ctx, features, bg_features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options,
                m_column):
        lib = load()
        opts, call, bg, outputs, (geom, binning, img), num_rendered = _forward_then_blend(
            features, bg_features, means3D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp, rs, options, differentiated=True)
        dev, n, c = call.dev, call.N, int(features.shape[1])
        h, w = int(rs.image_height), int(rs.image_width)
        with torch.cuda.device(dev):
            distortion = torch.empty((h, w), dtype=torch.float32, device=dev)
            median = torch.empty((h, w), dtype=torch.float32, device=dev)
            state = _lib.scratch(lib.lg_distortion_state_bytes(w, h), dev)
            _lib.check(lib.lg_blend_distortion(C.byref(call.view), n, _lib.ptr(geom), _lib.ptr(binning) if binning.numel() else None,
                                               C.c_int64(num_rendered), _column_ptr(features, m_column), c, _lib.ptr(distortion), _lib.ptr(median),
                                               _lib.ptr(state), _lib.stream()))
        _finish_forward(ctx, rs, num_rendered, opts)
        ctx.m_column = m_column
        ctx.save_for_backward(features, bg if bg is not None else binning.new_empty(0), call.means3D, call.sh, call.colors, call.opac,
                              call.scales, call.rots, call.cov, outputs[3], geom, binning, img, state)
        ctx.mark_non_differentiable(outputs[3])        # radii
        return outputs + (distortion, median)

    @staticmethod
    def backward(ctx, grad_out, grad_alpha, grad_color, _grad_radii=None, grad_dist=None, grad_median=None):
        lib = load()
        features, state = ctx.saved_tensors[0], ctx.saved_tensors[13]

        def launch(head, n, c, dev, grads, g_feat):
            g_m = torch.empty(n, dtype=torch.float32, device=dev)
            scratch = _lib.scratch(lib.lg_backward_distortion_scratch_bytes(n, ctx.num_rendered, c), dev)
            _lib.check(lib.lg_backward_distortion(
                *head, _lib.ptr(g_feat) if grads[0] is not None else None, _column_ptr(features, ctx.m_column), c, _lib.ptr(state),
                _lib.ptr(grads[3]), _lib.ptr(grads[4]), _lib.ptr(g_m), _lib.ptr(scratch), _lib.stream()))
            if g_feat is not None:
                g_feat[:, ctx.m_column] += g_m

        # (without a gradient on the feature image the library writes no dL_dfeatures: zeros, plus the dL_dm column)
        return _geometry_backward(ctx, (grad_out, grad_alpha, grad_color, grad_dist, grad_median), launch, trailing=3, feat_zeros=True)


def blend_geometry(raster_settings, features, *, m_column, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, shs=None,
                   colors_precomp=None, bg_features=None, options=None, means2D=None):
    """(features_image [C,H,W], alpha [H,W], color [3,H,W], radii [N], distortion [H,W], median [H,W]) of one view.

    The first four are features.blend_features(..., geometry_grad=True)'s, the same bits.  distortion and median are taken over
    m = features[:, m_column] (passed with its stride, no copy), with the weights of the same forward.  All maps but radii are
    differentiable with respect to `features`, means3D, opacities, scales / rotations or cov3D_precomp, shs or colors_precomp and means2D
    ([N, 3], optional: the view-space gradient); any subset may enter the loss, one backward call serves them all, and the sums run in a
    fixed order: two backward calls give identical bits.  The rasterizer options apply as for blend_features."""
    if raster_settings.f_count:
        raise ValueError("blend_geometry runs on a colour forward: raster_settings.f_count must be False")
    if _rasterizer.option_value("camera_grad", options):
        raise NotImplementedError("camera_grad is not implemented for feature blending: use render() for the pose gradient")
    _check_features(features, bg_features)
    if not isinstance(m_column, int) or isinstance(m_column, bool) or not 0 <= m_column < features.shape[1]:
        raise ValueError(f"m_column must be a column index of features, 0 .. {features.shape[1] - 1}, not {m_column!r}")
    _rasterizer._check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
    if means2D is None:
        means2D = torch.zeros(0, dtype=torch.float32, device=means3D.device)
    return _BlendGeometry.apply(features, bg_features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, shs, colors_precomp,
                                raster_settings, options, m_column)
