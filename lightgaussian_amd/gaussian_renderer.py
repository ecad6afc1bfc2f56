"""Host-side mirror of the reference's render boundary (gaussian_renderer/__init__.py).

render()        <- gaussian_renderer/__init__.py:22-124
count_render()  <- gaussian_renderer/__init__.py:127-229
Same names, argument meaning, result-dict keys and error behaviour; the only change is the import
target of the rasterizer (our HIP library instead of the CUDA submodule) and that tensors are
created on the Gaussians' own device instead of the hard-coded "cuda" (identical on one GPU,
required for one-process-per-GPU sharding).
"""
import contextlib
import math
import threading

import torch

from . import filter3d as _filter3d
from . import rasterizer as _rasterizer
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians_raw
from .sh_utils import eval_sh
from .vectree import CompressedGaussians, TrainableCompressed


def _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, f_count):
    tanfovx = math.tan(viewpoint_camera.FoVx * 0.5)
    tanfovy = math.tan(viewpoint_camera.FoVy * 0.5)
    return GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height),
        image_width=int(viewpoint_camera.image_width),
        tanfovx=tanfovx,
        tanfovy=tanfovy,
        bg=bg_color,
        scale_modifier=scaling_modifier,
        viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center,
        prefiltered=False,
        debug=pipe.debug,
        f_count=f_count,
    )


def _filter_3d(pc, pipe, options):
    """The model's 3D smoothing filter if this call is to honour one (filter3d.model_filter: `pc.filter_3D`, option "filter_3d"), else
    None -- a model without the attribute, the reference's GaussianModel, takes the code path it always took."""
    f = _filter3d.model_filter(pc, options)
    if f is not None and pipe.compute_cov3D_python:
        raise NotImplementedError("compute_cov3D_python with a filter_3D is not implemented: the filter is applied to the scales "
                                  "(render with options={'filter_3d': False}, or without compute_cov3D_python)")
    return f


def _inputs(viewpoint_camera, pc, pipe, scaling_modifier, override_color, options=None):
    means3D = pc.get_xyz
    opacity = pc.get_opacity
    scales = rotations = cov3D_precomp = None
    filter_3d = _filter_3d(pc, pipe, options)
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)
    else:
        scales = pc.get_scaling
        rotations = pc.get_rotation
        if filter_3d is not None:       # upstream's get_scaling_with_3D_filter / get_opacity_with_3D_filter, one launch
            scales, opacity = _filter3d.apply_filter_3d_activated(scales, opacity, filter_3d)
    shs = colors_precomp = None
    if override_color is None:
        if pipe.convert_SHs_python:
            shs_view = pc.get_features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = pc.get_xyz - viewpoint_camera.camera_center.repeat(pc.get_features.shape[0], 1)
            dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            sh2rgb = eval_sh(pc.active_sh_degree, shs_view, dir_pp_normalized)
            colors_precomp = torch.clamp_min(sh2rgb + 0.5, 0.0)
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color
    return means3D, opacity, scales, rotations, cov3D_precomp, shs, colors_precomp


def _camera_grad(options):
    return bool(_rasterizer.option_value("camera_grad", options))


def _pipe_options(pipe, options):
    """`options` with "antialiasing" switched on for a `pipe` that asks for it (the `antialiasing` attribute of upstream 3DGS's
    PipelineParams; the reference's has none, so nothing changes for it) unless the call's own options set the key."""
    if getattr(pipe, "antialiasing", False) and not (options and "antialiasing" in options):
        return dict(options or {}, antialiasing=True)
    return options


def _screenspace_points(pc):
    """Zero tensor whose .grad receives the 2D (NDC) mean gradients, gaussian_renderer/__init__.py:37-46.  The reference
    builds it as zeros(..., requires_grad=True) + 0 followed by retain_grad(); a plain leaf gets its .grad the same way
    and saves the add, its autograd node and the clone retain_grad() makes at the end of every backward (~25 us per step
    at 3M Gaussians)."""
    xyz = pc.get_xyz
    if not xyz.is_cuda or torch.is_inference_mode_enabled():      # (inference tensors cannot share a normal buffer's leaf machinery)
        return torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device=xyz.device)
    # Nothing ever writes this tensor (it exists for its .grad), so every view's leaf can share ONE zero buffer per device and
    # shape: detach() gives a fresh leaf -- its own .grad, its own identity in the render package -- over the same storage, and
    # the 36 MB fill per render (3M Gaussians: ~8 us) happens once.
    key = (xyz.device.index, tuple(xyz.shape), xyz.dtype)
    with _ZERO_LOCK:
        buf = _ZERO_POINTS.pop(key, None)
        if buf is None:
            buf = torch.zeros_like(xyz, requires_grad=False)
        _ZERO_POINTS[key] = buf                       # most recently used last
        # a few shapes per process (distill_train.py renders a teacher and a student of different N in every iteration; a prune
        # changes N): least recently used out, under the lock (backward_over_views(host_threads=True) renders from several threads)
        while len(_ZERO_POINTS) > _ZERO_KEEP:
            _ZERO_POINTS.pop(next(iter(_ZERO_POINTS)))
    return buf.detach().requires_grad_(True)


_ZERO_POINTS = {}
_ZERO_LOCK = threading.Lock()
_ZERO_KEEP = 4


_RAW_FIELDS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _has_reference_getters(pc):
    """True when `pc` is a GaussianModel whose getters are exactly the reference's (scene/gaussian_model.py:36-47 and
    :98-118: get_scaling = torch.exp(_scaling), get_opacity = torch.sigmoid(_opacity), get_rotation =
    F.normalize(_rotation), get_features = cat(_features_dc, _features_rest)) -- identified by the activation attributes
    setup_functions() installs.  Anything else (frozen getters, custom activations, foreign models) is not touched."""
    if not all(hasattr(pc, n) for n in _RAW_FIELDS):
        return False
    return (getattr(pc, "scaling_activation", None) is torch.exp and getattr(pc, "opacity_activation", None) is torch.sigmoid
            and getattr(pc, "rotation_activation", None) is torch.nn.functional.normalize
            and pc._features_rest.dim() == 3 and pc._features_dc.dim() == 3 and pc._features_dc.shape[1] == 1)


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None, *, options=None):
    """Render the scene.  Background tensor (bg_color) must be on the GPU.
    options (keyword-only extension): per-call overrides of the rasterizer knobs (rasterizer.set_option), e.g.
    {"sync_free": True}; the reference's six positional parameters are unchanged.

    With option fuse_getters (default True) and a GaussianModel carrying the reference's own activations, the getters
    are evaluated INSIDE the kernels from the raw parameters (render_fused: no torch.cat of the SH tensors, no
    activation kernels; same values to ~1e-7, gradients land on the raw parameters exactly as autograd would route
    them).  set_option("fuse_getters", False) restores the reference's literal call pattern.

    options={"camera_grad": True}: the image is also differentiable with respect to the camera's own world_view_transform,
    full_proj_transform and camera_center tensors, which are handed through as they are -- built under autograd (pose.PoseCamera),
    the chain continues into the pose parameters.  Fused and unfused paths alike; compressed models are not supported.

    A `pipe` with a true `antialiasing` attribute (upstream 3DGS's spelling) renders with options={"antialiasing": True} -- the opacity
    compensation of the 0.3-pixel blur, rasterizer.set_option -- unless `options` sets the key itself; count_render and render_features
    read it the same way.

    A model with a `filter_3D` attribute (upstream Mip-Splatting's name: one filter size per Gaussian, filter3d.compute_filter_3d) is
    rendered with the 3D smoothing filter applied to its scales and opacity -- on the fused path raw -> raw in front of the kernels, on
    every other path on the activated getters -- unless options={"filter_3d": False}.  The reference's GaussianModel has no such
    attribute: nothing changes for it.  A filter whose row count is not the model's raises ValueError (recompute it after a
    densification or prune); with pipe.compute_cov3D_python it raises NotImplementedError.

    options={"absgrad": True} (rasterizer.set_option): after backward(), result["viewspace_points"].absgrad holds the ABSOLUTE
    view-space mean gradients, float32 [N,3] in .grad's layout and units (z = 0): per Gaussian the sum over pixels of |dL/dmean2D|
    where .grad holds the |sum|, in which the signed pulls on a large splat over fine structure cancel (AbsGS; gsplat's `absgrad`).
    Overwritten by every backward, not accumulated.  densify.accumulate_stats(..., absgrad=True) reads it; the densification threshold
    usually wants raising 2-4 x with it.  Fused and unfused paths alike; every other output and gradient keeps its bits."""
    options = _pipe_options(pipe, options)
    if isinstance(pc, (CompressedGaussians, TrainableCompressed)) and _camera_grad(options):
        raise NotImplementedError("camera_grad is not implemented for compressed models: render pc.to_dense() instead")
    if isinstance(pc, TrainableCompressed) and override_color is None:
        return render_compressed_trainable(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, options=options)
    if isinstance(pc, CompressedGaussians) and override_color is None:
        return render_compressed(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, options=options)
    if (_rasterizer.resolve_options(options)["fuse_getters"] and override_color is None and not pipe.convert_SHs_python
            and not pipe.compute_cov3D_python and _has_reference_getters(pc)):
        return render_fused(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, options=options)
    return _render_unfused(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, options)


def _render_unfused(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, options=None):
    """gaussian_renderer/__init__.py:22-124 literally: getters in torch, activated tensors into the rasterizer."""
    screenspace_points = _screenspace_points(pc)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, False), options=options)
    means3D, opacity, scales, rotations, cov3D_precomp, shs, colors_precomp = _inputs(
        viewpoint_camera, pc, pipe, scaling_modifier, override_color, options)
    rendered_image, radii = rasterizer(
        means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp, opacities=opacity,
        scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "radii": radii}


def render_compressed(viewpoint_camera, cg, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, *, options=None):
    """render() of a vectree.CompressedGaussians (the reference's extreme_saving model, Scene(load_vq=True)) from its compressed
    form: lg_vq_colors turns (camera, fp16 SH row table + slot) into one RGB triple per Gaussian, and the unfused forward takes
    them as colors_precomp -- the [N, 3 M] float32 SH tensor is never built.  Same result dict as render(), same image bits as
    render() of cg.to_dense() with fuse_getters off.  Forward-only: runs under torch.no_grad(), nothing requires grad (to train,
    use cg.to_dense()).  The Python-side alternates of `pipe` need the dense tensors and are refused."""
    options = _pipe_options(pipe, options)
    if _camera_grad(options):
        raise NotImplementedError("camera_grad is not implemented for compressed models: render cg.to_dense() instead")
    if pipe.convert_SHs_python or pipe.compute_cov3D_python:
        raise NotImplementedError("convert_SHs_python / compute_cov3D_python need the dequantised tensors: render cg.to_dense() instead")
    with torch.no_grad():
        colors = cg.colors(viewpoint_camera.camera_center)
        pkg = _render_unfused(viewpoint_camera, cg, pipe, bg_color, scaling_modifier, colors, options)
    pkg["viewspace_points"] = pkg["viewspace_points"].detach()
    return pkg


def render_compressed_trainable(viewpoint_camera, tc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, *, options=None):
    """The grad-enabled twin of render_compressed for a vectree.TrainableCompressed: the same kernels on the same float16 rows
    (the image bits are render_compressed's), with autograd attached -- tc.colors() is differentiable (lg_vq_colors_bwd), the
    rasterizer returns dL/dcolors_precomp and the geometry gradients, viewspace_points stays attached for its .grad."""
    options = _pipe_options(pipe, options)
    if _camera_grad(options):
        raise NotImplementedError("camera_grad is not implemented for compressed models: render tc.to_dense() instead")
    if pipe.convert_SHs_python or pipe.compute_cov3D_python:
        raise NotImplementedError("convert_SHs_python / compute_cov3D_python need the dequantised tensors: render tc.to_dense() instead")
    colors = tc.colors(viewpoint_camera.camera_center)
    return _render_unfused(viewpoint_camera, tc, pipe, bg_color, scaling_modifier, colors, options)


def count_render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None, *, options=None):
    """render() + per-Gaussian hit count and Global Significance score (f_count=True).  options: as for render(), e.g.
    {"skip_color_in_count": True} for passes that only consume the counts / scores."""
    options = _pipe_options(pipe, options)
    if _camera_grad(options):
        raise NotImplementedError("camera_grad is not implemented for count renders: use render()")
    screenspace_points = _screenspace_points(pc)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, True), options=options)
    means3D, opacity, scales, rotations, cov3D_precomp, shs, colors_precomp = _inputs(
        viewpoint_camera, pc, pipe, scaling_modifier, override_color, options)
    gaussians_count, important_score, rendered_image, radii = rasterizer(
        means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp, opacities=opacity,
        scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "radii": radii, "gaussians_count": gaussians_count, "important_score": important_score}


def render_fused(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None, *, options=None):
    """render() with the getters fused into the kernels (opt-in extension -- the reference's
    render() evaluates exp/sigmoid/normalize and cat(_features_dc, _features_rest) in torch on every call, which at
    3M Gaussians costs as much HBM traffic as the whole rasterizer).  Reads GaussianModel's raw tensors
    (_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation: scene/gaussian_model.py:45-60) directly; same
    result dict, gradients land on the raw parameters.  Falls back to render() for the Python-side alternates."""
    options = _pipe_options(pipe, options)
    if override_color is not None or pipe.convert_SHs_python or pipe.compute_cov3D_python:
        return _render_unfused(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, options)
    screenspace_points = _screenspace_points(pc)
    rs = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, False)
    opacity_raw, scaling_raw = pc._opacity, pc._scaling
    filter_3d = _filter_3d(pc, pipe, options)
    if filter_3d is not None:
        # raw -> raw (lg_filter3d_apply): log-scales and logits come out in the domain LG_FLAG_RAW_PARAMS reads, so the fused path stays;
        # autograd carries the gradients on to _scaling / _opacity through lg_filter3d_apply_bwd
        scaling_raw, opacity_raw = _filter3d.apply_filter_3d(scaling_raw, opacity_raw, filter_3d)
    rendered_image, radii, visible = rasterize_gaussians_raw(pc._xyz, screenspace_points, pc._features_dc, pc._features_rest, opacity_raw,
                                                             scaling_raw, pc._rotation, rs, options)
    # visibility_filter = radii > 0 (gaussian_renderer/__init__.py:121), as K1 left it in the forward's geom buffer: no compare kernel
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": visible,
            "radii": radii}


_DEPTH_EPS = 1e-6


def render_features(viewpoint_camera, pc, pipe, features, bg_features=None, scaling_modifier=1.0, *, options=None, geometry_grad=False,
                    bg_color=None):
    """Blend per-Gaussian feature channels with the view's blending weights (lightgaussian_amd.features.blend_features): ONE ordinary
    forward, then lg_blend_features on the tile lists it left -- no second K1 / binning chain per three channels.

    features: a float32 tensor [N, C], 1 <= C <= 64, or the string "depth": the single channel is then the view-space z of pc.get_xyz
    (evaluated by torch) and the result gains "depth" = features / alpha.clamp_min(1e-6), the expected depth of what the pixel sees.
    bg_features: [C] values behind the last Gaussian (default zeros).  bg_color: the background of the colour by-product (default
    black).  options (keyword-only): the rasterizer knobs, as for render().

    Returns {"features" [C,H,W], "alpha" [H,W], "render" [3,H,W], "radii", "visibility_filter"}.  pc: a GaussianModel of the reference's
    shape, a SyntheticGaussians, or a vectree.CompressedGaussians / TrainableCompressed (colours from lg_vq_colors, as in
    render_compressed).

    geometry_grad=False (default): the model is a CONSTANT of this call: its getters are evaluated without grad, only `features`
    receives a gradient (deterministic, lg_blend_features_backward); alpha, render and depth's denominator carry none.

    geometry_grad=True: the getters (and the "depth" feature) are evaluated under grad, on the unfused inputs path, and "features",
    "alpha", "render" and "depth" (numerator and denominator) are differentiable with respect to the model: one call serves a joint
    photometric + depth + alpha loss, one backward (lg_backward_features) carries it to _xyz, _opacity, _scaling, _rotation and the
    colours.  The result gains "viewspace_points", whose .grad is the view-space gradient densification reads.  Compressed models are
    not supported in this mode."""
    options = _pipe_options(pipe, options)
    from .features import blend_features
    if _camera_grad(options):
        raise NotImplementedError("camera_grad is not implemented for render_features: use render() for the pose gradient")
    compressed = isinstance(pc, CompressedGaussians)
    if geometry_grad and isinstance(pc, (CompressedGaussians, TrainableCompressed)):
        raise NotImplementedError("render_features(geometry_grad=True) needs the dense tensors: pass pc.to_dense() instead")
    if compressed and (pipe.convert_SHs_python or pipe.compute_cov3D_python):
        raise NotImplementedError("convert_SHs_python / compute_cov3D_python need the dequantised tensors: pass pc.to_dense() instead")
    with contextlib.nullcontext() if geometry_grad else torch.no_grad():
        override = pc.colors(viewpoint_camera.camera_center) if compressed else None
        means3D, opacity, scales, rotations, cov3D_precomp, shs, colors_precomp = _inputs(viewpoint_camera, pc, pipe, scaling_modifier, override, options)
        if bg_color is None:
            bg_color = torch.zeros(3, dtype=torch.float32, device=means3D.device)
        want_depth = isinstance(features, str)
        if want_depth:
            if features != "depth":
                raise ValueError(f"features must be a tensor [N, C] or the string 'depth', not {features!r}")
            vm = viewpoint_camera.world_view_transform.to(means3D.device)
            features = (means3D @ vm[:3, 2:3] + vm[3, 2]).contiguous()          # view-space z, [N, 1]
    rs = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, False)
    screenspace_points = _screenspace_points(pc) if geometry_grad else None
    image, alpha, color, radii = blend_features(rs, features, means3D=means3D, opacities=opacity, scales=scales, rotations=rotations,
                                                cov3D_precomp=cov3D_precomp, shs=shs, colors_precomp=colors_precomp, bg_features=bg_features,
                                                options=options, geometry_grad=geometry_grad, means2D=screenspace_points)
    pkg = {"features": image, "alpha": alpha, "render": color, "radii": radii, "visibility_filter": radii > 0}
    if geometry_grad:
        pkg["viewspace_points"] = screenspace_points
    if want_depth:
        pkg["depth"] = image / alpha.clamp_min(_DEPTH_EPS)
    return pkg


def render_geometry(viewpoint_camera, pc, pipe, bg_color=None, *, options=None, geometry_grad=True, distortion=False):
    """The geometry maps of one view from ONE forward: the four columns of normals.gaussian_normals -- the view-space normal of every
    Gaussian (the axis of its smallest scale, facing the camera) and its view-space z -- blended with the view's weights in one
    blend_features call.

    Returns {"render" [3,H,W], "alpha" [H,W], "normal" [3,H,W] (blended, unnormalised: its length is about alpha), "depth" [H,W]
    (= blended z / alpha.clamp_min(1e-6), the expected depth render_features("depth") gives), "radii", "visibility_filter",
    "viewspace_points" (None without geometry_grad)}.  normal, depth and alpha are what normals.normal_consistency_loss takes.

    geometry_grad=True (default): every map is differentiable with respect to the model -- the normals reach _rotation and, through
    z, _xyz directly (lg_normal_rows_bwd), and everything reaches _xyz, _opacity, _scaling, _rotation through the blend
    (lg_backward_features).  The same models are accepted and refused as by render_features(geometry_grad=True); filter_3D and
    antialiasing apply through the same options.  pipe.compute_cov3D_python hands the renderer no scales and rotations: refused.

    distortion=True: the result gains "distortion" [H,W], the depth distortion sum_{i<j} w_i w_j (z_i - z_j)^2 over the view-space z (column
    3 of the rows), and "median_depth" [H,W], the z of the Gaussian that carries the transmittance across one half
    (lightgaussian_amd.distortion.blend_geometry: the same forward, one more walk of the tile lists; with geometry_grad=True both are
    differentiable and the one backward, lg_backward_distortion, serves every map).  False is the path above, unchanged."""
    from .features import blend_features
    from .normals import gaussian_normals
    options = _pipe_options(pipe, options)
    if _camera_grad(options):
        raise NotImplementedError("camera_grad is not implemented for render_geometry: use render() for the pose gradient")
    if isinstance(pc, (CompressedGaussians, TrainableCompressed)):
        if geometry_grad:
            raise NotImplementedError("render_geometry(geometry_grad=True) needs the dense tensors: pass pc.to_dense() instead")
        raise NotImplementedError("render_geometry needs the dense scales and rotations: pass pc.to_dense() instead")
    if pipe.compute_cov3D_python:
        raise NotImplementedError("render_geometry needs scales and rotations: compute_cov3D_python hands the renderer covariances only")
    with contextlib.nullcontext() if geometry_grad else torch.no_grad():
        means3D, opacity, scales, rotations, cov3D_precomp, shs, colors_precomp = _inputs(viewpoint_camera, pc, pipe, 1.0, None, options)
        if bg_color is None:
            bg_color = torch.zeros(3, dtype=torch.float32, device=means3D.device)
        rows = gaussian_normals(means3D.contiguous(), scales.contiguous(), rotations.contiguous(), viewpoint_camera)
    rs = _settings(viewpoint_camera, pc, pipe, bg_color, 1.0, False)
    screenspace_points = _screenspace_points(pc) if geometry_grad else None
    extra = {}
    if distortion:
        from .distortion import blend_geometry
        with contextlib.nullcontext() if geometry_grad else torch.no_grad():
            image, alpha, color, radii, dist, median = blend_geometry(rs, rows, m_column=3, means3D=means3D, opacities=opacity, scales=scales,
                                                                      rotations=rotations, cov3D_precomp=cov3D_precomp, shs=shs,
                                                                      colors_precomp=colors_precomp, options=options, means2D=screenspace_points)
        extra = {"distortion": dist, "median_depth": median}
    else:
        image, alpha, color, radii = blend_features(rs, rows, means3D=means3D, opacities=opacity, scales=scales, rotations=rotations,
                                                    cov3D_precomp=cov3D_precomp, shs=shs, colors_precomp=colors_precomp, options=options,
                                                    geometry_grad=geometry_grad, means2D=screenspace_points)
    return {"render": color, "alpha": alpha, "normal": image[:3], "depth": image[3] / alpha.clamp_min(_DEPTH_EPS), "radii": radii,
            "visibility_filter": radii > 0, "viewspace_points": screenspace_points, **extra}
