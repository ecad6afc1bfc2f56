"""Mip-Splatting's 3D smoothing filter: the other half of the `antialiasing` / `filter_3D` switch pair.

    compute_filter_3d(xyz, cameras)       the per-Gaussian filter size from the training cameras (lg_filter3d_update: one pass over the
                                          Gaussians, every camera visited in registers) -- upstream's compute_3D_filter, [N, 1];
    apply_filter_3d(_scaling, _opacity, f)            raw -> raw: log-scales and opacity logits with the filter applied, in the domain
                                                      LG_FLAG_RAW_PARAMS reads, so the fused render path stays (lg_filter3d_apply);
    apply_filter_3d_activated(scales, opacity, f)     the same on activated values (upstream's get_scaling_with_3D_filter /
                                                      get_opacity_with_3D_filter), for the unfused path and foreign getters;
    fuse_filter_3d(model)                 the raw tensors with the filter baked in: upstream's save_fused_ply semantics.

A trainer keeps `gaussians.filter_3D = compute_filter_3d(gaussians.get_xyz, train_cameras)` up to date (every 100 iterations and after
every densification or prune: the filter has one row per Gaussian); gaussian_renderer.render / count_render / render_features honour the
attribute (rasterizer option "filter_3d", default True).  All arithmetic runs in liblightgaussian_hip.so; there is no torch fallback.

With t_n = z_n / fx_n the world size of one pixel of camera n at the Gaussian, the filter is sqrt(0.2) min over the cameras that see it
of t_n: the paper's maximal sampling rate.  With cameras that share one focal length this equals the published code's
sqrt(0.2) * min depth / max focal."""
import ctypes as C
import math

import torch

from . import _lib
from .rasterizer import _prep, option_value


def camera_table(cameras):
    """The lg_filter_camera table of `cameras` (objects with world_view_transform, FoVx, FoVy, image_width, image_height, as the
    reference's Camera / MiniCam) as a CPU uint8 tensor [V, 80], built on the host."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("compute_filter_3d needs at least one camera")
    vms = torch.stack([c.world_view_transform.detach() for c in cameras]).to(device="cpu", dtype=torch.float32).reshape(len(cameras), 16)
    table = (_lib.lg_filter_camera * len(cameras))()
    for k, c in enumerate(cameras):
        table[k].viewmatrix[:] = vms[k].tolist()
        table[k].tanfovx, table[k].tanfovy = math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5)
        table[k].width, table[k].height = int(c.image_width), int(c.image_height)
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).reshape(len(cameras), C.sizeof(_lib.lg_filter_camera))


def compute_filter_3d(xyz, cameras, *, return_seen=False):
    """filter_3D [N, 1] float32 of the means `xyz` [N, 3] under `cameras` (upstream Mip-Splatting's compute_3D_filter; the [N, 1] shape
    is upstream's).  A Gaussian no camera sees gets the largest value of the seen ones; if none is seen at all every value is 0.
    cameras: a sequence of camera objects, or a uint8 [V, 80] table from camera_table() (any device) to reuse across calls.
    return_seen: also return the bool [N] mask of the Gaussians at least one camera sees."""
    lib = _lib.load()
    dev = xyz.device
    if dev.type != "cuda":
        raise RuntimeError("compute_filter_3d needs the means on a HIP device (torch 'cuda'); there is no CPU path")
    table = cameras if torch.is_tensor(cameras) else camera_table(cameras)
    if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != C.sizeof(_lib.lg_filter_camera) or table.shape[0] < 1:
        raise ValueError("cameras: a sequence of cameras or a uint8 [V, 80] table from camera_table()")
    table = table.to(dev).contiguous()
    means = _prep(xyz.detach(), dev)
    N = int(xyz.shape[0])
    out = torch.empty((N, 1), dtype=torch.float32, device=dev)
    seen = torch.empty((N,), dtype=torch.uint8, device=dev) if return_seen else None
    if N > 0:
        with torch.cuda.device(dev):
            scratch = _lib.scratch(lib.lg_filter3d_scratch_bytes(N), dev)
            flags = _lib.profile_flag(option_value("profile"))
            _lib.check(lib.lg_filter3d_update(N, _lib.ptr(means), int(table.shape[0]), _lib.ptr(table), _lib.ptr(out), _lib.ptr(seen),
                                              _lib.ptr(scratch), flags, _lib.stream()))
    return (out, seen.view(torch.bool)) if return_seen else out


class _ApplyFilter3D(torch.autograd.Function):
    """lg_filter3d_apply / lg_filter3d_apply_bwd, in the raw (log-scale, logit) or the activated domain.  The filter gets no gradient."""

    @staticmethod
    def forward(ctx, scaling, opacity, filter_3d, raw):
        lib = _lib.load()
        dev = scaling.device
        if dev.type != "cuda":
            raise RuntimeError("the 3D filter is applied on a HIP device (torch 'cuda'); there is no CPU path")
        N = int(scaling.shape[0])
        if scaling.shape != (N, 3) or opacity.numel() != N or filter_3d.numel() != N:
            raise ValueError(f"apply_filter_3d: scaling [N, 3], opacity [N, 1] and filter_3d [N, 1] must agree in N "
                             f"(got {tuple(scaling.shape)}, {tuple(opacity.shape)}, {tuple(filter_3d.shape)})")
        f32 = dict(dtype=torch.float32, device=dev)
        out_s, out_o = torch.empty((N, 3), **f32), torch.empty(opacity.shape, **f32)
        ctx.flags = (_lib.FILTER3D_RAW if raw else 0) | _lib.profile_flag(option_value("profile"))
        ctx.opacity_shape = tuple(opacity.shape)
        ctx.set_materialize_grads(False)
        if N == 0:                      # (an empty model: nothing to launch, nothing to save)
            return out_s, out_o
        s, o, f = _prep(scaling.detach(), dev), _prep(opacity.detach(), dev), _prep(filter_3d.detach(), dev)
        with torch.cuda.device(dev):
            _lib.check(lib.lg_filter3d_apply(N, _lib.ptr(s), _lib.ptr(o), _lib.ptr(f), _lib.ptr(out_s), _lib.ptr(out_o), ctx.flags,
                                             _lib.stream()))
        ctx.save_for_backward(s, o, f)
        return out_s, out_o

    @staticmethod
    def backward(ctx, g_s, g_o):
        if g_s is None and g_o is None:
            return None, None, None, None
        if not ctx.saved_tensors:
            dev = (g_s if g_s is not None else g_o).device
            return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros(ctx.opacity_shape, dtype=torch.float32, device=dev), None, None
        lib = _lib.load()
        s, o, f = ctx.saved_tensors
        dev, N = s.device, int(s.shape[0])
        f32 = dict(dtype=torch.float32, device=dev)
        g_s = torch.zeros((N, 3), **f32) if g_s is None else _prep(g_s, dev)
        g_o = torch.zeros(ctx.opacity_shape, **f32) if g_o is None else _prep(g_o, dev)
        d_s, d_o = torch.empty((N, 3), **f32), torch.empty(ctx.opacity_shape, **f32)
        with torch.cuda.device(dev):
            _lib.check(lib.lg_filter3d_apply_bwd(N, _lib.ptr(s), _lib.ptr(o), _lib.ptr(f), _lib.ptr(g_s), _lib.ptr(g_o), _lib.ptr(d_s),
                                                 _lib.ptr(d_o), ctx.flags, _lib.stream()))
        return d_s, d_o, None, None


def apply_filter_3d(scaling_raw, opacity_raw, filter_3d):
    """(log-scales', opacity logits') with the 3D filter applied, raw -> raw:  s'^2 = exp(r)^2 + f^2,  sigma' = sigmoid(o) c with
    c = sqrt(prod_k exp(r_k)^2 / s'_k^2).  Differentiable in the first two arguments; rows with f == 0 pass through bit for bit."""
    return _ApplyFilter3D.apply(scaling_raw, opacity_raw, filter_3d, True)


def apply_filter_3d_activated(scales, opacity, filter_3d):
    """(scales', opacity') = (sqrt(s^2 + f^2), sigma c) of ACTIVATED scales and opacities: upstream's get_scaling_with_3D_filter /
    get_opacity_with_3D_filter.  Differentiable in the first two arguments."""
    return _ApplyFilter3D.apply(scales, opacity, filter_3d, False)


def model_filter(pc, options=None):
    """`pc.filter_3D` when the model has one, it is not None and option "filter_3d" is on; None otherwise.  Raises ValueError for a
    filter whose row count is not the model's (after densify_and_prune / prune_points the filter must be recomputed)."""
    f = getattr(pc, "filter_3D", None)
    if f is None or not option_value("filter_3d", options):
        return None
    n = int(pc.get_xyz.shape[0])
    if f.dim() == 0 or int(f.shape[0]) != n or f.numel() != n:
        raise ValueError(f"filter_3D has shape {tuple(f.shape)} but the model has {n} Gaussians: recompute it with "
                         "filter3d.compute_filter_3d(pc.get_xyz, cameras) after every densification or prune")
    return f


def fuse_filter_3d(model):
    """(_scaling', _opacity') of `model` with its filter_3D baked in (raw -> raw, detached): a model that carries these in place of
    _scaling / _opacity and no filter renders, bit for bit, what `model` renders with the filter -- upstream's save_fused_ply.  The
    result can be exported by the reference's save_ply, pruned, VecTree-compressed and viewed anywhere without the filter."""
    f = getattr(model, "filter_3D", None)
    if f is None:
        raise ValueError("fuse_filter_3d: the model has no filter_3D (filter3d.compute_filter_3d)")
    if int(f.shape[0]) != int(model._scaling.shape[0]):
        raise ValueError(f"filter_3D has {int(f.shape[0])} rows but the model has {int(model._scaling.shape[0])} Gaussians: recompute it")
    with torch.no_grad():
        return apply_filter_3d(model._scaling, model._opacity, f)
