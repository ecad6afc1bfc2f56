"""Normals of the Gaussians, normals of a rendered depth map and the depth-normal consistency loss (2DGS, GOF, PGSR, RaDe-GS).

    gaussian_normals(xyz, scaling, rotation, camera, backend="hip")                      -> rows [N, 4]
        per Gaussian the view-space normal (columns 0..2: the axis of the smallest scale, turned to face the camera) and the
        view-space z (column 3): ONE lg_normal_rows launch; the backward (lg_normal_rows_bwd) reaches rotation and xyz.
    depth_to_normal(depth, camera, backend="hip")                                        -> N_d [3, H, W]
        the normal of the depth surface by finite differences of the un-projected points (2DGS's depth_to_normal); lg_depth_normals
        and its backward to depth.
    normal_consistency_loss(normal_map, depth, alpha, camera, weight=None, backend="hip") -> scalar
        mean_p (1 - w_p N_r(p) . N_d(p)), w = alpha or alpha * weight, a constant of the loss: lg_normal_loss (one pass and a reduce)
        and lg_normal_loss_bwd (one pass: dL/dN_r and, through the stencil, dL/ddepth).  alpha and weight receive no gradient.

gaussian_renderer.render_geometry blends the four columns of gaussian_normals in one forward and hands back normal, depth and alpha.

The contract (include/lightgaussian_normals.h), in float32:
    q^ = q / max(|q|, 1e-12)    R = R(q^)    k = argmin scaling (ties: lowest index)    n_w = column k of R
    n_v = n_w vm[:3, :3]        p_v = xyz vm[:3, :3] + vm[3, :3]        s = -1 where n_v . p_v > 0 else +1       rows = (s n_v, p_v.z)
    P(x, y) = depth(x, y) (((2x + 1) / W - 1) tanfovx, ((2y + 1) / H - 1) tanfovy, 1)
    c = (P(x, y+1) - P(x, y-1)) x (P(x+1, y) - P(x-1, y))        N_d = c / max(|c|, 1e-12)
scaling may be raw log-scales, activated or 3D-filtered scales (the same argmin); it receives no gradient, k and s are constants of the
backward.  The first and last row and column of N_d are zero, and so is a pixel whose own or neighbour depth is not finite; neither passes a
gradient.  Every sum runs in a fixed order: two calls give the same bits, on any stream.

backend="torch" is the same contract as a plain torch op sequence: the path CPU tensors take, and the comparand of
tools/normals_bench.py.  backend="hip" takes contiguous float32 tensors on the GPU and raises for anything else on the GPU.
set_profile(True) records the launches under "normal_rows", "normal_rows_bwd", "depth_normals", "depth_normals_bwd", "normal_loss",
"normal_loss_reduce", "normal_loss_bwd" (_lib.profile_read)."""
import ctypes as C
import math

import torch

from . import _lib, model_rows
from .model_rows import check_backend

EPS = 1e-12
MAX_ROWS = 1 << 30
MAX_DIM = 32768

# The C ABI of include/lightgaussian_normals.h, in header order: name -> (restype, argtypes).  tests/test_normals_host.py holds every
# entry against the header.
i32, u32, f32, sz, vp = C.c_int32, C.c_uint32, C.c_float, C.c_size_t, C.c_void_p
PROTOTYPES = {
    "lg_normal_rows": (C.c_int, (i32, vp, vp, vp, vp, vp, u32, vp)),
    "lg_normal_rows_bwd": (C.c_int, (i32, vp, vp, vp, vp, vp, vp, vp, u32, vp)),
    "lg_depth_normals": (C.c_int, (i32, i32, vp, f32, f32, vp, u32, vp)),
    "lg_depth_normals_bwd": (C.c_int, (i32, i32, vp, f32, f32, vp, vp, u32, vp)),
    "lg_normal_loss_scratch_bytes": (sz, (i32, i32)),
    "lg_normal_loss": (C.c_int, (i32, i32, vp, vp, vp, vp, f32, f32, vp, vp, vp, u32, vp)),
    "lg_normal_loss_bwd": (C.c_int, (i32, i32, vp, vp, vp, vp, f32, f32, vp, vp, vp, u32, vp)),
}

set_profile, _flags = model_rows.profile_switch()
def load():
    """The library object of _lib.load() with the prototypes of include/lightgaussian_normals.h set on it."""
    return _lib.bind(_lib.load(), PROTOTYPES)


def tanfov(camera):
    """(tanfovx, tanfovy) of a camera, as the renderer evaluates them."""
    return math.tan(camera.FoVx * 0.5), math.tan(camera.FoVy * 0.5)


# ---- argument checks --------------------------------------------------------------------------------------------------------------

def _check(what, name, t, shape, like=None):
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: {name} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, not {t.dtype}")
    if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{what}: {name} must have shape {list(shape)}, not {list(t.shape)}")
    if like is not None and t.device != like.device:
        raise ValueError(f"{what}: {name} is on {t.device}, not on {like.device}")


def _resolve(what, backend, tensors):
    """The backend a call takes: CPU tensors take the torch path; on the GPU backend="hip" asks for contiguous tensors."""
    check_backend(backend, what)
    if backend == "hip" and not tensors[0][1].is_cuda:
        return "torch"
    if backend == "hip":
        for name, t in tensors:
            if not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous for backend='hip' (call .contiguous())")
    return backend


def _grad(g, like):
    return torch.zeros_like(like) if g is None else g.contiguous()


# ---- per Gaussian -----------------------------------------------------------------------------------------------------------------

def _rotation_of_unit(q):
    r, x, y, z = q.unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def _rows_torch(xyz, scaling, rotation, vm):
    R = _rotation_of_unit(torch.nn.functional.normalize(rotation, dim=1, eps=EPS))
    k = torch.argmin(scaling.detach(), dim=1)                                       # (the first of equal minima)
    n_w = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1)).squeeze(2)         # column k
    n_v = n_w @ vm[:3, :3]
    p_v = xyz @ vm[:3, :3] + vm[3, :3]
    s = torch.where((n_v.detach() * p_v.detach()).sum(dim=1, keepdim=True) > 0, -1.0, 1.0).to(xyz.dtype)
    return torch.cat([s * n_v, p_v[:, 2:3]], dim=1)


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, scaling, rotation, vm):
        dev, n = xyz.device, int(xyz.shape[0])
        rows = torch.empty((n, 4), dtype=torch.float32, device=dev)
        xyz, scaling, rotation = xyz.detach(), scaling.detach(), rotation.detach()
        if n > 0:
            with torch.cuda.device(dev):
                _lib.check(load().lg_normal_rows(n, _lib.ptr(xyz), _lib.ptr(scaling), _lib.ptr(rotation), _lib.ptr(vm), _lib.ptr(rows), _flags(),
                                                 _lib.stream(dev)))
        ctx.save_for_backward(xyz, scaling, rotation, vm)
        return rows

    @staticmethod
    def backward(ctx, g):
        xyz, scaling, rotation, vm = ctx.saved_tensors
        dev, n = xyz.device, int(xyz.shape[0])
        d_xyz, d_rot = torch.empty_like(xyz), torch.empty_like(rotation)
        if n > 0:
            g = _grad(g, xyz.new_empty((n, 4)))
            with torch.cuda.device(dev):
                _lib.check(load().lg_normal_rows_bwd(n, _lib.ptr(xyz), _lib.ptr(scaling), _lib.ptr(rotation), _lib.ptr(vm), _lib.ptr(g), _lib.ptr(d_xyz),
                                                     _lib.ptr(d_rot), _flags(), _lib.stream(dev)))
        return d_xyz, None, d_rot, None


def gaussian_normals(xyz, scaling, rotation, camera, backend="hip"):
    """rows [N, 4] = (view-space normal, view-space z) of every Gaussian under `camera` (its world_view_transform), by the contract in
    the module docstring.  xyz [N, 3], scaling [N, 3] (raw, activated or filtered), rotation [N, 4] as (r, x, y, z), raw or normalised:
    float32.  Differentiable in xyz and rotation."""
    what = "gaussian_normals"
    _check(what, "xyz", xyz, (None, 3))
    n = int(xyz.shape[0])
    _check(what, "scaling", scaling, (n, 3), xyz)
    _check(what, "rotation", rotation, (n, 4), xyz)
    if n >= MAX_ROWS:
        raise ValueError(f"{what}: N >= 2^30")
    backend = _resolve(what, backend, (("xyz", xyz), ("scaling", scaling), ("rotation", rotation)))
    vm = camera.world_view_transform.detach().to(device=xyz.device, dtype=torch.float32)
    if tuple(vm.shape) != (4, 4):
        raise ValueError(f"{what}: camera.world_view_transform must be [4, 4]")
    if backend == "torch":
        return _rows_torch(xyz, scaling, rotation, vm)
    return _GaussianNormals.apply(xyz, scaling, rotation, vm.contiguous())


# ---- per pixel --------------------------------------------------------------------------------------------------------------------

def _depth_normals_torch(depth, tx, ty):
    H, W = depth.shape
    dt, dev = depth.dtype, depth.device
    finite = torch.isfinite(depth)
    d = torch.where(finite, depth, torch.zeros_like(depth))                         # a non-finite depth takes no gradient
    if H < 3 or W < 3:                                                              # border pixels only: zeros (attached, with a zero gradient)
        return torch.zeros((3, H, W), dtype=dt, device=dev) + 0 * d.sum()
    rx = ((2 * torch.arange(W, dtype=dt, device=dev) + 1) / W - 1) * tx
    ry = ((2 * torch.arange(H, dtype=dt, device=dev) + 1) / H - 1) * ty
    P = torch.stack([d * rx[None, :], d * ry[:, None], d], dim=0)
    a = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    b = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    c = torch.cross(a, b, dim=0)
    ok = (finite[1:-1, 1:-1] & finite[2:, 1:-1] & finite[:-2, 1:-1] & finite[1:-1, 2:] & finite[1:-1, :-2] & torch.isfinite(c).all(dim=0))[None]
    c = torch.where(ok, c, torch.zeros_like(c))
    n = c / c.norm(dim=0, keepdim=True).clamp_min(EPS)
    return torch.nn.functional.pad(n, (1, 1, 1, 1))


def _loss_torch(normal_map, depth, w, tx, ty):
    return (1 - w.detach() * (normal_map * _depth_normals_torch(depth, tx, ty)).sum(dim=0)).mean()


class _DepthToNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, tx, ty):
        H, W = depth.shape
        dev = depth.device
        depth = depth.detach()
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(load().lg_depth_normals(H, W, _lib.ptr(depth), tx, ty, _lib.ptr(out), _flags(), _lib.stream(dev)))
        ctx.save_for_backward(depth)
        ctx.tan = (tx, ty)
        return out

    @staticmethod
    def backward(ctx, g):
        (depth,) = ctx.saved_tensors
        H, W = depth.shape
        dev = depth.device
        g = _grad(g, depth.new_empty((3, H, W)))
        d_depth = torch.empty_like(depth)
        with torch.cuda.device(dev):
            _lib.check(load().lg_depth_normals_bwd(H, W, _lib.ptr(depth), ctx.tan[0], ctx.tan[1], _lib.ptr(g), _lib.ptr(d_depth), _flags(),
                                                   _lib.stream(dev)))
        return d_depth, None, None


def _check_image(what, depth):
    _check(what, "depth", depth, (None, None))
    H, W = (int(v) for v in depth.shape)
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"{what}: H and W must lie in [1, {MAX_DIM}], not {H} x {W}")
    return H, W


def depth_to_normal(depth, camera, backend="hip"):
    """N_d [3, H, W] of a depth map [H, W] (float32) under `camera` (its FoVx, FoVy), by the contract in the module docstring.
    Differentiable in depth."""
    what = "depth_to_normal"
    _check_image(what, depth)
    backend = _resolve(what, backend, (("depth", depth),))
    tx, ty = tanfov(camera)
    if backend == "torch":
        return _depth_normals_torch(depth, tx, ty)
    return _DepthToNormal.apply(depth, tx, ty)


class _NormalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal_map, depth, alpha, weight, tx, ty):
        H, W = depth.shape
        dev = depth.device
        lib = load()
        normal_map, depth, alpha = normal_map.detach(), depth.detach(), alpha.detach()
        weight = None if weight is None else weight.detach()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            scratch = _lib.scratch(lib.lg_normal_loss_scratch_bytes(H, W), dev)
            _lib.check(lib.lg_normal_loss(H, W, _lib.ptr(normal_map), _lib.ptr(depth), _lib.ptr(alpha), _lib.ptr(weight), tx, ty, _lib.ptr(loss), None,
                                          _lib.ptr(scratch), _flags(), _lib.stream(dev)))
        ctx.save_for_backward(normal_map, depth, alpha, *(() if weight is None else (weight,)))
        ctx.tan = (tx, ty)
        return loss

    @staticmethod
    def backward(ctx, g):
        normal_map, depth, alpha, *rest = ctx.saved_tensors
        weight = rest[0] if rest else None
        H, W = depth.shape
        dev = depth.device
        g = g.to(torch.float32).contiguous()                    # stays on the device: the kernel reads it there
        d_nr, d_depth = torch.empty_like(normal_map), torch.empty_like(depth)
        with torch.cuda.device(dev):
            _lib.check(load().lg_normal_loss_bwd(H, W, _lib.ptr(normal_map), _lib.ptr(depth), _lib.ptr(alpha), _lib.ptr(weight), ctx.tan[0], ctx.tan[1],
                                                 _lib.ptr(g), _lib.ptr(d_nr), _lib.ptr(d_depth), _flags(), _lib.stream(dev)))
        return d_nr, d_depth, None, None, None, None


def normal_consistency_loss(normal_map, depth, alpha, camera, weight=None, backend="hip"):
    """mean_p (1 - w_p N_r(p) . N_d(p)): normal_map = N_r [3, H, W] (the blended, unnormalised normals), depth [H, W], alpha [H, W],
    weight [H, W] or None, all float32; w = alpha (* weight), a constant.  A 0-dim tensor, differentiable in normal_map and depth."""
    what = "normal_consistency_loss"
    H, W = _check_image(what, depth)
    _check(what, "normal_map", normal_map, (3, H, W), depth)
    _check(what, "alpha", alpha, (H, W), depth)
    tensors = [("normal_map", normal_map), ("depth", depth), ("alpha", alpha)]
    if weight is not None:
        _check(what, "weight", weight, (H, W), depth)
        tensors.append(("weight", weight))
    backend = _resolve(what, backend, tensors)
    tx, ty = tanfov(camera)
    if backend == "torch":
        return _loss_torch(normal_map, depth, alpha if weight is None else alpha * weight, tx, ty)
    return _NormalLoss.apply(normal_map, depth, alpha, weight, tx, ty)
