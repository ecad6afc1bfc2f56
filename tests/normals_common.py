"""Shared by tests/test_normals_host.py and tests/test_gpu_normals.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_normals_harness.cpp, the inputs, and the float64 twin of the contract of DESIGN section 10.11.

Rows.  rows_inputs(): positions in a box the cameras look at, log-scales uniform in [-5, 0], quaternions randn times exp(U(-2, 2))
(unnormalised).  rows_twin() is the contract in torch, any dtype, differentiable; in float64 it also returns the two decision margins:
the gap between the two smallest scales and |n . p| / |p|.  keep_rows() drops the rows within 1e-4 of either decision, so the float64
twin decides k and s with a margin thousands of times the float32 error and the comparisons exclude no kept row.
Bounds of the float32 rows against the float64 twin (u = 2^-24):  normal: q^ carries 3 u per component, an entry of R(q^) at most
20 u, a view-space component sums three of them against |vm| <= 1 and rounds three times: 64 u absolute.  z: 4 u (|xyz| . |vm[:3, 2]| +
|vm[3, 2]|), the bound of three products and three sums.

Images.  depth_maps(): a noisy depth uniform in [2, 6] and a tilted plane plus noise.  depth_normals_twin() / loss_twin(): the contract
in torch, any dtype, differentiable.  On these inputs min |c| is above 2.5 % of the median |c| and nothing is near the 1e-12 clamp, so
the float32 formula stays within 5e-6 of the float64 one (N_D_TOL) and rule 3 (tests/tolerance.py) applies to the gradients."""
import ctypes as C
import math

import numpy as np
import torch

import common
import tolerance
from common import f32, ptr, syn  # noqa: F401

NS = (1, 3, 4, 5, 63, 64, 65, 257)
FWD_COLS, BWD_COLS, ROWS = 62, 60, 32           # LG_NRM_FWD_COLS, LG_NRM_BWD_COLS, LG_NRM_ROWS of lg_normals.h
# W x H: the issue's five, then one pixel either side of both strip widths and of the rows per wave
SIZES = ((1, 1), (2, 2), (3, 3), (33, 17), (70, 45), (61, 31), (63, 33), (59, 31), (61, 33))
U = 2.0 ** -24
NORMAL_BOUND = 64 * U
N_D_TOL = 5e-6
MARGIN = 1e-4
TANFOV = (0.5773502691896257, 0.3247595264191645)      # tan(30 deg), and the same times 9 / 16


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("normals", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_normal_rows": (None, [I, P, P, P, P, P, P, P]), "h_normal_rows_bwd": (None, [I, P, P, P, P, P, P, P]),
        "h_depth_normals": (None, [I, I, P, F, F, P]), "h_depth_normals_bwd": (None, [I, I, P, F, F, P, P]),
        "h_normal_loss": (C.c_double, [I, I, P, P, P, P, F, F]), "h_normal_loss_bwd": (None, [I, I, P, P, P, P, F, F, F, P, P])})


# ---- rows ---------------------------------------------------------------------------------------------------------------------
def cameras(W=70, H=45):
    return [syn.orbit_camera(1, 7, W, H, radius=4.0), syn.orbit_camera(4, 7, W, H, radius=6.0, height_y=-1.5)]


def view_matrix(cam):
    return np.ascontiguousarray(cam.world_view_transform.numpy(), np.float32)


def rows_inputs(N, seed=0):
    rs = np.random.RandomState(1000 * seed + N)
    xyz = (rs.uniform(-1.5, 1.5, (N, 3)) * np.array([1.0, 0.7, 1.0])).astype(np.float32)
    sc = rs.uniform(-5.0, 0.0, (N, 3)).astype(np.float32)
    q = (rs.randn(N, 4) * np.exp(rs.uniform(-2.0, 2.0, (N, 1)))).astype(np.float32)
    return xyz, sc, q


def rotation_of_unit(q):
    r, x, y, z = q.unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def rows_twin(xyz, sc, q, vm, k=None, s=None):
    """(rows [N,4], k, s, scale gap, |n . p| / |p|) of torch tensors of one dtype; k and s given: held at those values."""
    qh = q / torch.sqrt((q * q).sum(dim=1, keepdim=True)).clamp_min(1e-12)
    R = rotation_of_unit(qh)
    srt = torch.sort(sc.detach(), dim=1).values
    if k is None:
        k = torch.argmin(sc.detach(), dim=1)
    n_w = R[torch.arange(R.shape[0]), :, k]
    n_v = n_w @ vm[:3, :3]
    p_v = xyz @ vm[:3, :3] + vm[3, :3]
    dot = (n_v * p_v).sum(dim=1).detach()
    if s is None:
        s = torch.where(dot > 0, -1.0, 1.0).to(xyz.dtype)
    rows = torch.cat([s[:, None] * n_v, p_v[:, 2:3]], dim=1)
    return rows, k, s, srt[:, 1] - srt[:, 0], dot.abs() / p_v.detach().norm(dim=1).clamp_min(1e-30)


def t64(*arrays):
    return [torch.from_numpy(np.asarray(a, np.float64).copy()) for a in arrays]


def keep_rows(xyz, sc, q, vm):
    """The float64 twin's (rows, k, s) and the mask of the rows outside both decision margins."""
    rows, k, s, gap, ndp = rows_twin(*t64(xyz, sc, q, vm))
    keep = (gap >= MARGIN) & (ndp >= MARGIN)
    return rows.numpy(), k.numpy(), s.numpy(), keep.numpy()


def z_bound(xyz, vm):
    return 4 * U * (np.abs(np.asarray(xyz, np.float64)) @ np.abs(np.asarray(vm, np.float64)[:3, 2]) + abs(float(vm[3, 2])))


def harness_rows(xyz, sc, q, vm):
    N = xyz.shape[0]
    rows, axis, sign = np.zeros((N, 4), np.float32), np.zeros(N, np.int32), np.zeros(N, np.float32)
    harness().h_normal_rows(N, ptr(f32(xyz)), ptr(f32(sc)), ptr(f32(q)), ptr(f32(vm)), ptr(rows), ptr(axis), ptr(sign))
    return rows, axis, sign


def harness_rows_bwd(xyz, sc, q, vm, g):
    N = xyz.shape[0]
    d_xyz, d_rot = np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32)
    harness().h_normal_rows_bwd(N, ptr(f32(xyz)), ptr(f32(sc)), ptr(f32(q)), ptr(f32(vm)), ptr(f32(g)), ptr(d_xyz), ptr(d_rot))
    return d_xyz, d_rot


_ROWS_REF = {}


def rows_grad_reference(N, cam_index):
    """{"float64" / "float32": (d_xyz, d_rotation)} of sum(rows g) by autograd through rows_twin, k and s held at the float64 twin's; plus
    the inputs.  Computed once per key."""
    key = (N, cam_index)
    if key not in _ROWS_REF:
        xyz, sc, q = rows_inputs(N, seed=2)
        vm = view_matrix(cameras()[cam_index])
        g = np.random.RandomState(7 + N).randn(N, 4).astype(np.float32)
        _rows, k, s, _gap, _ndp = rows_twin(*t64(xyz, sc, q, vm))
        out = dict(inputs=(xyz, sc, q, vm, g))
        for dd, name in ((torch.float64, "float64"), (torch.float32, "float32")):
            x, r = torch.from_numpy(xyz).to(dd).requires_grad_(), torch.from_numpy(q).to(dd).requires_grad_()
            rows = rows_twin(x, torch.from_numpy(sc).to(dd), r, torch.from_numpy(vm).to(dd), k=k, s=s.to(dd))[0]
            (rows * torch.from_numpy(g).to(dd)).sum().backward()
            out[name] = (x.grad.numpy().astype(np.float64), r.grad.numpy().astype(np.float64))
        _ROWS_REF[key] = out
    return _ROWS_REF[key]


# ---- images -------------------------------------------------------------------------------------------------------------------
def depth_maps(W, H):
    """{"noisy": uniform in [2, 6], "plane": a tilted plane plus noise}: float32 [H, W]."""
    rs = np.random.RandomState(31 * W + H)
    ys, xs = np.mgrid[0:H, 0:W]
    plane = 3.0 + 0.02 * xs - 0.015 * ys + 0.01 * rs.randn(H, W)
    return {"noisy": rs.uniform(2.0, 6.0, (H, W)).astype(np.float32), "plane": plane.astype(np.float32)}


def loss_maps(W, H):
    """N_r [3,H,W] (unit-ish, random), alpha in [0, 1], weight in [0, 1], dL/dN_d [3,H,W]: float32."""
    rs = np.random.RandomState(17 * W + H)
    return (rs.randn(3, H, W).astype(np.float32), rs.uniform(0.0, 1.0, (H, W)).astype(np.float32), rs.uniform(0.0, 1.0, (H, W)).astype(np.float32),
            rs.randn(3, H, W).astype(np.float32))


def cross_products(depth, tx, ty):
    """The interior cross products c [3, H-2, W-2] of the contract, dtype of depth."""
    H, W = depth.shape
    dd = depth.dtype
    rx = ((2 * torch.arange(W, dtype=dd) + 1) / W - 1) * tx
    ry = ((2 * torch.arange(H, dtype=dd) + 1) / H - 1) * ty
    P = torch.stack([depth * rx[None, :], depth * ry[:, None], depth], dim=0)
    return torch.cross(P[:, 2:, 1:-1] - P[:, :-2, 1:-1], P[:, 1:-1, 2:] - P[:, 1:-1, :-2], dim=0)


def depth_normals_twin(depth, tx, ty):
    """N_d [3,H,W] of a FINITE depth map, dtype of depth, differentiable."""
    H, W = depth.shape
    if H < 3 or W < 3:
        return torch.zeros((3, H, W), dtype=depth.dtype) + 0 * depth.sum()
    c = cross_products(depth, tx, ty)
    return torch.nn.functional.pad(c / c.norm(dim=0, keepdim=True).clamp_min(1e-12), (1, 1, 1, 1))


def loss_twin(nr, depth, alpha, weight, tx, ty):
    w = alpha if weight is None else alpha * weight
    return (1 - w.detach() * (nr * depth_normals_twin(depth, tx, ty)).sum(dim=0)).mean()


G_LOSS = 1.7            # the upstream scalar gradient of the loss in every backward test

_IMG_REF = {}


def image_reference(W, H, kind, weighted=True):
    """Per dtype name: {"nd", "d_depth_plain" (of sum(N_d g)), "loss", "d_nr", "d_depth" (of G_LOSS * loss)} as float64 arrays, by autograd
    through the twins; plus "inputs" = (depth, nr, alpha, weight or None, g).  Computed once per key."""
    key = (W, H, kind, weighted)
    if key not in _IMG_REF:
        depth = depth_maps(W, H)[kind]
        nr, alpha, weight, g = loss_maps(W, H)
        if not weighted:
            weight = None
        out = dict(inputs=(depth, nr, alpha, weight, g))
        for dd, name in ((torch.float64, "float64"), (torch.float32, "float32")):
            to = lambda a: None if a is None else torch.from_numpy(a).to(dd)  # noqa: E731
            d = to(depth).requires_grad_()
            nd = depth_normals_twin(d, *TANFOV)
            (nd * to(g)).sum().backward()
            plain = d.grad.numpy().astype(np.float64)
            d2, n2 = to(depth).requires_grad_(), to(nr).requires_grad_()
            loss = loss_twin(n2, d2, to(alpha), to(weight), *TANFOV)
            (G_LOSS * loss).backward()
            out[name] = dict(nd=nd.detach().numpy().astype(np.float64), d_depth_plain=plain, loss=float(loss.detach()), d_nr=n2.grad.numpy().astype(np.float64),
                             d_depth=d2.grad.numpy().astype(np.float64))
        _IMG_REF[key] = out
    return _IMG_REF[key]


def harness_depth_normals(depth):
    H, W = depth.shape
    nd = np.zeros((3, H, W), np.float32)
    harness().h_depth_normals(H, W, ptr(f32(depth)), TANFOV[0], TANFOV[1], ptr(nd))
    return nd


def harness_depth_normals_bwd(depth, g):
    H, W = depth.shape
    d = np.zeros((H, W), np.float32)
    harness().h_depth_normals_bwd(H, W, ptr(f32(depth)), TANFOV[0], TANFOV[1], ptr(f32(g)), ptr(d))
    return d


def harness_loss(nr, depth, alpha, weight):
    H, W = depth.shape
    return harness().h_normal_loss(H, W, ptr(f32(nr)), ptr(f32(depth)), ptr(f32(alpha)), ptr(f32(weight)), TANFOV[0], TANFOV[1])


def harness_loss_bwd(nr, depth, alpha, weight, g_loss=G_LOSS):
    H, W = depth.shape
    d_nr, d_depth = np.zeros((3, H, W), np.float32), np.zeros((H, W), np.float32)
    harness().h_normal_loss_bwd(H, W, ptr(f32(nr)), ptr(f32(depth)), ptr(f32(alpha)), ptr(f32(weight)), TANFOV[0], TANFOV[1], g_loss, ptr(d_nr), ptr(d_depth))
    return d_nr, d_depth


def assert_image_gradients(got, ref, what, names):
    """Rule 3 per tensor for sizes with an interior; exact zeros where the image has none (every pixel a border pixel)."""
    for n in names:
        r64 = ref["float64"][n]
        if not np.asarray(r64).any():
            assert not np.asarray(got[n]).any(), f"{what} {n}: must be exact zeros"
            continue
        tolerance.assert_rule3(got[n], r64, ref["float32"][n], f"{what} {n}")


class Camera:
    """What normals.depth_to_normal / normal_consistency_loss read of a camera, with TANFOV's field of view."""
    FoVx, FoVy = 2 * math.atan(TANFOV[0]), 2 * math.atan(TANFOV[1])
