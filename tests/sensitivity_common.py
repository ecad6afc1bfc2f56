"""Shared by tests/test_sensitivity_host.py, tests/test_gpu_sensitivity.py and tests/golden/make_golden_sensitivity.py (test
infrastructure): the g++ build of tests/cpu_harness/lg_sensitivity_harness.cpp, the golden scene, the blocks of the dense twin
(J^T J of its float64 / float32 Jacobian) and the scaled comparison of 6 x 6 blocks."""
import ctypes as C
import math
import os

import numpy as np
import torch

import common
import dense_twin
from common import f32, ptr, syn

GOLDEN = os.path.join(common.ROOT, "tests", "golden", "sensitivity_blocks.npz")
GOLDEN_VIEWS = (0, 3)
GOLDEN_BG = (0.2, 0.3, 0.1)
IU = np.triu_indices(6)


def harness():
    P, F, I, D = C.c_void_p, C.c_float, C.c_int, C.c_double
    return common.build_harness("sensitivity", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_sens_ray": (I, [I, P, F, F, P, P, P]),
        "h_sens_block": (None, [P, F, F, F, F, P, P, P, P, P, I, I, F, F, P]),
        "h_sens_logdet": (D, [P]),
        "h_sens_view": (C.c_longlong, [I, I, I] + [P] * 8 + [F, F, P, P, P])})


def golden_scene():
    """(gaussians, colours [24,3], [camera of view k for k in GOLDEN_VIEWS]) of the golden scene, on the CPU."""
    g = syn.make_gaussians(24, sh_degree=0, seed=11, extent=(1.2, 1.2, 1.2), log_scale_mean=math.log(0.12), log_scale_std=0.4,
                           opacity_mean=0, opacity_std=1)
    colors = torch.rand(24, 3, generator=torch.Generator().manual_seed(3))
    cams = [syn.orbit_camera(k, 8, 32, 32, radius=6, fovx_deg=40) for k in GOLDEN_VIEWS]
    return g, colors, cams


BRUTE_SEED, BRUTE_N, BRUTE_PILE, BRUTE_W, BRUTE_H, BRUTE_VIEWS = 7, 200, 20, 40, 24, (0, 2)


def brute_scene(seed=BRUTE_SEED):
    """(gaussians, colours [200,3], cameras) of the brute-force scene at 40 x 24 (partial tiles): 180 Gaussians in a box the cameras look
    at -- lists longer than one 64-entry batch -- and a pile of 20 near-opaque splats in front of it, between the box and both cameras, so
    that rays end early.  Two views 90 degrees apart: a single view's blocks have rank 5 (their kappa is infinite).  Seeds 5, 6, 7 leave
    6.5 %, 7.5 % and 4 % of the blocks above kappa = 1e3 (CPU walk of tests/cpu_harness); at 45 degrees it is 14 .. 20 %."""
    g = syn.make_gaussians(BRUTE_N, sh_degree=0, seed=seed, extent=(0.9, 0.5, 0.9), log_scale_mean=math.log(0.12), log_scale_std=0.4,
                           opacity_mean=-0.5, opacity_std=1.0)
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        mid = math.pi * sum(BRUTE_VIEWS) / 8       # between the two cameras (view k of 8 stands at 2 pi k / 8)
        centre = 1.3 * torch.tensor([math.sin(mid), 0.0, -math.cos(mid)])
        g._xyz[-BRUTE_PILE:] = centre + 0.15 * torch.randn(BRUTE_PILE, 3, generator=gen)
        g._opacity[-BRUTE_PILE:] = 4.0
        g._scaling[-BRUTE_PILE:] = math.log(0.1) + 0.2 * torch.randn(BRUTE_PILE, 3, generator=gen)
    colors = torch.rand(BRUTE_N, 3, generator=gen)
    cams = [syn.orbit_camera(k, 8, BRUTE_W, BRUTE_H, radius=5, fovx_deg=40) for k in BRUTE_VIEWS]
    return g, colors, cams


def scene_kw(g, colors, cam, W, H, bg):
    with torch.no_grad():
        return common.scene_kwargs(g, cam, W, H, deg=0, precolor=colors, bg=bg, as_torch=True)


def full(tri):
    """[..., 21] upper triangles -> [..., 6, 6] symmetric blocks (numpy float64)."""
    tri = np.asarray(tri, np.float64)
    out = np.zeros(tri.shape[:-1] + (6, 6))
    out[..., IU[0], IU[1]] = tri
    out[..., IU[1], IU[0]] = tri
    return out


def tri(blocks):
    return np.asarray(blocks, np.float64)[..., IU[0], IU[1]]


def twin_blocks(kw, dd):
    """[N, 6, 6] float64: sum over pixels and channels of the outer product of the dense twin's Jacobian (evaluated in dtype dd, colours
    constant) with respect to (means3D, scales) of every Gaussian; the products are summed in float64."""
    xyz, sc = kw["means3D"].detach().to(dd).clone(), kw["scales"].detach().to(dd).clone()

    def image(x, s):
        return dense_twin.render(kw, dd, leaves={"means3D": x, "scales": s})[0].reshape(-1)

    Jx, Js = torch.autograd.functional.jacobian(image, (xyz, sc))
    J = torch.cat([Jx, Js], 2).double().numpy()          # [P, N, 6]
    return np.einsum("pni,pnj->nij", J, J)


def scaled(blocks, ref):
    """blocks / (d d^T) with d = sqrt(diag(ref)) per Gaussian (zeros where the reference's diagonal is zero)."""
    d = np.sqrt(np.maximum(np.diagonal(ref, axis1=-2, axis2=-1), 0.0))
    inv = np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 0.0)
    return blocks * inv[..., :, None] * inv[..., None, :]


def scaled_err(got, ref):
    """[N]: the max-norm error of every block scaled by the reference's diagonal."""
    return np.abs(scaled(got, ref) - scaled(ref, ref)).reshape(got.shape[0], -1).max(1)


def kappa(ref):
    """[N]: the condition number of every diagonally scaled block (inf for a singular one)."""
    out = np.full(ref.shape[0], np.inf)
    for i, b in enumerate(scaled(ref, ref)):
        w = np.linalg.eigvalsh(b)
        if w[0] > 0:
            out[i] = w[-1] / w[0]
    return out


def logdet(blocks):
    """[N]: numpy's log det of every block, -inf where it is not positive definite."""
    out = np.full(blocks.shape[0], -np.inf)
    for i, b in enumerate(blocks):
        if np.linalg.eigvalsh(b)[0] > 0:
            sign, val = np.linalg.slogdet(b)
            if sign > 0:
                out[i] = val
    return out


def harness_logdet(tri21):
    t = np.ascontiguousarray(tri21, np.float64)
    return float(harness().h_sens_logdet(ptr(t)))


def harness_view(kw, Hacc=None):
    """The CPU walk of one view (kw: scene kwargs with colors_precomp, scales, rotations; torch or numpy): H [N, 21] float64 added to
    Hacc (None: zeros), radii [N], dict(instances, longest list, pixels that ended before their list did)."""
    means3D = f32(kw["means3D"]); N = means3D.shape[0]
    op = f32(kw["opacities"]).reshape(-1); sc = f32(kw["scales"]); rot = f32(kw["rotations"]); col = f32(kw["colors_precomp"])
    bg = f32(kw["bg"]); vm = f32(kw["viewmatrix"]); pm = f32(kw["projmatrix"])
    Hacc = np.zeros((N, 21), np.float64) if Hacc is None else Hacc
    radii, info = np.zeros(N, np.int32), np.zeros(2, np.int64)
    n = harness().h_sens_view(N, int(kw["W"]), int(kw["H"]), ptr(means3D), ptr(op), ptr(sc), ptr(rot), ptr(col), ptr(bg), ptr(vm), ptr(pm),
                              float(kw["tanfovx"]), float(kw["tanfovy"]), ptr(radii), ptr(Hacc), ptr(info))
    return Hacc, radii, dict(instances=int(n), longest=int(info[0]), early=int(info[1]))
