"""Shared by tests/test_filter3d_host.py and tests/test_gpu_filter3d.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_filter3d_harness.cpp, the camera sets and point generator of the update tests, the rows of the apply tests and
the float64 / float32 formulas both are compared with.

Update.  Cameras: syn.orbit_camera / syn.look_at_camera around the origin, two focal lengths among them (FoVx 60 and 40 degrees).
The point generator works in float64 on the float32 inputs the kernel reads and DROPS every candidate whose u or v lies within
1e-3 W (1e-3 H) of a border of the widened frustum [-0.15 W, 1.15 W] x [-0.15 H, 1.15 H], or whose z lies within 1e-4 of 0.2, for
any camera: the float64 reference then decides every seen_n with a margin thousands of times the float32 error, and the comparisons
exclude no row.  assert_categories() checks that the rows kept still hold Gaussians seen by all cameras, by some, by none, and behind
a camera.

Apply.  rows(): log-scales N(log 0.05, 0.7), logits N(0, 2), filters exp(N(log 0.03, 1)) with a quarter of the rows at exactly 0.
apply_formula() is the specification written in torch (any dtype, differentiable):
    raw        u_k = exp(r_k)^2 + f^2   r'_k = 0.5 log u_k   w_k = exp(r_k)^2 / u_k   c = sqrt(w_0 w_1 w_2)   y = sigmoid(o) c
               o' = log(y / (1 - y))
    activated  s'_k = sqrt(s_k^2 + f^2),  sigma' = sigma c."""
import ctypes as C
import math

import numpy as np
import torch

import common
from common import ptr, syn  # noqa: F401  (the tests of this feature take ptr from here)

SIZES = ((70, 45), (33, 17))
NS = (1, 63, 64, 65, 257, 1000)
CHUNK = 64                      # LG_F3D_CHUNK: cameras per LDS stage of lg_filter3d_update_kernel
VS = (1, 3, CHUNK + 1)


def harness():
    P, I = C.c_void_p, C.c_int
    return common.build_harness("filter3d", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_filter3d": (None, [I, P, I, P, P, P, P, P])})


# ---- cameras -----------------------------------------------------------------------------------------------------------------
def cameras(V, W, H):
    """V cameras of W x H pixels: camera 0 is the pitched, rolled look_at camera of the parity scenes, the others orbit the origin at
    radius 6 on two heights; FoVx alternates between 60 and 40 degrees (two focal lengths)."""
    cams = [syn.look_at_camera((2.5, -1.0, -4.0), (0.1, 0.0, 0.0), W, H, roll_deg=20.0)]
    n = max(V - 1, 1)
    for k in range(V - 1):
        cams.append(syn.orbit_camera(k, n, W, H, radius=6.0, fovx_deg=40.0 if k % 2 == 0 else 60.0, height_y=0.0 if k % 3 else -1.5))
    return cams


def camera_rows(cams):
    """float32 [V, 20]: {viewmatrix[16], tanfovx, tanfovy, W, H} -- the values lg_filter_camera holds (tan evaluated in double and
    rounded once, as the binding does)."""
    rows = np.zeros((len(cams), 20), np.float32)
    for k, c in enumerate(cams):
        rows[k, :16] = c.world_view_transform.numpy().reshape(16)
        rows[k, 16], rows[k, 17] = math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5)
        rows[k, 18], rows[k, 19] = c.image_width, c.image_height
    return rows


def reference64(means, rows):
    """The float64 formula on the float32 inputs.  dict of [N, V] arrays x, y, z, u, v, t, seen, bound (the issue's bound on |t32 - t64|)
    and margin_ok (the generator's acceptance)."""
    p = np.asarray(means, np.float64)
    r = np.asarray(rows, np.float64)
    vm = r[:, :16].reshape(-1, 4, 4)
    W, H = r[:, 18], r[:, 19]
    fx, fy = W / (2.0 * r[:, 16]), H / (2.0 * r[:, 17])
    xyz = np.einsum("nk,vkc->nvc", p, vm[:, :3, :3]) + vm[None, :, 3, :3]
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = x / z * fx + 0.5 * W, y / z * fy + 0.5 * H
        t = z / fx
    seen = (z > 0.2) & (u >= -0.15 * W) & (u <= 1.15 * W) & (v >= -0.15 * H) & (v <= 1.15 * H)
    mag = np.einsum("nk,vk->nv", np.abs(p), np.abs(vm[:, :3, 2])) + np.abs(vm[None, :, 3, 2])
    bound = 4.0 * 2.0 ** -24 * mag / fx + 2.0 ** -23 * np.abs(t)
    with np.errstate(invalid="ignore"):
        near_border = ((np.abs(u + 0.15 * W) < 1e-3 * W) | (np.abs(u - 1.15 * W) < 1e-3 * W) | (np.abs(v + 0.15 * H) < 1e-3 * H)
                       | (np.abs(v - 1.15 * H) < 1e-3 * H))
    margin_ok = ~(near_border | (np.abs(z - 0.2) < 1e-4) | (np.abs(z) < 1e-6))
    return dict(x=x, y=y, z=z, u=u, v=v, t=t, seen=seen, bound=bound, margin_ok=margin_ok)


def filter64(ref):
    """(filter [N] float64, seen [N]) of the float64 reference: sqrt(0.2) min t, the maximum for unseen rows, 0 if nobody is seen."""
    seen = ref["seen"].any(1)
    t = np.where(ref["seen"], ref["t"], np.inf).min(1)
    f = math.sqrt(0.2) * t
    fill = f[seen].max() if seen.any() else 0.0
    return np.where(seen, f, fill), seen


_POINTS = {}


def points(N, V, W, H, seed=11):
    """(means float32 [N, 3], camera rows float32 [V, 20]): N candidates that pass the generator's margins for every camera.  A third
    of the candidates lies in the scene's box (seen by most cameras), a third in a box of +-7 (seen by some: many lie behind a camera),
    a third far above the orbit plane (seen by none).  Computed once per key."""
    key = (N, V, W, H, seed)
    if key in _POINTS:
        return _POINTS[key]
    rows = camera_rows(cameras(V, W, H))
    g = torch.Generator().manual_seed(seed + 1000 * V + N)
    M = 6 * N + 60
    u = torch.rand(M, 3, generator=g).double() * 2 - 1
    kind = torch.arange(M) % 3
    box = torch.where(kind[:, None] == 0, torch.tensor([1.5, 1.0, 1.5]).double(), torch.tensor([7.0, 3.0, 7.0]).double())
    cand = u * box
    cand[kind == 2, 1] = -40.0 - 20.0 * u[kind == 2, 1].abs()        # far "above" (down is +y): outside every widened frustum
    cand = cand.float().numpy()
    ok = reference64(cand, rows)["margin_ok"].all(1)
    means = np.ascontiguousarray(cand[ok][:N])
    assert means.shape[0] == N, "the generator ran out of candidates"
    _POINTS[key] = (means, rows)
    return _POINTS[key]


def assert_categories(ref, V, what=""):
    """The rows the generator kept still hold every kind of Gaussian (for V == 1 `some` and `all` coincide)."""
    seen_n = ref["seen"].sum(1)
    facts = dict(all=int((seen_n == V).sum()), some=int(((seen_n > 0) & (seen_n < V)).sum()), none=int((seen_n == 0).sum()),
                 behind=int((ref["z"] < 0).any(1).sum()))
    print(f"{what} rows seen by all / some / none / behind a camera: {facts}")
    assert facts["all"] >= 1 and facts["none"] >= 1 and facts["behind"] >= 1
    assert V == 1 or facts["some"] >= 1
    return facts


def run_harness(means, rows):
    """dict t [N, V], seen_nv [N, V], filter [N], seen [N] of the g++ build of the kernel's arithmetic."""
    lib = harness()
    N, V = means.shape[0], rows.shape[0]
    t, snv = np.zeros((N, V), np.float32), np.zeros((N, V), np.uint8)
    f, s = np.zeros(N, np.float32), np.zeros(N, np.uint8)
    lib.h_filter3d(N, ptr(means), V, ptr(rows), ptr(t), ptr(snv), ptr(f), ptr(s))
    return dict(t=t, seen_nv=snv.astype(bool), filter=f, seen=s.astype(bool))


# ---- apply -------------------------------------------------------------------------------------------------------------------
def rows(N, seed=5):
    """(log-scales [N, 3], logits [N, 1], filter [N, 1]) float32 CPU tensors; every fourth row has filter 0."""
    g = torch.Generator().manual_seed(seed + N)
    r = torch.randn(N, 3, generator=g) * 0.7 + math.log(0.05)
    o = torch.randn(N, 1, generator=g) * 2.0
    f = torch.exp(torch.randn(N, 1, generator=g) + math.log(0.03))
    f[torch.arange(N) % 4 == 3] = 0.0
    return r, o, f


def apply_formula(scaling, opacity, f, raw):
    """The specification in torch, in the dtype of its arguments, differentiable.  scaling [N, 3], opacity [N, 1], f [N, 1]."""
    s = torch.exp(scaling) if raw else scaling
    u = s * s + f * f
    w = s * s / u
    c = torch.sqrt(w[:, 0:1] * w[:, 1:2] * w[:, 2:3])
    if raw:
        y = torch.sigmoid(opacity) * c
        return 0.5 * torch.log(u), torch.log(y / (1 - y))
    return torch.sqrt(u), opacity * c


def activated(out_scaling, out_opacity, raw):
    """The outputs in the activated domain, float64 numpy: (exp(r'), sigmoid(o')) of raw outputs, the outputs themselves otherwise."""
    a, b = out_scaling.detach().cpu().double(), out_opacity.detach().cpu().double()
    if raw:
        a, b = torch.exp(a), torch.sigmoid(b)
    return a.numpy(), b.numpy()


def rel_elem(got, ref):
    """Largest elementwise relative error."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.abs(ref)).max())


_ERR32 = {}


def err32(N, raw):
    """{"scaling": e, "opacity": e}: the float32 formula's own elementwise relative error against float64, in the activated domain, on
    rows(N); with the float64 outputs ("ref": (scales, opacity))."""
    key = (N, raw)
    if key in _ERR32:
        return _ERR32[key]
    r, o, f = rows(N)
    a = (r if raw else torch.exp(r)), (o if raw else torch.sigmoid(o))
    ref = activated(*apply_formula(a[0].double(), a[1].double(), f.double(), raw), raw)
    got = activated(*apply_formula(a[0], a[1], f, raw), raw)
    _ERR32[key] = dict(scaling=rel_elem(got[0], ref[0]), opacity=rel_elem(got[1], ref[1]), ref=ref, inputs=(a[0], a[1], f))
    return _ERR32[key]


def upstream_gradients(N, seed=9):
    g = torch.Generator().manual_seed(seed + N)
    return torch.randn(N, 3, generator=g), torch.randn(N, 1, generator=g)


_GRAD = {}


def grad_reference(N, raw):
    """{"float64": {"scaling", "opacity"}, "float32": {...}}: autograd of sum(g_s s') + sum(g_o o') through apply_formula on rows(N)."""
    key = (N, raw)
    if key in _GRAD:
        return _GRAD[key]
    a_s, a_o, f = err32(N, raw)["inputs"]
    gs, go = upstream_gradients(N)
    out = {}
    for dd in (torch.float64, torch.float32):
        s, o = a_s.to(dd).clone().requires_grad_(), a_o.to(dd).clone().requires_grad_()
        os_, oo = apply_formula(s, o, f.to(dd), raw)
        ((os_ * gs.to(dd)).sum() + (oo * go.to(dd)).sum()).backward()
        out["float64" if dd == torch.float64 else "float32"] = {"scaling": s.grad.numpy().astype(np.float64), "opacity": o.grad.numpy().astype(np.float64)}
    _GRAD[key] = out
    return out


def backward_formula(scaling, opacity, f, gs, go, raw):
    """The issue's closed-form backward in torch (any dtype): what lg_filter3d_apply_bwd evaluates.  Returns (dL/dscaling, dL/dopacity)."""
    s = torch.exp(scaling) if raw else scaling
    u = s * s + f * f
    w = s * s / u
    c = torch.sqrt(w[:, 0:1] * w[:, 1:2] * w[:, 2:3])
    if raw:
        sg = torch.sigmoid(opacity)
        y = sg * c
        return gs * w + go * (1 - w) / (1 - y), go * (1 - sg) / (1 - y)
    sp = torch.sqrt(u)
    return gs * s / sp + go * opacity * c * (1 - w) / s, go * c
