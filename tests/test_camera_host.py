"""Camera pose gradients without a GPU: lg_backward_camera / lg_camera_scratch_bytes declared, bound and exported; every argument
refusal that comes before a device call (C ABI and Python); lg_backward_camera_terms -- the per-Gaussian step of lg_camera_bwd, compiled
from the product's lg_math.h with g++ -- summed in double over a scene and compared with float64 torch autograd; the translation
identity; and pose.PoseCamera.

The comparand of the harness test is autograd of the LINEAR functional
    F = sum_i  a0 ix + a1 iy + a2 A + a3 B + a4 C + dRGB . rgb
of the per-Gaussian projection (pixel mean ix, iy; conic A, B, C with power = -(A dx^2 + C dy^2) / 2 - B dx dy; SH colour), restated
below from oracle/torch_dense.py::render_dense's lines, with respect to viewmatrix, projmatrix and campos: its gradient is exactly what
the kernel sums when the blend stage hands it acc = (a0..a4) and dL/drgb = dRGB.  Rule 3 (camera_grad_common.assert_rule3), with the
same autograd in float32 as d32.  Measured on 2000 Gaussians at 161 x 83, float32 autograd floor / harness error:
    camera            viewmatrix            projmatrix            campos
    pitched_rolled    1.2e-06 / 1.3e-06     1.7e-07 / 5.0e-08     9.6e-08 / 2.0e-07
    steep_offcentre   1.6e-06 / 1.5e-06     2.6e-07 / 6.7e-08     2.1e-07 / 9.6e-08
    inside            1.1e-05 / 2.6e-05     1.6e-07 / 1.2e-07     1.7e-07 / 2.2e-07
    inside_wide       5.5e-06 / 3.1e-06     1.5e-07 / 4.6e-07     3.0e-07 / 2.3e-07
    orbit             1.4e-06 / 1.2e-06     5.9e-07 / 6.6e-08     8.3e-07 / 1.8e-07
so the bound is 1e-4 everywhere; the translation identity holds to 1.3e-8 of sum |dL/dp|.  The floors of the full render are in
tests/test_gpu_camera.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import camera_common
import camera_grad_common as cg
import common
from common import f32, ptr, syn
from lightgaussian_amd import _lib, gaussian_renderer, pose, rasterizer
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
from lightgaussian_amd.vectree import CompressedGaussians, TrainableCompressed
from oracle import torch_dense

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")


def test_symbols_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("lg_camera_scratch_bytes", 1), ("lg_backward_camera", 12)):
        m = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, f"{name} is not declared in include/lightgaussian.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.EXPORTS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.lg_camera_scratch_bytes.restype is C.c_size_t and lib.lg_backward_camera.restype is C.c_int
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.lg_abi_version() == 7      # purely additive


def test_scratch_bytes_monotone_and_non_zero():
    lib = _lib.load()
    prev = 0
    for n in (0, 1, 63, 64, 65, 256, 257, 65536, 65537, 70001, 1 << 20, 3 << 20, (1 << 29) - 1):
        b = lib.lg_camera_scratch_bytes(n)
        assert b >= prev and (n < 1 or b > 0), (n, b)
        # one row of 27 doubles per workgroup of 256 Gaussians
        assert b >= ((max(n, 1) + 255) // 256) * 27 * 8
        prev = b


P = 0x1000      # a non-null pointer that must never be dereferenced


def _view(**kw):
    a = dict(H=32, W=32, flags=0, seg=0)
    a.update(kw)
    return _lib.lg_view(a["H"], a["W"], 1.0, 1.0, P, 1.0, P, P, 0, P, 0, a["flags"], a["seg"])


def _call(lib, **kw):
    a = dict(view=_view(), N=10, M=0, shs=None, colors=P, radii=P, geom=P, binning=P, R=100, rows=P, g_vm=P, g_pm=P, g_cp=P, scratch=P, gauss=True)
    a.update(kw)
    g = _lib.lg_gaussians(a["N"], a["M"], P, a["shs"], a["colors"], P, P, P, None, None)
    v = None if a["view"] is None else C.byref(a["view"])
    return lib.lg_backward_camera(v, C.byref(g) if a["gauss"] else None, a["radii"], a["geom"], a["binning"], a["R"], a["rows"], a["g_vm"],
                                  a["g_pm"], a["g_cp"], a["scratch"], None)


@pytest.mark.parametrize("what, kw", [
    ("null view", dict(view=None)), ("null view", dict(gauss=False)), ("bad sizes", dict(N=-1)), ("bad sizes", dict(view=_view(H=0))),
    ("segment_length", dict(view=_view(seg=100))), ("precomputed colors", dict(colors=None)),
    ("gradient outputs are required", dict(g_vm=None)), ("gradient outputs are required", dict(g_pm=None)),
    ("gradient outputs are required", dict(g_cp=None)), ("gradient outputs are required", dict(N=0, g_cp=None)),
    ("missing scratch", dict(scratch=None)), ("missing scratch", dict(N=0, scratch=None)),
    ("num_rendered", dict(R=-1)), ("num_rendered", dict(R=1 << 30)),
    ("missing buffer", dict(radii=None)), ("missing buffer", dict(geom=None)), ("missing buffer", dict(binning=None)),
    ("missing buffer", dict(rows=None)),
    ("LG_FLAG_SAVE_SH_JACOBIAN", dict(colors=None, shs=P, M=16)),
])
def test_c_abi_refuses_bad_arguments_before_any_device_call(what, kw):
    """This process has no GPU: a call that reached the HIP runtime would come back as LG_ERR_DEVICE."""
    lib = _lib.load()
    assert _call(lib, **kw) == _lib.LG_ERR_INVALID_ARGUMENT
    assert what.lower() in lib.lg_last_error().decode().lower(), lib.lg_last_error().decode()


# ---- the per-Gaussian terms against float64 autograd -------------------------------------------------------------------------
def _functional(dd, p, scales, rots, sh, acc5, drgb, vis, vm, pm, cp, W, H, tanfovx, tanfovy):
    """F (see the module docstring) in dtype dd; the projection is render_dense's, line for line, without the rasterisation."""
    N = p.shape[0]
    ph = torch.cat([p, torch.ones(N, 1, dtype=dd)], 1)
    pview = ph @ vm
    phom = ph @ pm
    p_w = 1.0 / (phom[:, 3] + 1e-7)
    ndc = phom[:, :2] * p_w[:, None]
    tz = pview[:, 2]
    r, x, y, z = rots[:, 0], rots[:, 1], rots[:, 2], rots[:, 3]
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(N, 3, 3)
    L = Rm * scales[:, None, :]
    Sig = L @ L.transpose(1, 2)
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = pview[:, 0] / tz, pview[:, 1] / tz
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz).detach(), pview[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz).detach(), pview[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], 1).view(N, 2, 3)
    T2 = J @ vm[:3, :3].t()
    cov = T2 @ Sig @ T2.transpose(1, 2)
    a, b, c_ = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c_ - b * b
    A, B, Cc = c_ / det, -b / det, a / det
    ix = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    iy = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    d = p - cp[None, :]
    d = d / d.norm(dim=1, keepdim=True)
    rgb = torch_dense.eval_sh(3, sh, d) + 0.5
    per = acc5[:, 0] * ix + acc5[:, 1] * iy + acc5[:, 2] * A + acc5[:, 3] * B + acc5[:, 4] * Cc + (drgb * rgb).sum(1)
    return per[vis].sum()


def _camera(name):
    if name == "orbit":
        return syn.orbit_camera(1, 7, camera_common.W, camera_common.H, radius=4.0)
    return camera_common.camera(name)


@pytest.mark.parametrize("name", camera_common.NAMES + ("orbit",))
def test_camera_terms_match_float64_autograd(name):
    lib = cg.harness()
    g, cam = camera_common.gaussians(), _camera(name)
    W, H = camera_common.W, camera_common.H
    N = g.num
    rs = np.random.RandomState(17)
    acc5 = rs.randn(N, 5).astype(np.float32)
    drgb = rs.randn(N, 3).astype(np.float32)
    p, sc, rot, sh = f32(g.get_xyz), f32(g.get_scaling), f32(g.get_rotation), f32(g.get_features)
    vm, pm, cp = f32(cam.world_view_transform), f32(cam.full_proj_transform), f32(cam.camera_center)
    tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    sums = np.zeros(27, np.float64); dmean = np.zeros((N, 3), np.float32); vis = np.zeros(N, np.int32)
    n = lib.h_camera_terms(N, 3, W, H, ptr(p), ptr(sc), ptr(rot), ptr(acc5), ptr(drgb), ptr(sh), ptr(vm), ptr(pm), ptr(cp), tanx, tany,
                           ptr(sums), ptr(dmean), ptr(vis))
    assert n == int(vis.sum()) >= 200
    if name in camera_common.INSIDE:
        assert n < N        # Gaussians behind the near plane are invisible lanes: zeros
    got = dict(zip(cg.NAMES, cg.unpack(sums)))
    ref = {}
    for dd in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(a).to(dd)  # noqa: E731
        cam_t = [t(vm).requires_grad_(), t(pm).requires_grad_(), t(cp).requires_grad_()]
        _functional(dd, t(p), t(sc), t(rot), t(sh), t(acc5), t(drgb), torch.from_numpy(vis > 0), *cam_t, W, H, tanx, tany).backward()
        ref["float64" if dd == torch.float64 else "float32"] = {k: c.grad.numpy().astype(np.float64) for k, c in zip(cg.NAMES, cam_t)}
    cg.assert_rule3(got, ref, f"terms {name}")
    # the twin gives exact zeros in the columns the forward never reads; the packed layout has no slot for them
    assert not ref["float64"]["viewmatrix"][:, 3].any() and not ref["float64"]["projmatrix"][:, 2].any()
    # the translation identity: sum_i dL/dmeans3D_i = vm[:3,:3] g_vm[3,:3] + pm[:3,:] g_pm[3,:] - g_campos, the left side from
    # lg_backward_geom's mean3D (plus the direction term) of the same Gaussians
    lhs = dmean.astype(np.float64).sum(0)
    rhs = vm[:3, :3].astype(np.float64) @ got["viewmatrix"][3, :3] + pm[:3, :].astype(np.float64) @ got["projmatrix"][3, :] - got["campos"]
    scale = np.abs(dmean.astype(np.float64)).sum(0)
    print(f"identity {name}: |lhs - rhs| / sum|dL/dp| = {np.abs(lhs - rhs) / scale}")
    assert (np.abs(lhs - rhs) <= 1e-4 * scale).all()
    # and in the float64 autograd itself it is exact to rounding (the issue's 1e-16 is relative to the sum of magnitudes)
    r = ref["float64"]
    rhs64 = vm[:3, :3].astype(np.float64) @ r["viewmatrix"][3, :3] + pm[:3, :].astype(np.float64) @ r["projmatrix"][3, :] - r["campos"]
    assert (np.abs(lhs - rhs64) <= 1e-4 * scale).all()


def test_colours_as_inputs_have_no_camera_centre_term():
    lib = cg.harness()
    g, cam = camera_common.gaussians(), _camera("pitched_rolled")
    N = g.num
    rs = np.random.RandomState(3)
    acc5 = rs.randn(N, 5).astype(np.float32); drgb = rs.randn(N, 3).astype(np.float32)
    p, sc, rot = f32(g.get_xyz), f32(g.get_scaling), f32(g.get_rotation)
    vm, pm, cp = f32(cam.world_view_transform), f32(cam.full_proj_transform), f32(cam.camera_center)
    sums = np.zeros(27, np.float64); dmean = np.zeros((N, 3), np.float32); vis = np.zeros(N, np.int32)
    lib.h_camera_terms(N, 3, camera_common.W, camera_common.H, ptr(p), ptr(sc), ptr(rot), ptr(acc5), ptr(drgb), None, ptr(vm), ptr(pm), ptr(cp),
                       math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), ptr(sums), ptr(dmean), ptr(vis))
    assert not sums[24:].any() and np.abs(sums[:24]).min() > 0


# ---- PoseCamera --------------------------------------------------------------------------------------------------------------
def test_pose_camera_at_zero_equals_the_base_camera():
    base = camera_common.camera("pitched_rolled")
    cam = pose.PoseCamera(base)
    assert [n for n, _ in cam.named_parameters()] == ["xi"] and cam.xi.shape == (6,) and not cam.xi.any()
    assert torch.equal(cam.world_view_transform, base.world_view_transform)
    # P is recovered as inverse(world_view) @ full_proj and rounded to float32 once: equal to float32 rounding of the products
    assert torch.allclose(cam.full_proj_transform, base.full_proj_transform, rtol=1e-5, atol=1e-5)
    assert torch.allclose(cam.camera_center, base.camera_center, rtol=1e-6, atol=1e-6)
    for n in ("image_width", "image_height", "FoVx", "FoVy"):
        assert getattr(cam, n) == getattr(base, n)
    # a base camera that carries its projection matrix (scene/cameras.py) is taken at its word
    base.projection_matrix = syn.projection_matrix(base.znear, base.zfar, base.FoVx, base.FoVy).transpose(0, 1)
    cam2 = pose.PoseCamera(base)
    assert torch.equal(cam2.projection_matrix, base.projection_matrix)
    assert torch.allclose(cam2.full_proj_transform, base.full_proj_transform, rtol=1e-6, atol=1e-6)


def test_pose_camera_construction_passes_gradcheck():
    base = camera_common.camera("inside")
    wvt = base.world_view_transform.double()
    proj = torch.linalg.inv(wvt) @ base.full_proj_transform.double()
    xi = torch.tensor([0.03, -0.02, 0.05, 0.1, -0.04, 0.02], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: pose.pose_matrices(v, wvt, proj), (xi,), eps=1e-6, atol=1e-6)
    # a rigid correction: the rotation block stays as orthonormal as the base's (a float32 matrix: 1e-6), the camera centre maps to the
    # view-space origin, and a pure translation moves the view-space origin by tau
    w, _f, c = pose.pose_matrices(xi.detach(), wvt, proj)
    assert torch.allclose(w[:3, :3] @ w[:3, :3].t(), torch.eye(3, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(torch.cat([c, torch.ones(1, dtype=torch.float64)]) @ w, torch.tensor([0, 0, 0, 1.0], dtype=torch.float64), atol=1e-12)
    tau = torch.tensor([0, 0, 0, 0.1, 0.2, 0.3], dtype=torch.float64)
    assert torch.allclose(pose.pose_matrices(tau, wvt, proj)[0][3, :3], wvt[3, :3] + tau[3:], atol=1e-12)


def test_pose_camera_has_the_attribute_surface_render_reads():
    cam = pose.PoseCamera(syn.orbit_camera(0, 4, 16, 16))
    g = syn.make_gaussians(8)
    rs = gaussian_renderer._settings(cam, g, syn.PipelineParams(), torch.zeros(3), 1.0, False)
    assert rs.viewmatrix.shape == (4, 4) and rs.projmatrix.shape == (4, 4) and rs.campos.shape == (3,)
    assert rs.viewmatrix.requires_grad and rs.projmatrix.requires_grad and rs.campos.requires_grad
    assert (rs.image_width, rs.image_height) == (16, 16)


# ---- Python refusals (no GPU needed: they come before any device call) -----------------------------------------------------------
def _rs(**kw):
    return GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False, False)._replace(**kw)


def _inputs(n=4):
    return dict(means3D=torch.zeros(n, 3), means2D=torch.zeros(n, 3), opacities=torch.ones(n, 1), scales=torch.ones(n, 3), rotations=torch.ones(n, 4),
                colors_precomp=torch.ones(n, 3))


def test_python_refuses_camera_grad_where_it_cannot_be_honoured():
    on = {"camera_grad": True}
    with pytest.raises(ValueError, match="f_count"):
        GaussianRasterizer(_rs(f_count=True), options=on)(**_inputs())
    with pytest.raises(ValueError, match="sh_jacobian"):
        GaussianRasterizer(_rs(), options=dict(on, sh_jacobian=False))(**_inputs())
    rasterizer.set_grad_chunk_hook(lambda first, count, grads: None, chunks=2)
    try:
        with pytest.raises(ValueError, match="chunk hook"):
            GaussianRasterizer(_rs(), options=on)(**_inputs())
    finally:
        rasterizer.set_grad_chunk_hook(None)

    class Sink:
        def add(self, *a):
            pass
    with pytest.raises(ValueError, match="sh_grad_sink"):
        GaussianRasterizer(_rs(), options=dict(on, sh_grad_sink=Sink()))(**_inputs())
    with pytest.raises(ValueError, match="True or False"):
        rasterizer.resolve_options({"camera_grad": 1})
    # the raw path refuses the same way
    g = syn.make_gaussians(4)
    with pytest.raises(ValueError, match="sh_jacobian"):
        rasterizer.rasterize_gaussians_raw(g._xyz, torch.zeros(4, 3), g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation, _rs(),
                                           dict(on, sh_jacobian=False))
    # with the option on and nothing in its way the call gets as far as the device check; off, it is the call it always was
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianRasterizer(_rs(), options=on)(**_inputs())
    assert rasterizer.resolve_options()["camera_grad"] is False


def test_render_entry_points_that_would_ignore_the_option_refuse_it():
    on = {"camera_grad": True}
    cam, g, pipe = syn.orbit_camera(0, 4, 16, 16), syn.make_gaussians(8), syn.PipelineParams()
    with pytest.raises(NotImplementedError, match="camera_grad"):
        gaussian_renderer.count_render(cam, g, pipe, torch.zeros(3), options=on)
    with pytest.raises(NotImplementedError, match="camera_grad"):
        gaussian_renderer.render_features(cam, g, pipe, "depth", options=on)
    for cls in (CompressedGaussians, TrainableCompressed):
        with pytest.raises(NotImplementedError, match="camera_grad"):
            gaussian_renderer.render(cam, object.__new__(cls), pipe, torch.zeros(3), options=on)
    with rasterizer.options(camera_grad=True):      # the thread-local form reaches the same checks
        with pytest.raises(NotImplementedError, match="camera_grad"):
            gaussian_renderer.count_render(cam, g, pipe, torch.zeros(3))
