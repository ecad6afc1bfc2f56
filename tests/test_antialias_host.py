"""Antialiased splatting without a GPU: the arithmetic of LG_FLAG_ANTIALIAS -- lg_aa_ratio / lg_aa_rho, lg_project_t, lg_backward_geom_t and
lg_backward_camera_terms_t of the product's lg_math.h, compiled with g++ (tests/cpu_harness/lg_antialias_harness.cpp) -- against float64
torch; the <false> instantiations against the functions that existed before the mode did, bit for bit; the flag, the ABI version, the
option and the `pipe.antialiasing` pick-up.

The comparand of the backward tests is autograd of the LINEAR functional
    F = sum_i  a0 ix + a1 iy + a2 A + a3 B + a4 C + a5 op'          op' = sigma rho
of the per-Gaussian projection (tests/antialias_common.py::cov2d: render_dense's own lines), in float64 (d64) and float32 (d32): its
gradient is what K9 (or lg_camera_bwd) computes when the blend stage hands it acc = (a0..a5).  Rule of tests/camera_grad_common.py,
per tensor in the max norm: rel_err(got, d64) <= max(1e-4, 3 rel_err(d32, d64)).  Scene: "N300_70x45" with the six hand-placed
Gaussians of antialias_common (rho at the floor, a rank-one covariance, behind the camera, the EWA clamp active, ...)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import antialias_common as aa
import camera_grad_common as cg
import common
import tolerance
from common import syn
from lightgaussian_amd import _lib, gaussian_renderer, rasterizer

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")
NAME = "N300_70x45"


def test_scene_conditions_of_the_float64_twin():
    facts = aa.assert_scene_conditions()
    assert facts["hits_on"] < facts["hits_off"]


# ---- rho -------------------------------------------------------------------------------------------------------------------
def _rho_harness(a0, b, c0):
    lib = aa.harness()
    a0, b, c0 = (np.ascontiguousarray(v, np.float32) for v in (a0, b, c0))
    out = np.zeros(a0.shape[0], np.float32)
    lib.h_aa_rho(a0.shape[0], aa.ptr(a0), aa.ptr(b), aa.ptr(c0), aa.ptr(out))
    return out


def test_rho_against_the_float64_formula():
    rs = np.random.RandomState(1)
    n = 20000
    # random symmetric positive definite 2 x 2 matrices over five decades of size, kept where the blurred matrix is well conditioned
    l1, l2 = 10.0 ** rs.uniform(-3, 2, n), 10.0 ** rs.uniform(-3, 2, n)
    th = rs.uniform(0, math.pi, n)
    a0 = l1 * np.cos(th) ** 2 + l2 * np.sin(th) ** 2
    c0 = l1 * np.sin(th) ** 2 + l2 * np.cos(th) ** 2
    b = (l1 - l2) * np.sin(th) * np.cos(th)
    a0, b, c0 = (v.astype(np.float32) for v in (a0, b, c0))
    a, c = a0.astype(np.float64) + 0.3, c0.astype(np.float64) + 0.3
    keep = a * c / (a * c - b.astype(np.float64) ** 2) < 100
    a0, b, c0 = a0[keep], b[keep], c0[keep]
    assert keep.sum() > n // 2
    got = _rho_harness(a0, b, c0)
    d64 = aa.rho_of(*(torch.from_numpy(v).double() for v in (a0, b, c0))).numpy()
    d32 = aa.rho_of(*(torch.from_numpy(v) for v in (a0, b, c0))).numpy()
    floor, err = aa.rel_err(d32, d64), aa.rel_err(got, d64)
    print(f"rho: rel_err {err:.3e} (float32 torch {floor:.3e}); range {d64.min():.3f} .. {d64.max():.3f}")
    assert d64.min() < 0.1 and d64.max() > 0.99
    assert err <= tolerance.rule3_bound(floor)


def test_rho_edge_cases_are_exact():
    at_floor = np.sqrt(np.float32(aa.FLOOR))            # sqrtf(0.000025f), correctly rounded
    nan = np.float32("nan")
    # x below the floor; det0 < 0 < det1 (rounding of a rank-one covariance); det0 == 0; NaN in each place; a0 = c0 = 0.3f
    a0 = np.array([1e-6, 1.0, 1.0, nan, 1.0, 1.0, 0.3], np.float32)
    b = np.array([0.0, 1.1, 1.0, 0.0, nan, 0.0, 0.0], np.float32)
    c0 = np.array([1e-6, 1.0, 1.0, 1.0, 1.0, nan, 0.3], np.float32)
    got = _rho_harness(a0, b, c0)
    print("rho edge cases:", got)
    assert (got[:6].view(np.uint32) == at_floor.view(np.uint32)).all()
    # a0 = c0 = 0.3f: det0 / det1 is 1/4 up to the rounding of 0.3f + 0.3f, rho 0.5 to an ulp
    assert abs(float(got[6]) - 0.5) <= 2.0 ** -23


# ---- lg_project ------------------------------------------------------------------------------------------------------------
def _project(mode, kw, opacities):
    lib = aa.harness()
    m, sc, rot, op = aa.f32(kw["means3D"]), aa.f32(kw["scales"]), aa.f32(kw["rotations"]), np.ascontiguousarray(opacities, np.float32).reshape(-1)
    vm, pm = aa.f32(kw["viewmatrix"]), aa.f32(kw["projmatrix"])
    out = np.zeros((m.shape[0], 16), np.float32)
    lib.h_aa_project(mode, m.shape[0], kw["W"], kw["H"], aa.ptr(m), aa.ptr(sc), aa.ptr(rot), aa.ptr(op), aa.ptr(vm), aa.ptr(pm),
                     float(kw["tanfovx"]), float(kw["tanfovy"]), aa.ptr(out))
    return out.view(np.uint32)


def test_project_uses_the_compensated_opacity_wherever_it_uses_the_opacity():
    kw = aa.combo_kwargs(NAME, "sh3")
    sigma = aa.f32(kw["opacities"]).reshape(-1)
    rho32 = aa.rho32_harness(kw)
    plain, off, on = _project(2, kw, sigma), _project(0, kw, sigma), _project(1, kw, sigma)
    assert np.array_equal(plain, off)                                  # mode off: the existing function, bit for bit
    vis = plain[:, 0] != 0
    assert vis.sum() >= 250 and np.array_equal(on[:, 0], plain[:, 0])
    # radius, reference rectangle, mean and conic do not depend on the option
    assert np.array_equal(on[:, 1:6], plain[:, 1:6]) and np.array_equal(on[:, 10:15], plain[:, 10:15])
    # the record's opacity is the float32 product sigma rho32 ...
    assert np.array_equal(on[vis, 15], (sigma * rho32)[vis].view(np.uint32))
    # ... and the footprint cull is the one lg_project makes when it is handed that product
    pre = _project(2, kw, sigma * rho32)
    assert np.array_equal(on[:, 6:10], pre[:, 6:10])
    tiles = lambda r: ((r[:, 8].astype(np.int64) - r[:, 6]) * (r[:, 9].astype(np.int64) - r[:, 7]))  # noqa: E731
    t_on, t_off = tiles(on.view(np.float32)), tiles(plain.view(np.float32))
    print(f"instances: {int(t_off.sum())} without, {int(t_on.sum())} with the compensation")
    assert (t_on <= t_off).all() and t_on.sum() < t_off.sum()
    removed = (sigma >= 1 / 255) & (sigma * rho32 < 1 / 255) & vis
    assert removed.any() and not t_on[removed].any() and t_off[removed].all()


# ---- the per-Gaussian backward -----------------------------------------------------------------------------------------------
def _functional(dd, t, form, acc6, vis, vm, pm, W, H, tanx, tany):
    p = t["means3D"]
    scales = rots = cov = None
    op = t["opacities"].reshape(-1)
    if form == "precov":
        cov = t["cov3D_precomp"]
    elif form == "raw":
        scales, rots, op = torch.exp(t["scales"]), torch.nn.functional.normalize(t["rotations"]), torch.sigmoid(op)
    else:
        scales, rots = t["scales"], t["rotations"]
    a0, b, c0, _tz = aa.cov2d(p, vm, W, H, tanx, tany, scales, rots, cov)
    a, c = a0 + 0.3, c0 + 0.3
    det = a * c - b * b
    A, B, Cc = c / det, -b / det, a / det
    phom = torch.cat([p, torch.ones(p.shape[0], 1, dtype=dd)], 1) @ pm
    ndc = phom[:, :2] / (phom[:, 3:4] + 1e-7)
    ix = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    iy = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    per = acc6[:, 0] * ix + acc6[:, 1] * iy + acc6[:, 2] * A + acc6[:, 3] * B + acc6[:, 4] * Cc + acc6[:, 5] * op * aa.rho_of(a0, b, c0)
    return per[vis].sum()


def _inputs(form):
    """The per-Gaussian tensors of one geometry input form (float32 torch), the camera and the image size."""
    g, cam, W, H = aa.small_scene(NAME)
    kw = aa.combo_kwargs(NAME, "precov" if form == "precov" else "sh3")
    t = {k: kw[k] for k in ("means3D", "opacities", "scales", "rotations", "cov3D_precomp") if k in kw}
    if form == "raw":
        t = dict(means3D=g._xyz.detach(), opacities=g._opacity.detach(), scales=g._scaling.detach(), rotations=g._rotation.detach())
    return t, kw, W, H


def _harness_backward(mode, form, t, kw, acc6):
    lib = aa.harness()
    N = t["means3D"].shape[0]
    a = {k: aa.f32(v) for k, v in t.items()}
    out = dict(means3D=np.zeros((N, 3), np.float32), scales=np.zeros((N, 3), np.float32), rotations=np.zeros((N, 4), np.float32),
               cov3D_precomp=np.zeros((N, 6), np.float32), opacities=np.zeros((N, 1), np.float32))
    vis = np.zeros(N, np.int32)
    pre = form == "precov"
    lib.h_aa_backward(mode, N, int(form == "raw"), kw["W"], kw["H"], aa.ptr(a["means3D"]), aa.ptr(a.get("scales")), aa.ptr(a.get("rotations")),
                      aa.ptr(a.get("cov3D_precomp")), aa.ptr(a["opacities"]), aa.ptr(acc6), aa.ptr(aa.f32(kw["viewmatrix"])),
                      aa.ptr(aa.f32(kw["projmatrix"])), float(kw["tanfovx"]), float(kw["tanfovy"]), aa.ptr(out["means3D"]),
                      None if pre else aa.ptr(out["scales"]), None if pre else aa.ptr(out["rotations"]),
                      aa.ptr(out["cov3D_precomp"]) if pre else None, aa.ptr(out["opacities"]), aa.ptr(vis))
    for k in (("scales", "rotations") if pre else ("cov3D_precomp",)):
        del out[k]
    return out, vis


@pytest.mark.parametrize("form", ["scales_rotations", "precov", "raw"])
def test_backward_against_float64_autograd(form):
    t, kw, W, H = _inputs(form)
    N = t["means3D"].shape[0]
    acc6 = np.random.RandomState(23).randn(N, 6).astype(np.float32)
    got, vis = _harness_backward(1, form, t, kw, acc6)
    assert N - aa.N_EXTRA <= vis.sum() < N                     # one of the hand-placed Gaussians is behind the camera
    ref = {}
    for dd in (torch.float64, torch.float32):
        leaves = {k: v.to(dd).detach().clone().requires_grad_() for k, v in t.items()}
        _functional(dd, leaves, form, torch.from_numpy(acc6).to(dd), torch.from_numpy(vis > 0), kw["viewmatrix"].to(dd), kw["projmatrix"].to(dd),
                    W, H, kw["tanfovx"], kw["tanfovy"]).backward()
        ref["float64" if dd == torch.float64 else "float32"] = {k: v.grad.numpy().astype(np.float64) for k, v in leaves.items()}
    aa.assert_rule(got, ref, tuple(got), f"backward {form}")
    assert not any(v[vis == 0].any() for v in got.values())
    # the compensation is in the numbers: without its terms the same call is far outside the rule
    plain, _ = _harness_backward(0, form, t, kw, acc6)
    geo = "cov3D_precomp" if form == "precov" else "scales"
    assert aa.rel_err(plain[geo], ref["float64"][geo]) > 1e-2 and aa.rel_err(plain["opacities"], ref["float64"]["opacities"]) > 1e-2


@pytest.mark.parametrize("form", ["scales_rotations", "precov", "raw"])
def test_mode_off_is_the_existing_backward_bit_for_bit(form):
    t, kw, _W, _H = _inputs(form)
    acc6 = np.random.RandomState(29).randn(t["means3D"].shape[0], 6).astype(np.float32)
    off, _ = _harness_backward(0, form, t, kw, acc6)
    old, _ = _harness_backward(2, form, t, kw, acc6)
    for k in off:
        assert np.array_equal(off[k].view(np.uint32), old[k].view(np.uint32)), k
        assert off[k].any()


# ---- the camera terms --------------------------------------------------------------------------------------------------------
def _camera_sums(mode, t, kw, acc6):
    lib = aa.harness()
    a = {k: aa.f32(v) for k, v in t.items()}
    sums = np.zeros(27, np.float64)
    lib.h_aa_camera_terms(mode, a["means3D"].shape[0], kw["W"], kw["H"], aa.ptr(a["means3D"]), aa.ptr(a["scales"]), aa.ptr(a["rotations"]),
                          aa.ptr(a["opacities"]), aa.ptr(acc6), aa.ptr(aa.f32(kw["viewmatrix"])), aa.ptr(aa.f32(kw["projmatrix"])),
                          float(kw["tanfovx"]), float(kw["tanfovy"]), aa.ptr(sums))
    return sums


def test_camera_terms_against_float64_autograd():
    t, kw, W, H = _inputs("scales_rotations")
    N = t["means3D"].shape[0]
    acc6 = np.random.RandomState(31).randn(N, 6).astype(np.float32)
    vm_g, pm_g, cp_g = cg.unpack(_camera_sums(1, t, kw, acc6))
    assert not cp_g.any()                       # colours as inputs: no camera-centre term
    vm32 = kw["viewmatrix"].float()
    vis = (t["means3D"].float() @ vm32[:3, 2] + vm32[3, 2]) > 0.2
    ref = {}
    for dd in (torch.float64, torch.float32):
        vm, pm = (kw[n].to(dd).detach().clone().requires_grad_() for n in ("viewmatrix", "projmatrix"))
        _functional(dd, {k: v.to(dd) for k, v in t.items()}, "scales_rotations", torch.from_numpy(acc6).to(dd), vis, vm, pm, W, H,
                    kw["tanfovx"], kw["tanfovy"]).backward()
        ref["float64" if dd == torch.float64 else "float32"] = dict(viewmatrix=vm.grad.numpy().astype(np.float64),
                                                                    projmatrix=pm.grad.numpy().astype(np.float64))
    aa.assert_rule(dict(viewmatrix=vm_g, projmatrix=pm_g), ref, ("viewmatrix", "projmatrix"), "camera terms")
    # mode off: the existing function's sums, bit for bit -- and not the antialiased ones
    off, old = _camera_sums(0, t, kw, acc6), _camera_sums(2, t, kw, acc6)
    assert np.array_equal(off.view(np.uint64), old.view(np.uint64))
    assert aa.rel_err(cg.unpack(off)[0], ref["float64"]["viewmatrix"]) > 1e-2


# ---- the flag, the ABI, the option ---------------------------------------------------------------------------------------------
def test_flag_is_declared_once_with_a_value_of_its_own():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    flags = dict((n, int(v)) for n, v in re.findall(r"\b(LG_FLAG_\w+)\s*=\s*(\d+)", src))
    assert flags["LG_FLAG_ANTIALIAS"] == 16384 == _lib.FLAG_ANTIALIAS
    assert [n for n, v in flags.items() if v == 16384] == ["LG_FLAG_ANTIALIAS"]
    assert all(v & (v - 1) == 0 for v in flags.values()) and len(set(flags.values())) == len(flags)
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", src).group(1)) == 7 and _lib.load().lg_abi_version() == 7 == _lib.ABI_VERSION


def test_option_is_a_validated_bool_off_by_default():
    assert rasterizer.resolve_options()["antialiasing"] is False
    assert rasterizer.resolve_options({"antialiasing": True})["antialiasing"] is True
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="True or False"):
            rasterizer.resolve_options({"antialiasing": bad})
        with pytest.raises(ValueError, match="True or False"):
            rasterizer.set_option("antialiasing", bad)
        with pytest.raises(ValueError, match="True or False"):
            rasterizer.options(antialiasing=bad)
    with rasterizer.options(antialiasing=True):
        assert rasterizer.resolve_options()["antialiasing"] is True
        assert rasterizer.resolve_options({"antialiasing": False})["antialiasing"] is False
    assert rasterizer.resolve_options()["antialiasing"] is False
    assert len(rasterizer.GaussianRasterizationSettings._fields) == 13


class _Pipe(syn.PipelineParams):
    antialiasing = True


def test_pipe_antialiasing_is_picked_up_and_an_explicit_option_wins(monkeypatch):
    seen = []

    class Recorder:
        def __init__(self, raster_settings, options=None):
            seen.append(options)

        def __call__(self, **kw):
            raise RuntimeError("stop")

    def raw(*args):
        seen.append(args[-1])
        raise RuntimeError("stop")

    def blend(*args, **kw):
        seen.append(kw["options"])
        raise RuntimeError("stop")

    monkeypatch.setattr(gaussian_renderer, "GaussianRasterizer", Recorder)
    monkeypatch.setattr(gaussian_renderer, "rasterize_gaussians_raw", raw)
    import lightgaussian_amd.features as features
    monkeypatch.setattr(features, "blend_features", blend)
    cam, g, bg = syn.orbit_camera(0, 4, 16, 16), syn.make_gaussians(8), torch.zeros(3)
    calls = (lambda pipe, o: gaussian_renderer.render(cam, g, pipe, bg, options=o),                                      # fused
             lambda pipe, o: gaussian_renderer.render(cam, g, pipe, bg, options=dict(o or {}, fuse_getters=False)),     # unfused
             lambda pipe, o: gaussian_renderer.count_render(cam, g, pipe, bg, options=o),
             lambda pipe, o: gaussian_renderer.render_features(cam, g, pipe, "depth", options=o))
    for call in calls:
        for pipe, opts, want in ((_Pipe(), None, True), (_Pipe(), {"antialiasing": False}, False), (_Pipe(), {"fast_exp": False}, True),
                                 (syn.PipelineParams(), None, None), (syn.PipelineParams(), {"antialiasing": True}, True)):
            seen.clear()
            with pytest.raises(RuntimeError, match="stop"):
                call(pipe, opts)
            assert len(seen) == 1 and (seen[0] or {}).get("antialiasing") is want, (pipe, opts, seen)
    assert not hasattr(syn.PipelineParams(), "antialiasing")
