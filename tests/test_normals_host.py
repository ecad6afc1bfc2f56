"""Normals, host side (no GPU): lg_math.h's normals arithmetic through the g++ harness against the float64 twin of
tests/normals_common.py, the hand-placed rows and maps of the contract, the header against the binding, and the
Python surface of lightgaussian_amd.normals / gaussian_renderer.render_geometry."""
import os
import types

import numpy as np
import pytest
import torch

import normals_common as nc
import test_abi
import tolerance
from common import ROOT, syn
from lightgaussian_amd import normals
from lightgaussian_amd.gaussian_renderer import render_features, render_geometry


# ---- rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", nc.NS)
def test_rows_against_float64(N):
    for ci, cam in enumerate(nc.cameras()):
        xyz, sc, q = nc.rows_inputs(N, seed=ci)
        vm = nc.view_matrix(cam)
        r64, k64, s64, keep = nc.keep_rows(xyz, sc, q, vm)
        rows, axis, sign = nc.harness_rows(xyz, sc, q, vm)
        assert np.array_equal(axis[keep], k64[keep]) and np.array_equal(sign[keep], s64[keep])
        en = np.abs(rows[keep, :3] - r64[keep, :3]).max(initial=0.0)
        ez = (np.abs(rows[keep, 3] - r64[keep, 3]) / nc.z_bound(xyz, vm)[keep]).max(initial=0.0)
        print(f"N {N} camera {ci}: normal error {en:.3e} (bound {nc.NORMAL_BOUND:.3e}), z error {ez:.3f} x its bound, {int((~keep).sum())} dropped")
        assert en <= nc.NORMAL_BOUND and ez <= 1.0
        assert np.abs(np.linalg.norm(rows[keep, :3], axis=1) - 1).max(initial=0.0) <= 2 * nc.NORMAL_BOUND


def test_rows_dropped_share():
    """Over every N of the list and both cameras at most 2 % of the rows lie within a decision margin."""
    dropped = total = 0
    for N in nc.NS:
        for ci, cam in enumerate(nc.cameras()):
            xyz, sc, q = nc.rows_inputs(N, seed=ci)
            keep = nc.keep_rows(xyz, sc, q, nc.view_matrix(cam))[3]
            dropped += int((~keep).sum()); total += N
    print(f"{dropped} of {total} rows dropped ({100.0 * dropped / total:.2f} %)")
    assert dropped <= 0.02 * total


def _one(xyz, sc, q, vm):
    rows, axis, sign = nc.harness_rows(np.array([xyz], np.float32), np.array([sc], np.float32), np.array([q], np.float32), vm)
    return rows[0], int(axis[0]), float(sign[0])


def test_rows_hand_placed():
    vm = np.eye(4, dtype=np.float32)
    vm[3, :3] = (0.0, 0.0, 4.0)                                  # the camera looks down +z from (0, 0, -4)
    unit = (1.0, 0.0, 0.0, 0.0)
    # equal smallest scales: the lowest index; all three equal: index 0
    assert _one((0, 0, 0), (-1.0, -3.0, -3.0), unit, vm)[1] == 1
    assert _one((0, 0, 0), (-3.0, -1.0, -3.0), unit, vm)[1] == 0
    assert _one((0, 0, 0), (-2.0, -2.0, -2.0), unit, vm)[1] == 0
    # a unit quaternion: R is the identity, the normal of axis 2 is (0, 0, 1), p_v = (0, 0, 4): n . p > 0 turns it to the camera
    row, k, s = _one((0, 0, 0), (0.0, 0.0, -3.0), unit, vm)
    assert k == 2 and s == -1.0 and row.tolist() == [0.0, 0.0, -1.0, 4.0]
    # n . p == 0 exactly keeps the sign: axis 0 = (1, 0, 0) against p_v = (0, 0, 4)
    row, k, s = _one((0, 0, 0), (-3.0, 0.0, 0.0), unit, vm)
    assert k == 0 and s == 1.0 and row.tolist() == [1.0, 0.0, 0.0, 4.0]
    # behind the camera: z < 0 comes out as it is, the normal (0, 0, 1) has n . p < 0 and stays
    row, k, s = _one((0, 0, -6.0), (0.0, 0.0, -3.0), unit, vm)
    assert s == 1.0 and row.tolist() == [0.0, 0.0, 1.0, -2.0]
    # the scale of the quaternion does not matter beyond rounding; powers of two not at all
    q = np.array([0.3, -0.5, 0.7, 0.2], np.float32)
    base = _one((0.2, -0.1, 0.3), (-1.0, -2.0, -0.5), q, vm)[0]
    for f, exact in ((1e3, False), (1e-3, False), (1024.0, True), (2.0 ** -10, True)):
        got = _one((0.2, -0.1, 0.3), (-1.0, -2.0, -0.5), q * np.float32(f), vm)[0]
        assert np.array_equal(got, base) if exact else np.abs(got - base).max() <= nc.NORMAL_BOUND, (f, got, base)
    # a zero quaternion: q^ = 0, R = identity (the forward's own treatment); a NaN one: NaN normal, z untouched
    assert _one((0, 0, 0), (0.0, 0.0, -3.0), (0.0, 0.0, 0.0, 0.0), vm)[0].tolist() == [0.0, 0.0, -1.0, 4.0]
    row = _one((0, 0, 0), (0.0, 0.0, -3.0), (np.nan, 0.0, 0.0, 0.0), vm)[0]
    assert np.isnan(row[:3]).all() and row[3] == 4.0


@pytest.mark.parametrize("N,cam_index", [(65, 0), (257, 1)])
def test_rows_backward(N, cam_index):
    ref = nc.rows_grad_reference(N, cam_index)
    xyz, sc, q, vm, g = ref["inputs"]
    d_xyz, d_rot = nc.harness_rows_bwd(xyz, sc, q, vm, g)
    for name, got, k in (("d_xyz", d_xyz, 0), ("d_rotation", d_rot, 1)):
        tolerance.assert_rule3(got, ref["float64"][k], ref["float32"][k], f"rows backward N {N} {name}")


# ---- images -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", nc.SIZES)
@pytest.mark.parametrize("kind", ("noisy", "plane"))
def test_depth_normals_and_gradients(W, H, kind):
    ref = nc.image_reference(W, H, kind)
    depth, nr, alpha, weight, g = ref["inputs"]
    if W >= 3 and H >= 3:
        c = nc.cross_products(torch.from_numpy(depth).double(), *nc.TANFOV).norm(dim=0).numpy()
        print(f"{W}x{H} {kind}: min |c| {c.min():.3e}, median {np.median(c):.3e}")
        assert c.min() >= 0.025 * np.median(c) and c.min() > 1e-6
        for n in ("nd", "d_depth_plain", "d_nr", "d_depth"):            # the float32 formula itself is well conditioned here
            assert np.abs(ref["float32"][n] - ref["float64"][n]).max() <= nc.N_D_TOL * max(1.0, np.abs(ref["float64"][n]).max()), n
    nd = nc.harness_depth_normals(depth)
    e = np.abs(nd - ref["float64"]["nd"]).max()
    print(f"{W}x{H} {kind}: N_d error {e:.3e}")
    assert e <= nc.N_D_TOL
    assert not nd[:, 0].any() and not nd[:, -1].any() and not nd[:, :, 0].any() and not nd[:, :, -1].any()
    d_nr, d_depth = nc.harness_loss_bwd(nr, depth, alpha, weight)
    got = dict(d_depth_plain=nc.harness_depth_normals_bwd(depth, g), d_nr=d_nr, d_depth=d_depth)
    nc.assert_image_gradients(got, ref, f"{W}x{H} {kind}", ("d_depth_plain", "d_nr", "d_depth"))
    loss = nc.harness_loss(nr, depth, alpha, weight)
    print(f"{W}x{H} {kind}: loss {loss:.7f} (float64 twin {ref['float64']['loss']:.7f})")
    assert abs(loss - ref["float64"]["loss"]) <= 1e-5


def test_unweighted_loss():
    ref = nc.image_reference(33, 17, "noisy", weighted=False)
    depth, nr, alpha, _none, _g = ref["inputs"]
    d_nr, d_depth = nc.harness_loss_bwd(nr, depth, alpha, None)
    nc.assert_image_gradients(dict(d_nr=d_nr, d_depth=d_depth), ref, "33x17 unweighted", ("d_nr", "d_depth"))
    assert abs(nc.harness_loss(nr, depth, alpha, None) - ref["float64"]["loss"]) <= 1e-5


def test_hand_placed_maps():
    W, H = 9, 7
    nr, alpha, weight, g = nc.loss_maps(W, H)
    # constant depth: (0, 0, -1) exactly in the interior
    nd = nc.harness_depth_normals(np.full((H, W), 3.25, np.float32))
    assert np.array_equal(nd[:, 1:-1, 1:-1], np.broadcast_to(np.array([0.0, 0.0, -1.0], np.float32)[:, None, None], (3, H - 2, W - 2)))
    # a NaN pixel zeroes itself and its four neighbours, and they pass no gradient
    depth = nc.depth_maps(W, H)["noisy"]
    clean = nc.harness_depth_normals(depth)
    depth[3, 4] = np.nan
    nd = nc.harness_depth_normals(depth)
    hit = np.zeros((H, W), bool)
    hit[3, 4] = hit[2, 4] = hit[4, 4] = hit[3, 3] = hit[3, 5] = True
    assert not nd[:, hit].any() and np.array_equal(nd[:, ~hit], clean[:, ~hit]) and np.isfinite(nd).all()
    d_plain = nc.harness_depth_normals_bwd(depth, g)
    d_nr, d_depth = nc.harness_loss_bwd(nr, depth, alpha, weight)
    assert np.isfinite(d_plain).all() and np.isfinite(d_depth).all() and np.isfinite(d_nr).all()
    assert d_plain[3, 4] == 0 and d_depth[3, 4] == 0 and not d_nr[:, hit].any()
    only = np.zeros_like(g)
    only[:, hit] = g[:, hit]                                          # a gradient arriving at the zeroed pixels alone goes nowhere
    assert not nc.harness_depth_normals_bwd(depth, only).any()
    # weight = 0 everywhere: L = 1 and every gradient is zero
    depth = nc.depth_maps(W, H)["plane"]
    zero = np.zeros((H, W), np.float32)
    assert nc.harness_loss(nr, depth, alpha, zero) == 1.0
    d_nr, d_depth = nc.harness_loss_bwd(nr, depth, alpha, zero)
    assert not d_nr.any() and not d_depth.any()


# ---- the header and the binding -----------------------------------------------------------------------------------------------
def test_header_matches_binding():
    declared = test_abi.check_extension_header("lightgaussian_normals.h", normals.PROTOTYPES)
    assert len(declared) == 7 and declared["lg_normal_loss_scratch_bytes"] == ("size_t", ["int32", "int32"])
    assert declared["lg_depth_normals"] == ("int32", ["int32", "int32", "pointer", "float", "float", "pointer", "uint32", "pointer"])
    text = open(os.path.join(ROOT, "include", "lightgaussian_normals.h")).read()
    assert "#define LG_ABI_VERSION" not in text and '#include "lightgaussian.h"' in text
    make = open(os.path.join(ROOT, "lightgaussian_amd", "csrc", "Makefile")).read()
    assert "lg_normals.h" in make and "lightgaussian_normals.h" in make


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def _cpu_inputs(N=65):
    xyz, sc, q = nc.rows_inputs(N, seed=0)
    return torch.from_numpy(xyz), torch.from_numpy(sc), torch.from_numpy(q), nc.cameras()[0]


def test_torch_backend_on_cpu_tensors():
    xyz, sc, q, cam = _cpu_inputs()
    vm = nc.view_matrix(cam)
    _r64, _k, _s, keep = nc.keep_rows(xyz.numpy(), sc.numpy(), q.numpy(), vm)
    want = nc.harness_rows(xyz.numpy(), sc.numpy(), q.numpy(), vm)[0]
    for backend in ("hip", "torch"):                                  # CPU tensors take the torch path either way
        x, r = xyz.clone().requires_grad_(), q.clone().requires_grad_()
        rows = normals.gaussian_normals(x, sc, r, cam, backend=backend)
        assert rows.shape == (65, 4) and rows.dtype == torch.float32
        assert np.abs(rows.detach().numpy()[keep] - want[keep]).max() <= 2 * nc.NORMAL_BOUND * max(1.0, np.abs(want[:, 3]).max())
        rows.sum().backward()
        assert x.grad is not None and r.grad is not None and torch.isfinite(r.grad).all()
    ref = nc.image_reference(33, 17, "noisy")
    depth, nr, alpha, weight, _g = (None if a is None else torch.from_numpy(a) for a in ref["inputs"])
    cam = nc.Camera()
    nd = normals.depth_to_normal(depth, cam, backend="torch")
    assert nd.shape == (3, 17, 33) and np.abs(nd.numpy() - ref["float64"]["nd"]).max() <= nc.N_D_TOL
    d, n = depth.clone().requires_grad_(), nr.clone().requires_grad_()
    loss = normals.normal_consistency_loss(n, d, alpha, cam, weight=weight)
    assert loss.dim() == 0 and abs(float(loss.detach()) - ref["float64"]["loss"]) <= 1e-5
    (nc.G_LOSS * loss).backward()
    nc.assert_image_gradients(dict(d_nr=n.grad.numpy(), d_depth=d.grad.numpy()), ref, "torch backend", ("d_nr", "d_depth"))
    for shape in ((1, 1), (2, 5)):                                    # no interior: zeros, and a backward that runs
        d = torch.rand(shape).requires_grad_()
        nd = normals.depth_to_normal(d, cam)
        nd.sum().backward()
        assert not nd.any() and not d.grad.any()
    # the torch path treats a NaN depth as the kernels do
    d = depth.clone(); d[5, 7] = float("nan"); d.requires_grad_()
    nd = normals.depth_to_normal(d, cam)
    nd.sum().backward()
    assert torch.isfinite(nd).all() and torch.isfinite(d.grad).all() and not nd[:, 4, 7].any() and d.grad[5, 7] == 0
    assert np.array_equal(nd.detach().numpy(), nc.harness_depth_normals(d.detach().numpy())) or \
        np.abs(nd.detach().numpy() - nc.harness_depth_normals(d.detach().numpy())).max() <= nc.N_D_TOL


def test_refusals():
    xyz, sc, q, cam = _cpu_inputs(8)
    bad = [lambda: normals.gaussian_normals(xyz.double(), sc, q, cam), lambda: normals.gaussian_normals(xyz, sc[:, :2], q, cam),
           lambda: normals.gaussian_normals(xyz, sc, q[:7], cam), lambda: normals.gaussian_normals(xyz, sc, q, cam, backend="triton"),
           lambda: normals.gaussian_normals(xyz.numpy(), sc, q, cam)]
    depth, nr, alpha = torch.rand(5, 6), torch.rand(3, 5, 6), torch.rand(5, 6)
    c = nc.Camera()
    bad += [lambda: normals.depth_to_normal(depth[None], c), lambda: normals.depth_to_normal(depth.half(), c),
            lambda: normals.depth_to_normal(torch.zeros(0, 4), c),
            lambda: normals.normal_consistency_loss(nr[:2], depth, alpha, c), lambda: normals.normal_consistency_loss(nr, depth, alpha[:4], c),
            lambda: normals.normal_consistency_loss(nr, depth, alpha, c, weight=alpha.double()),
            lambda: normals.normal_consistency_loss(nr, depth, alpha, c, weight=torch.rand(6, 5)),
            lambda: normals.normal_consistency_loss(nr, depth, alpha.to("meta"), c)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")
    # contiguity is asked of GPU tensors by backend='hip' (no device needed to see the check: a fake .is_cuda)
    t = types.SimpleNamespace(is_cuda=True, is_contiguous=lambda: False)
    with pytest.raises(ValueError, match="contiguous"):
        normals._resolve("depth_to_normal", "hip", (("depth", t),))
    assert normals._resolve("depth_to_normal", "hip", (("depth", depth),)) == "torch"


def test_render_geometry_refuses_what_render_features_refuses():
    from lightgaussian_amd.vectree import CompressedGaussians, TrainableCompressed
    g = syn.make_gaussians(16, seed=3)
    cam = syn.orbit_camera(1, 7, 33, 17, radius=4.0)
    pipe = syn.PipelineParams()
    for cls in (CompressedGaussians, TrainableCompressed):
        pc = cls.__new__(cls)
        for call in (lambda: render_features(cam, pc, pipe, "depth", geometry_grad=True), lambda: render_geometry(cam, pc, pipe)):
            with pytest.raises(NotImplementedError, match="to_dense"):
                call()
    for call in (lambda: render_features(cam, g, pipe, "depth", geometry_grad=True, options={"camera_grad": True}),
                 lambda: render_geometry(cam, g, pipe, options={"camera_grad": True})):
        with pytest.raises(NotImplementedError, match="camera_grad"):
            call()
    cov = syn.PipelineParams()
    cov.compute_cov3D_python = True
    with pytest.raises(NotImplementedError, match="compute_cov3D_python"):
        render_geometry(cam, g, cov)
