"""-m gpu: fine-tuning a VecTree-compressed model in place -- vectree.TrainableCompressed, lg_vq_code_index / lg_vq_colors_bwd
(csrc/lg_vq_color_bwd.h), gaussian_renderer.render_compressed_trainable -- against float64 autograd, the dense backward on the
dequantised model, and its own promises (determinism, forward unchanged, trains what it saves)."""
import functools

import numpy as np
import pytest
import torch

import vq_finetune_common as fc
from common import syn
from lightgaussian_amd import vectree
from lightgaussian_amd.gaussian_renderer import render, render_compressed
from vq_finetune_common import DEV, UNFUSED, bits

pytestmark = pytest.mark.gpu

# N (no multiple of 64), max degree, active degree, assignment: a vq_ratio (0: no VQ Gaussian, 1: no non-VQ row) or "hand"
# (K = 16: a code of three chunks, one of exactly 256, one of 257, three empty codes).  d = 48 and d = 27 (rows padded 54 -> 64 B).
CASES = [(3001, 3, 3, 0.6), (3001, 3, 1, "hand"), (3001, 2, 2, "hand"), (2113, 2, 0, 0.6), (2113, 3, 3, 0.0), (2113, 2, 2, 1.0),
         (2113, 3, 1, 1.0), (2113, 2, 2, 0.0)]
WITH_OWN_ROWS = [c for c in CASES if c[3] != 1.0]


def bg_color():
    return torch.tensor([0.1, 0.2, 0.3], device=DEV)


@functools.lru_cache(maxsize=None)
def case(N, deg, active, how):
    """Everything the tests of one case share, computed once and left unchanged: the packed model, its plain device form, the
    camera, dL/dcolours of one rasterizer backward (L1 against a second scene's render)."""
    packed = fc.packed_case(N, deg, how)
    cg = vectree.CompressedGaussians.from_packed(packed, DEV)
    cg.active_sh_degree = active
    cam = syn.orbit_camera(1, 8, fc.W, fc.H).to(DEV)
    g = fc.dl_dcolors(cg, cam, 1, bg_color())
    return packed, cg, cam, g


def colour_stage_grads(tc, cam, g):
    """_rows.grad and the colour part of _xyz.grad: the backward of colors() alone, fed with g."""
    tc._rows.grad = tc._xyz.grad = None
    tc.colors(cam.camera_center).backward(g)
    return tc._rows.grad.clone(), tc._xyz.grad.clone()


@pytest.mark.parametrize("N,deg,active,how", CASES)
def test_gradients_against_float64_autograd(N, deg, active, how):
    """|kernel - float64| <= 4 |torch float32 - float64| on the max error, per tensor: the same restatement (rows[slot] ->
    eval_sh, + 0.5, clamp_min 0) at float32 is the yardstick, both sides fed the same dL/dcolours.  At active degree 0 the
    colour does not depend on the view direction: both sides give dL/dxyz = 0 exactly and there is no yardstick to apply."""
    packed, cg, cam, g = case(N, deg, active, how)
    tc = cg.trainable(("rows", "xyz"))
    M, d, K = (deg + 1) ** 2, cg.sh_dim, cg.codebook_size
    assert int((g != 0).any(1).sum()) > N // 20
    rows_grad, xyz_grad = colour_stage_grads(tc, cam, g)
    assert rows_grad.shape == (K + int((cg._slot >= K).sum()), d) and xyz_grad.shape == (N, 3)
    vals = tc.rows[:, :d].float()
    r64, x64, col64 = fc.restated_gradients(vals, tc._xyz, tc._slot, cam.camera_center, active, M, g, torch.float64)
    r32, x32, _ = fc.restated_gradients(vals, tc._xyz, tc._slot, cam.camera_center, active, M, g, torch.float32)
    for name, got, f32, f64 in (("_rows.grad", rows_grad, r32, r64), ("_xyz.grad (colour part)", xyz_grad, x32, x64)):
        yard = (f32.double() - f64).abs().max().item()
        err = (got.double() - f64).abs().max().item()
        print(f"N {N} degree {active}/{deg} {how}: {name} |kernel - f64| {err:.3g}, |torch f32 - f64| {yard:.3g}, max |f64| {f64.abs().max().item():.3g}")
        if name.startswith("_xyz") and active == 0:
            assert not got.any() and not f64.any()
            continue
        assert yard > 0 and err <= 4 * yard
    # the clamp is exercised, and a clamped channel contributes nothing: its g is live, the float64 colour is 0
    clamped_live = (col64 == 0) & (g != 0)
    assert int(clamped_live.sum()) > 10
    # columns of inactive degrees: exactly 0 (and nothing but zeros behind them in the float64 reference)
    inactive = torch.ones(M, 3, dtype=torch.bool)
    inactive[:(active + 1) ** 2] = False
    cols = fc.m3_to_file_order(inactive[None])[0].to(DEV)
    assert int(cols.sum()) == 3 * (M - (active + 1) ** 2)
    assert not rows_grad[:, cols].any() and not r64[:, cols].any()
    assert rows_grad[:, ~cols].abs().sum() > 0
    # rows of empty codes: exactly 0
    used = torch.zeros(rows_grad.shape[0], dtype=torch.bool, device=DEV)
    used[tc._slot.long()] = True
    if how == "hand":
        assert not used[list(fc.HAND_EMPTY)].any() and int(used[:K].sum()) == K - len(fc.HAND_EMPTY)
        counts = torch.bincount(tc._slot.long(), minlength=K)[:3].tolist()
        assert counts == [600, 256, 257]
    assert used[K:].all()
    assert not rows_grad[~used].any()
    assert torch.isfinite(rows_grad).all() and torch.isfinite(xyz_grad).all()


@pytest.mark.parametrize("N,deg,active,how", WITH_OWN_ROWS)
def test_rows_of_their_own_equal_the_dense_backward(N, deg, active, how):
    """For a non-VQ Gaussian _rows.grad[slot[i]], permuted to [M][3], is the shs.grad[i] of render(to_dense()) with the getters
    unfused, value for value: both go through lg_backward_sh on the same dL/drgb.  (torch.equal: an invisible Gaussian's row is
    +0 in the dense path, which never runs lg_backward_sh for it, and C * 0 = +-0 here -- the one difference in bits.)"""
    packed, cg, cam, _ = case(N, deg, active, how)
    tc = cg.trainable(fc.ALL_PARAMS)
    pipe, bg, M, K = syn.PipelineParams(), bg_color(), (deg + 1) ** 2, cg.codebook_size
    fc.l1(render(cam, tc, pipe, bg, options=UNFUSED)["render"], fc.target_image(1)).backward()
    dense = tc.to_dense().requires_grad_(True)
    fc.l1(render(cam, dense, pipe, bg, options=UNFUSED)["render"], fc.target_image(1)).backward()
    shs_grad = torch.cat([dense._features_dc.grad, dense._features_rest.grad], dim=1)             # [N, M, 3]
    own = tc._slot >= K
    assert bool(own.all()) if how == 0.0 else 0 < int(own.sum()) < N
    got = fc.file_order_to_m3(tc._rows.grad[tc._slot[own].long()], M)
    assert got.abs().sum() > 0
    assert torch.equal(got, shs_grad[own])
    nz = shs_grad[own] != 0
    assert torch.equal(bits(got)[nz], bits(shs_grad[own])[nz])
    # the whole position gradient too: geometry part + colour part, one addition in either path
    assert torch.equal(tc._xyz.grad, dense._xyz.grad)


@pytest.mark.parametrize("N,deg,active,how", [(3001, 3, 3, 0.6), (3001, 2, 2, "hand"), (2113, 3, 1, 1.0)])
def test_end_to_end_gradient_of_render(N, deg, active, how):
    """loss.backward() through render(TrainableCompressed) with every tensor trainable against to_dense() + the unfused render,
    the SH gradient gathered onto the rows in float64: max |g - ref| <= 1e-4 max |ref| per tensor (rule 1)."""
    packed, cg, cam, _ = case(N, deg, active, how)
    tc = cg.trainable(fc.ALL_PARAMS)
    pipe, bg, d = syn.PipelineParams(), bg_color(), cg.sh_dim
    pkg = render(cam, tc, pipe, bg, options=UNFUSED)
    assert pkg["render"].requires_grad and pkg["viewspace_points"].requires_grad
    fc.l1(pkg["render"], fc.target_image(1)).backward()
    dense = tc.to_dense().requires_grad_(True)
    ref_pkg = render(cam, dense, pipe, bg, options=UNFUSED)
    fc.l1(ref_pkg["render"], fc.target_image(1)).backward()
    shs_grad = torch.cat([dense._features_dc.grad, dense._features_rest.grad], dim=1)
    ref_rows = torch.zeros(tc._rows.shape, dtype=torch.float64, device=DEV).index_add_(0, tc._slot.long(), fc.m3_to_file_order(shs_grad).double())
    pairs = [("_rows", tc._rows.grad.double(), ref_rows), ("_xyz", tc._xyz.grad, dense._xyz.grad), ("_opacity", tc._opacity.grad, dense._opacity.grad),
             ("_scaling", tc._scaling.grad, dense._scaling.grad), ("_rotation", tc._rotation.grad, dense._rotation.grad),
             ("viewspace_points", pkg["viewspace_points"].grad, ref_pkg["viewspace_points"].grad)]
    for name, got, ref in pairs:
        err, scale = (got.double() - ref.double()).abs().max().item(), ref.abs().max().item()
        print(f"N {N} degree {active}/{deg} {how}: {name} max |g - ref| {err:.3g}, max |ref| {scale:.3g}")
        assert scale > 0 and err <= 1e-4 * scale
    assert ref_rows.shape[1] == d


def test_the_backward_is_deterministic():
    """The same backward twice, once more on a second stream, once after an unrelated render: every gradient bit equal.  And
    sync_rows() leaves the padding of the fp16 table zero."""
    packed, cg, cam, g = case(3001, 2, 2, "hand")
    tc = cg.trainable(("rows", "xyz"))
    pipe, bg = syn.PipelineParams(), bg_color()
    first = colour_stage_grads(tc, cam, g)
    second = colour_stage_grads(tc, cam, g)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = colour_stage_grads(tc, cam, g)
    torch.cuda.current_stream(DEV).wait_stream(side)
    other = fc.scene(5003, 3, seed=9).to(DEV)
    with torch.no_grad():
        render(syn.orbit_camera(4, 8, 160, 120).to(DEV), other, pipe, bg)
    fourth = colour_stage_grads(tc, cam, g)
    for again in (second, third, fourth):
        assert torch.equal(bits(first[0]), bits(again[0])) and torch.equal(bits(first[1]), bits(again[1]))

    def whole():
        for t in tc.parameters():
            t.grad = None
        fc.l1(render(cam, tc, pipe, bg)["render"], fc.target_image(1)).backward()
        return tc._rows.grad.clone(), tc._xyz.grad.clone()

    a, b = whole(), whole()
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])) and a[0].abs().sum() > 0
    d = tc.sh_dim
    assert tc.rows.shape[1] == 32 and d == 27
    with torch.no_grad():
        tc._rows.add_(0.01 * torch.randn(tc._rows.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)))
    tc.sync_rows()
    assert not tc.rows[:, d:].any()
    assert torch.equal(tc.rows[:, :d], tc._rows.detach().half())
    assert not torch.equal(tc.rows, cg.rows)                              # the model it came from keeps its own table


def test_training_lowers_the_loss_and_saves_what_it_trained():
    """A coarse codebook (K = 16), 30 Adam steps on _rows against renders of the unquantised scene over 4 cameras: the mean L1
    goes down; from_packed(repack()) renders, by the plain forward-only path, the training forward's image bit for bit."""
    N, deg, K = 3001, 2, 16
    g = fc.scene(N, deg, seed=5, rest_std=0.1)
    feats = fc.ply_rows(g)
    importance = (torch.randperm(N, generator=torch.Generator().manual_seed(8)).float() + 1.0) / N
    packed = vectree.quantize_model(feats.to(DEV), importance.to(DEV), vq_ratio=0.9, codebook_size=K, iterations=4, chunk=1024,
                                    generator=torch.Generator(device=DEV).manual_seed(5))
    cg = vectree.CompressedGaussians.from_packed(packed, DEV)
    tc = cg.trainable()
    assert [tuple(p.shape) for p in tc.parameters()] == [(K + int(N * (1 - 0.9)), 27)]
    pipe, bg = syn.PipelineParams(), bg_color()
    cams = [syn.orbit_camera(k, 8, fc.W, fc.H).to(DEV) for k in (0, 2, 4, 6)]
    dense = g.to(DEV)
    with torch.no_grad():
        targets = [render(c, dense, pipe, bg)["render"].clone() for c in cams]

    def mean_l1():
        with torch.no_grad():
            return sum(fc.l1(render(c, tc, pipe, bg)["render"], t).item() for c, t in zip(cams, targets)) / len(cams)

    before = mean_l1()
    opt = torch.optim.Adam(tc.parameters(), lr=2e-3)
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        for c, t in zip(cams, targets):
            (fc.l1(render(c, tc, pipe, bg)["render"], t) / len(cams)).backward()
        opt.step()
        tc.sync_rows()
    after = mean_l1()
    print(f"mean L1 over {len(cams)} cameras: {before:.6f} before, {after:.6f} after 30 Adam steps on the rows")
    assert after < before
    with torch.no_grad():
        trained = render(cams[1], tc, pipe, bg)
    repacked = tc.repack()
    back = render_compressed(cams[1], vectree.CompressedGaussians.from_packed(repacked, DEV), pipe, bg)
    assert torch.equal(bits(trained["render"]), bits(back["render"])) and torch.equal(trained["radii"], back["radii"])
    assert torch.equal(tc._slot, cg._slot)
    assert np.array_equal(repacked["vq_indexs"], packed["vq_indexs"]) and np.array_equal(repacked["non_vq_mask"], packed["non_vq_mask"])
    assert not np.array_equal(repacked["codebook"], packed["codebook"]) and repacked["codebook"].dtype == np.float16
    assert np.array_equal(repacked["other_attribute"], packed["other_attribute"]) and np.array_equal(repacked["xyz"], packed["xyz"])


@pytest.mark.parametrize("N,deg,active,how", [(3001, 3, 3, 0.6), (2113, 2, 0, 0.6)])
def test_the_forward_is_unchanged(N, deg, active, how):
    packed, cg, cam, _ = case(N, deg, active, how)
    pipe, bg = syn.PipelineParams(), bg_color()
    plain = render_compressed(cam, cg, pipe, bg)
    for params in (("rows",), fc.ALL_PARAMS):
        tc = cg.trainable(params)
        assert tc.active_sh_degree == active
        out = render(cam, tc, pipe, bg)
        assert out["render"].requires_grad and set(out) == set(plain)
        assert torch.equal(bits(out["render"]), bits(plain["render"])) and torch.equal(out["radii"], plain["radii"])
        assert torch.equal(out["visibility_filter"], plain["visibility_filter"])
        assert fc.np_equal_packed(tc.repack(), packed)
    # a plain CompressedGaussians keeps the forward-only path: nothing requires grad
    again = render(cam, cg, pipe, bg)
    assert not any(torch.is_tensor(v) and v.requires_grad for v in again.values())
    assert torch.equal(bits(again["render"]), bits(plain["render"]))
    with pytest.raises(NotImplementedError):
        render(cam, cg.trainable(), syn.PipelineParams(convert_SHs_python=True), bg)
