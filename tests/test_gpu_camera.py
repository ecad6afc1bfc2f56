"""-m gpu: camera pose gradients (option camera_grad: lg_backward_camera behind lg_backward) against the dense autograd twin.

Reference and rule: tests/camera_grad_common.py -- oracle/torch_dense.py::render_dense differentiated with respect to viewmatrix,
projmatrix and campos in float64 (d64) and float32 (d32) on the CPU with the same image gradient; per output tensor, in the max norm,
    rel_err(g, d64) <= max(1e-4, 3 rel_err(d32, d64)).
Every reference is computed once per (scene, input combination) and shared by both arithmetic modes.

FLOAT32 FLOORS rel_err(d32, d64), measured on the CPU (image gradient: torch.randn, seed 0; SH degree 3; background (0.1, 0.2, 0.3)):

  scene                                  viewmatrix   projmatrix   campos
  N300_70x45 (camera_grad_common)        3.8e-06      2.5e-06      8.0e-07
  N64_33x17                              2.1e-06      2.2e-06      7.1e-07
  pitched_rolled (camera_common, 2000)   7.5e-06      2.4e-05      2.8e-05
  steep_offcentre                        4.1e-06      6.5e-06      1.2e-06
  inside                                 1.7e-06      2.4e-06      1.7e-06
  inside_wide                            8.2e-06      2.7e-06      9.9e-07

so the bound is 1e-4 on all of them.  The tests recompute the floors and print every figure before asserting.

Cases of the parity test: the four input combinations (SH degree 3, SH degree 1, colors_precomp, cov3D_precomp) on the two small
scenes and on the `inside` camera (near-plane lanes, both clamps, 300 px splats), SH degree 3 on the other three cameras -- the dense
twin of a 2000-Gaussian view at 161 x 83 takes 2 .. 11 s per combination on the CPU -- each in both arithmetic modes (fast_exp on / off).

test_fused_and_unfused_render: whether the two paths give the same camera-gradient bits is printed by the test.  Measured on an
MI355X on N300_70x45: bit-equal (they need not be: the fused path evaluates the activations inside the kernels, to ~1e-7 of torch's).

lg_camera_reduce loops when there are more than 256 partial rows, one per workgroup of 256 Gaussians: N > 65536.
test_reduction_beyond_one_pass uses N = 70001 (274 rows)."""
import math

import numpy as np
import pytest
import torch

import camera_common as cc
import camera_grad_common as cg
import gpu_common
import tolerance
from common import bits as _bits
from common import syn
from lightgaussian_amd import pose
from lightgaussian_amd.gaussian_renderer import render
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [pytest.param(True, id="fast_exp"), pytest.param(False, id="canonical")]


def run(kw, gimg, *, camera_grad=True, fast_exp=True, options=None, after_forward=None):
    """gpu_common.run_rasterizer with the camera gradients on and fast_exp spelled out."""
    return gpu_common.run_rasterizer(kw, gimg, dict(options or {}, fast_exp=fast_exp), camera_grad=camera_grad, after_forward=after_forward)


def _small(name, combo, n=None):
    g, cam, W, H = cg.small_scene(name)
    return cg.combo_kwargs(g, cam, W, H, combo, n=n), cg.image_gradient(H, W)


def _camera_scene(name, combo):
    cc.check_preconditions()
    return cg.combo_kwargs(cc.gaussians(), cc.camera(name), cc.W, cc.H, combo), cg.image_gradient(cc.H, cc.W)


PARITY = ([("N300_70x45", c) for c in cg.COMBOS] + [("N64_33x17", c) for c in cg.COMBOS] + [(n, "sh3") for n in cc.NAMES]
          + [("inside", c) for c in cg.COMBOS[1:]])


# ---- 1. parity against the dense twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_exp", MODES)
@pytest.mark.parametrize("scene, combo", PARITY, ids=lambda v: str(v))
def test_parity_against_the_dense_twin(scene, combo, fast_exp):
    cc.check_preconditions()
    kw, gimg = _camera_scene(scene, combo) if scene in cc.NAMES else _small(scene, combo)
    ref = cg.dense_camera_reference((scene, combo), kw, gimg)
    out = run(kw, gimg, fast_exp=fast_exp)
    cg.assert_rule3(out["camera"], ref, f"{scene} {combo} fast_exp={fast_exp}")
    cg.assert_unused_columns_zero(out["camera"], scene)
    if scene in cc.INSIDE:
        fa = cc.check_preconditions()[scene]
        assert fa["near"] >= 50 and fa["xclamp"] >= 10 and fa["yclamp"] >= 10 and fa["max_radius"] >= 200     # they all feed the sum


# ---- 2. the option changes nothing else ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_exp", MODES)
@pytest.mark.parametrize("combo", cg.COMBOS)
def test_per_gaussian_gradients_and_image_are_bit_identical_to_the_option_off(combo, fast_exp):
    kw, gimg = _small("N300_70x45", combo)
    on, off = run(kw, gimg, fast_exp=fast_exp), run(kw, gimg, camera_grad=False, fast_exp=fast_exp)
    assert off["camera"] is None
    assert np.array_equal(_bits(on["image"]), _bits(off["image"])) and torch.equal(on["radii"], off["radii"])
    assert set(on["grads"]) == set(off["grads"])
    for n in on["grads"]:
        assert np.abs(off["grads"][n].cpu().numpy()).max() > 0 or n == "means2D", n
        assert np.array_equal(_bits(on["grads"][n]), _bits(off["grads"][n])), n


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------------
def test_two_backward_calls_give_the_same_bits():
    kw, gimg = _camera_scene("inside", "sh3")
    first, again = run(kw, gimg), run(kw, gimg)
    for n in cg.NAMES:
        assert np.abs(first["camera"][n]).max() > 0
        assert np.array_equal(first["camera"][n].view(np.uint32), again["camera"][n].view(np.uint32)), n


def test_backward_twice_through_one_graph_gives_the_same_bits():
    dev = torch.device(DEV)
    kw, gimg = _small("N300_70x45", "sh3")
    t = {k: (v.detach().to(dev).clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
    cam = {n: t[n].requires_grad_(True) for n in cg.NAMES}
    rs = GaussianRasterizationSettings(t["H"], t["W"], t["tanfovx"], t["tanfovy"], t["bg"], 1.0, cam["viewmatrix"], cam["projmatrix"], 3,
                                       cam["campos"], False, False, False)
    color, _ = GaussianRasterizer(rs, options={"camera_grad": True})(means3D=t["means3D"], means2D=torch.zeros(300, 3, device=dev),
                                                                    opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    loss = (color * gimg.to(dev)).sum()
    a = torch.autograd.grad(loss, list(cam.values()), retain_graph=True)
    b = torch.autograd.grad(loss, list(cam.values()))
    for x, y in zip(a, b):
        assert x.abs().max() > 0 and np.array_equal(_bits(x), _bits(y))


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_edge_counts_against_the_twin(n):
    g = syn.make_gaussians(257, seed=5, extent=(1.0, 0.7, 1.0), log_scale_mean=math.log(0.08), opacity_mean=0.5)
    cam = syn.look_at_camera((2.5, -1.0, -4.0), (0.1, 0.0, 0.0), 33, 17, roll_deg=20.0)
    kw = cg.combo_kwargs(g, cam, 33, 17, "sh3", n=n)
    gimg = cg.image_gradient(17, 33)
    out = run(kw, gimg)
    assert int((out["radii"] > 0).sum()) >= 1
    cg.assert_rule3(out["camera"], cg.dense_camera_reference(("edge", n), kw, gimg), f"N={n}")
    cg.assert_unused_columns_zero(out["camera"], f"N={n}")


def test_nothing_to_sum_gives_exact_zeros():
    kw, gimg = _small("N64_33x17", "sh3")
    # an empty model
    empty = cg.combo_kwargs(*cg.small_scene("N64_33x17"), "sh3", n=0)
    out = run(empty, gimg)
    for n in cg.NAMES:
        assert not out["camera"][n].any(), f"N=0 {n}"
    # a camera that sees nothing: it looks away from the scene
    g, _cam, W, H = cg.small_scene("N64_33x17")
    away = syn.look_at_camera((2.5, -1.0, -4.0), (5.0, -2.0, -8.0), W, H, roll_deg=20.0)
    out = run(cg.combo_kwargs(g, away, W, H, "sh3"), gimg)
    assert int((out["radii"] > 0).sum()) == 0
    for n in cg.NAMES:
        assert not out["camera"][n].any(), f"away {n}"
    # a zero image gradient
    out = run(kw, torch.zeros_like(gimg))
    assert int((out["radii"] > 0).sum()) > 0
    for n in cg.NAMES:
        assert not out["camera"][n].any(), f"zero dL/dimage {n}"


# ---- 5. cooperative gather -----------------------------------------------------------------------------------------------------------
def _touched(fn, N):
    """touched[N] of the forward's geom buffer (saved by the autograd node): [N][3] float4 records, [N] uint4 binning records, then
    [N] uint32 instance counts, every sub-buffer 256-byte aligned (lg_host.h carve_geom)."""
    geom = fn.saved_tensors[8]
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731
    off = al(N * 48) + al(N * 16)
    return geom[off:off + 4 * N].view(torch.int32).cpu().numpy()


def test_a_splat_on_every_tile_is_gathered_by_the_whole_wave():
    W, H = cc.W, cc.H
    g = syn.make_gaussians(40, seed=9, extent=(1.0, 0.6, 1.0), log_scale_mean=math.log(0.1), opacity_mean=0.0)
    eye, target = cc.CAMERAS["pitched_rolled"][0], cc.CAMERAS["pitched_rolled"][1]
    with torch.no_grad():
        g._xyz[0] = torch.tensor(target)
        g._scaling[0] = math.log(1.5)
        g._opacity[0] = 6.0
    cam = cc.camera("pitched_rolled")
    kw = cg.combo_kwargs(g, cam, W, H, "sh3")
    gimg = cg.image_gradient(H, W)
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    seen = {}

    def state(fn, radii):       # the forward's own state, before the backward consumes it
        touched = _touched(fn, 40)
        seen["max"] = int(touched.max())
        print(f"touched: max {touched.max()} of {ntiles} tiles; {fn.num_rendered} instances")
        assert int(touched[radii.cpu().numpy() > 0].sum()) == fn.num_rendered      # the layout above is the library's

    out = run(kw, gimg, after_forward=state, options={"sync_free": False})      # the exact forward: num_rendered is the instance count itself
    assert ntiles == 66 and seen["max"] > 48      # LG_COOP_ROWS = 48
    cg.assert_rule3(out["camera"], cg.dense_camera_reference(("coop",), kw, gimg), "one splat on every tile")
    cg.assert_unused_columns_zero(out["camera"], "coop")


# ---- 6. reduction beyond one pass ----------------------------------------------------------------------------------------------------
def test_reduction_beyond_one_pass():
    N, W, H = 70001, 64, 64       # 274 workgroups of 256 Gaussians > the 256 threads of lg_camera_reduce: its strided loop runs twice
    assert (N + 255) // 256 > 256
    g = syn.make_gaussians(N, seed=2, extent=(2.0, 1.2, 2.0), log_scale_mean=math.log(0.02))
    cam = syn.look_at_camera((2.5, -1.0, -4.0), (0.1, 0.0, 0.0), W, H, roll_deg=20.0)
    kw = cg.combo_kwargs(g, cam, W, H, "sh3")
    gimg = cg.image_gradient(H, W)
    a, b = run(kw, gimg), run(kw, gimg)
    for n in cg.NAMES:
        assert np.array_equal(a["camera"][n].view(np.uint32), b["camera"][n].view(np.uint32)), n
    # the translation identity, against the float64 sum of the dL/dmeans3D the same backward returned
    gm = a["grads"]["means3D"].double().cpu().numpy()
    lhs, scale = gm.sum(0), np.abs(gm).sum(0)
    vm, pm = kw["viewmatrix"].double().numpy(), kw["projmatrix"].double().numpy()
    c = {n: a["camera"][n].astype(np.float64) for n in cg.NAMES}
    rhs = vm[:3, :3] @ c["viewmatrix"][3, :3] + pm[:3, :] @ c["projmatrix"][3, :] - c["campos"]
    print(f"identity: lhs {lhs}, rhs {rhs}, |lhs - rhs| / sum|dL/dp| {np.abs(lhs - rhs) / scale}; visible {int((a['radii'] > 0).sum())}")
    assert int((a["radii"] > 0).sum()) > 65536 // 2 and (scale > 0).all()
    assert (np.abs(lhs - rhs) <= 1e-4 * scale).all()
    cg.assert_unused_columns_zero(a["camera"], "70001")


# ---- 7. render(): fused raw path and unfused path ------------------------------------------------------------------------------------
def _render_camera_grads(g, cam, gimg, fuse):
    dev = torch.device(DEV)
    pc = g.to(dev).requires_grad_(True)
    c = cam.to(dev)
    for t in (c.world_view_transform, c.full_proj_transform, c.camera_center):
        t.requires_grad_(True)
    bg = torch.tensor(cg.BG, device=dev)
    pkg = render(c, pc, syn.PipelineParams(), bg, options={"camera_grad": True, "fuse_getters": fuse})
    (pkg["render"] * gimg.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert pc._xyz.grad is not None and pc._xyz.grad.abs().max() > 0
    return {"viewmatrix": c.world_view_transform.grad.cpu().numpy(), "projmatrix": c.full_proj_transform.grad.cpu().numpy(),
            "campos": c.camera_center.grad.cpu().numpy()}


def test_fused_and_unfused_render():
    g, cam, W, H = cg.small_scene("N300_70x45")
    gimg = cg.image_gradient(H, W)
    ref = cg.dense_camera_reference(("N300_70x45", "sh3"), cg.combo_kwargs(g, cam, W, H, "sh3"), gimg)
    fused, unfused = _render_camera_grads(g, cam, gimg, True), _render_camera_grads(g, cam, gimg, False)
    cg.assert_rule3(fused, ref, "render fused")
    cg.assert_rule3(unfused, ref, "render unfused")
    cg.assert_unused_columns_zero(fused, "fused"); cg.assert_unused_columns_zero(unfused, "unfused")
    print("fused and unfused camera gradients bit-equal:", all(np.array_equal(fused[n].view(np.uint32), unfused[n].view(np.uint32)) for n in cg.NAMES))


# ---- 8. PoseCamera end to end ----------------------------------------------------------------------------------------------------------
def test_pose_camera_gradient_reaches_the_six_vector():
    g, base, W, H = cg.small_scene("N300_70x45")
    gimg = cg.image_gradient(H, W)
    xi0 = torch.tensor([0.02, -0.03, 0.015, 0.05, -0.02, 0.04])
    kw = cg.combo_kwargs(g, base, W, H, "sh3")
    ref = {}
    for dd in (torch.float64, torch.float32):
        xi = xi0.to(dd).requires_grad_()
        wvt = base.world_view_transform.to(dd)
        proj = (torch.linalg.inv(base.world_view_transform.double()) @ base.full_proj_transform.double()).float().to(dd)   # PoseCamera's float32 P
        (cg.dense_render(kw, dd, pose.pose_matrices(xi, wvt, proj)) * gimg.to(dd)).sum().backward()
        ref[dd] = xi.grad.numpy().astype(np.float64)
    dev = torch.device(DEV)
    cam = pose.PoseCamera(base).to(dev)
    with torch.no_grad():
        cam.xi.copy_(xi0)
    pc = g.to(dev)
    pkg = render(cam, pc, syn.PipelineParams(), torch.tensor(cg.BG, device=dev), options={"camera_grad": True})
    (pkg["render"] * gimg.to(dev)).sum().backward()
    got = cam.xi.grad.double().cpu().numpy()
    print(f"d/dxi: d64 {ref[torch.float64]}")
    assert np.abs(ref[torch.float64]).min() > 0
    tolerance.assert_rule3(got, ref[torch.float64], ref[torch.float32], "d/dxi")
