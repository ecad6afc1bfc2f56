"""-m gpu: the HIP path (through the drop-in API -> ctypes -> C ABI) against the CPU oracle.

Contract (BASELINE.json north_star): rendered RGB and gradients within 1e-4 rel; hit counts,
significance scores and prune masks bit-identical.  In exact mode (default) the image is in fact
bit-identical to the float oracle; we assert the stronger property where it holds.
"""
import math

import numpy as np
import pytest
import torch

import common
import tolerance
from common import syn
from common import to_numpy as _np
from oracle import oracle

pytestmark = pytest.mark.gpu

# scenes on which even the float32 ORACLE meets the element-wise bound |a-b| <= 1e-4|b| + 2e-5 max|b| against the float64 one
# (measured on CPU: worst ratio 0.30 over all gradients; case 0 reaches 1.56 on scales/rotations, cases 1 and 7 8-1600):
# there the HIP path must meet it too
WELL_CONDITIONED = (2, 3, 4, 5, 6)
TOL = 1e-4  # north_star tolerance for floating-point outputs (relative to tensor max)

CASES = [
    # N, W, H, seed, log-scale mean, opacity mean, extent, sh degree, precolor, precov
    dict(N=10000, W=256, H=256, seed=1, scale=0.004, opm=-1.0, ext=(4, 2.25, 4), deg=3),
    dict(N=3000, W=200, H=120, seed=2, scale=0.05, opm=1.0, ext=(2, 1.2, 2), deg=3),          # saturating pixels
    dict(N=800, W=128, H=96, seed=3, scale=0.3, opm=2.0, ext=(2, 1, 2), deg=2),               # huge splats, early stop
    dict(N=2000, W=161, H=83, seed=4, scale=0.02, opm=-3.0, ext=(3, 2, 3), deg=1),            # ragged image size
    dict(N=1500, W=96, H=64, seed=5, scale=0.03, opm=0.0, ext=(2, 1, 2), deg=0, precolor=True),
    dict(N=1500, W=96, H=64, seed=6, scale=0.03, opm=0.0, ext=(2, 1, 2), deg=3, precov=True),
    dict(N=300, W=320, H=240, seed=7, scale=0.6, opm=-1.5, ext=(2, 1, 2), deg=3),            # screen-filling splats: >48 tile instances each (cooperative row gather in K9)
    dict(N=1500, W=100, H=100, seed=8, scale=0.05, opm=0.5, ext=(2, 1, 2), deg=3, aniso=True),  # needle-like splats: ill-conditioned conics fall back to the full rectangle
]


def _scene(c):
    g = syn.make_gaussians(c["N"], seed=c["seed"], log_scale_mean=math.log(c["scale"]), opacity_mean=c["opm"],
                           extent=c["ext"], log_scale_std=0.9)
    if c.get("aniso"):
        g._scaling[:, 0] += 3.0
        g._scaling[:, 1] -= 2.0
    cam = syn.orbit_camera(1, 5, c["W"], c["H"], radius=5.0)
    pre = torch.rand(c["N"], 3, generator=torch.Generator().manual_seed(7)) if c.get("precolor") else None
    return common.scene_kwargs(g, cam, c["W"], c["H"], deg=c["deg"], precolor=pre, precov=c.get("precov", False),
                               bg=(0.1, 0.2, 0.3), as_torch=True)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c['N']}_{c['W']}x{c['H']}_d{c['deg']}")
def test_forward_count_parity(case):
    import gpu_common
    kw = _scene(case)
    ref = oracle.forward(count=True, **_np(kw))
    out = gpu_common.hip_forward_backward(kw, count=True)
    assert np.array_equal(out["radii"], ref.radii)
    assert gpu_common.rel_err(out["color"], ref.color) <= TOL
    assert np.array_equal(out["count"], ref.count), f"hit counts differ in {np.count_nonzero(out['count'] != ref.count)} Gaussians"
    assert np.array_equal(out["score"].view(np.uint32), ref.score.view(np.uint32)), "significance score not bit-identical"
    # exact mode: the image itself is bit-identical to the float oracle
    assert np.array_equal(out["color"].view(np.uint32), ref.color.view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c['N']}_{c['W']}x{c['H']}_d{c['deg']}")
def test_backward_parity(case):
    """Gradients vs the float64 oracle.  Tolerance: 1e-4 relative (north_star), widened only where
    float32 arithmetic of the published algorithm itself cannot reach it -- measured as the error
    of the float32 ORACLE against the float64 one on the same inputs (T = T/(1-alpha) replay and the
    conic chain amplify rounding); the HIP path must be within 3x of that fp32 noise floor."""
    import gpu_common
    kw = _scene(case)
    gimg = np.random.RandomState(11).randn(3, case["H"], case["W"]).astype(np.float32)
    ref32 = oracle.forward(**_np(kw)); g32 = oracle.backward(ref32, gimg)
    ref64 = oracle.forward(dtype=np.float64, **_np(kw)); g64 = oracle.backward(ref64, gimg)
    out = gpu_common.hip_forward_backward(kw, grad_image=gimg)
    assert gpu_common.rel_err(out["color"], ref32.color) <= TOL
    gpu_common.assert_backward_parity(out["grads"], g32, g64, well_conditioned=CASES.index(case) in WELL_CONDITIONED)


def test_render_equals_count_render_image():
    """render() defaults to the hardware-exp training variant; with fast_exp off it is the same
    canonical arithmetic as count_render() and the images are bit-identical."""
    import gpu_common
    from lightgaussian_amd import rasterizer
    kw = _scene(CASES[1])
    b = gpu_common.hip_forward_backward(kw, count=True)
    a = gpu_common.hip_forward_backward(kw, count=False)
    assert gpu_common.rel_err(a["color"], b["color"]) <= 1e-5 and np.array_equal(a["radii"], b["radii"])
    rasterizer.set_option("fast_exp", False)
    try:
        a = gpu_common.hip_forward_backward(kw, count=False)
    finally:
        rasterizer.set_option("fast_exp", True)
    assert np.array_equal(a["color"], b["color"])


def test_backward_parity_canonical_arithmetic():
    """Same gradient check with fast_exp off (canonical exp / IEEE division in the backward)."""
    import gpu_common
    from lightgaussian_amd import rasterizer
    rasterizer.set_option("fast_exp", False)
    try:
        test_backward_parity(CASES[1])
        test_backward_parity(CASES[2])
    finally:
        rasterizer.set_option("fast_exp", True)


@pytest.mark.parametrize("case_id", [2, 0, 6])
def test_keys_beyond_64_bits_give_the_same_order(case_id):
    """When tile | depth | id exceed 64 bits (6 M Gaussians at 3840x2160, 20 M at 1080p) the lowest depth bits are left out of the
    stored key and lg_tile_ranges completes the order from the full depth in the binning record (r2 fell back to a hipCUB pair
    sort there, without the bounded forward).  option narrow_key lays the key out as if only 40 bits were available, which drops
    depth bits on small scenes too: same (tile, depth, id) order => bit-identical outputs and gradients, in the exact and the
    bounded forward."""
    import os
    import gpu_common
    from lightgaussian_amd import rasterizer
    case = CASES[case_id]
    gimg = np.random.RandomState(5).randn(3, case["H"], case["W"]).astype(np.float32)
    res = {}
    for mode in ("full", "narrow", "narrow_bounded"):
        with rasterizer.options(narrow_key=mode != "full", sync_free="validated" if mode == "narrow_bounded" else False):
            res[mode] = (gpu_common.hip_forward_backward(_scene(case), count=True),
                         gpu_common.hip_forward_backward(_scene(case), grad_image=gimg),
                         gpu_common.hip_forward_backward(_scene(case), count=True))      # (second view of the shape: bounded when enabled)
    a = res["full"]
    ref = oracle.forward(count=True, **_np(_scene(case)))
    assert np.array_equal(a[0]["count"], ref.count) and np.array_equal(a[0]["color"].view(np.uint32), ref.color.view(np.uint32))
    for mode in ("narrow", "narrow_bounded"):
        b = res[mode]
        for k in (0, 2):
            assert np.array_equal(a[0]["count"], b[k]["count"]) and np.array_equal(a[0]["color"], b[k]["color"]), (mode, k)
            assert np.array_equal(a[0]["score"], b[k]["score"]) and np.array_equal(a[0]["radii"], b[k]["radii"]), (mode, k)
        for name in a[1]["grads"]:
            assert np.array_equal(a[1]["grads"][name], b[1]["grads"][name]), (mode, name)   # rows + fixed-order gather: deterministic


def test_a_slab_of_coplanar_splats_on_few_tiles_is_ordered_by_the_wave_level_run_sort():
    """20 000 splats at ONE depth on a handful of tiles: every tile list is a single run of equal sorted bits, thousands of
    entries long.  r2 finished such runs with one thread (merge sort; 14.8 ms when the runs got long); lg_tile_ranges now hands
    runs beyond 32 entries to the whole wave (stable LSD counting sort on the low depth bits).  Counts, scores and image must
    equal the oracle bit for bit, with depth bits dropped from the sort, with every bit sorted, and with the narrow key."""
    import os
    import gpu_common
    N, W, H = 20000, 64, 48
    g = syn.make_gaussians(N, seed=33, log_scale_mean=math.log(0.03), opacity_mean=-4.0, extent=(0.35, 0.25, 0.0))
    cam = syn.orbit_camera(0, 5, W, H, radius=5.0)              # camera 0 looks along +z from (0, 0, -5): the plane z = 0 is at depth 5
    gen = torch.Generator().manual_seed(4)
    g._xyz[:, 2] = 0.0
    g._xyz[::7, 2] = 3e-6 * torch.randn(g._xyz[::7].shape[0], generator=gen)        # a few within the dropped bits of the others
    kw = common.scene_kwargs(g, cam, W, H, deg=1, bg=(0.1, 0.2, 0.3), as_torch=True)
    ref = oracle.forward(count=True, **_np(kw))
    assert ref.num_rendered > 20000
    from lightgaussian_amd import rasterizer
    for env in ({}, {"sort_all_bits": True}, {"narrow_key": True}):
        with rasterizer.options(**env):
            out = gpu_common.hip_forward_backward(kw, count=True)
        assert np.array_equal(out["count"], ref.count), env
        assert np.array_equal(out["score"].view(np.uint32), ref.score.view(np.uint32)), env
        assert np.array_equal(out["color"].view(np.uint32), ref.color.view(np.uint32)), env


@pytest.mark.parametrize("jitter", [0.0, 3e-6, 1e-4])
def test_sort_with_dropped_depth_bits_gives_the_full_order(jitter):
    """The radix sort skips the lowest depth bits when that saves an 8-bit pass and lg_tile_ranges finishes runs of
    equal sorted bits by stable insertion.  A wall of Gaussians at (almost) one depth makes such runs long: hit counts
    and scores must still be bit-identical to the oracle and to a sort over all bits (option sort_all_bits)."""
    import os
    import gpu_common
    N, W, H = 6000, 160, 96
    g = syn.make_gaussians(N, seed=21, log_scale_mean=math.log(0.05), opacity_mean=-0.5, extent=(2, 1.2, 2))
    cam = syn.orbit_camera(0, 5, W, H, radius=5.0)
    # camera 0 sits at (0, 0, -5) looking along +z: put every Gaussian on the plane z = 0 (+ relative jitter)
    gen = torch.Generator().manual_seed(3)
    g._xyz[:, 2] = jitter * 5.0 * torch.randn(N, generator=gen)
    kw = common.scene_kwargs(g, cam, W, H, deg=3, bg=(0.1, 0.2, 0.3), as_torch=True)
    ref = oracle.forward(count=True, **_np(kw))
    outs = {}
    from lightgaussian_amd import rasterizer
    for mode in ("drop", "all"):
        with rasterizer.options(sort_all_bits=mode == "all"):
            outs[mode] = gpu_common.hip_forward_backward(kw, count=True)
    for mode, out in outs.items():
        assert np.array_equal(out["count"], ref.count), mode
        assert np.array_equal(out["score"].view(np.uint32), ref.score.view(np.uint32)), mode
        assert np.array_equal(out["color"].view(np.uint32), ref.color.view(np.uint32)), mode
    assert int(ref.count.sum()) > 10000


def test_gradients_are_run_to_run_deterministic():
    import gpu_common
    gimg = np.random.RandomState(6).randn(3, CASES[1]["H"], CASES[1]["W"]).astype(np.float32)
    a = gpu_common.hip_forward_backward(_scene(CASES[1]), grad_image=gimg)
    b = gpu_common.hip_forward_backward(_scene(CASES[1]), grad_image=gimg)
    for name in a["grads"]:
        assert np.array_equal(a["grads"][name], b["grads"][name]), name


def test_packed_wave_reduction():
    """The permlane-swap reduction of the backward blend: 9 values x 64 lanes -> 9 sums."""
    import ctypes as C
    from lightgaussian_amd import _lib
    lib = _lib.load()
    x = torch.randn(64, 9, generator=torch.Generator().manual_seed(3))
    xd = x.cuda().contiguous(); out = torch.zeros(9, device="cuda")
    _lib.check(lib.lg_debug_reduce9(C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    ref = x.double().sum(0)
    assert np.allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5), (out.cpu().numpy(), ref.numpy())


def test_empty_and_all_culled():
    import gpu_common
    c = dict(N=64, W=64, H=48, seed=9, scale=0.05, opm=0.0, ext=(1, 1, 1), deg=3)
    kw = _scene(c)
    # everything behind the camera
    kw_b = dict(kw); kw_b["means3D"] = kw["means3D"] * 0 + torch.tensor([0.0, 0.0, -50.0])
    out = gpu_common.hip_forward_backward(kw_b, count=True, grad_image=None)
    assert (out["radii"] == 0).all() and (out["count"] == 0).all()
    bg = kw["bg"].numpy()
    assert np.allclose(out["color"], bg[:, None, None] * np.ones_like(out["color"]))
    # N = 0
    kw_e = {k: (v[:0] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == c["N"] else v) for k, v in kw.items()}
    out = gpu_common.hip_forward_backward(kw_e, count=True)
    assert out["radii"].shape == (0,) and np.allclose(out["color"], bg[:, None, None] * np.ones_like(out["color"]))


def test_invalid_argument_combinations_raise():
    import gpu_common
    kw = _scene(CASES[4])
    bad = dict(kw); bad["shs"] = torch.zeros(kw["means3D"].shape[0], 16, 3)
    with pytest.raises(Exception, match="excatly one"):
        gpu_common.hip_forward_backward(bad)
    bad = dict(kw); bad["cov3D_precomp"] = torch.zeros(kw["means3D"].shape[0], 6)
    with pytest.raises(Exception, match="exactly one"):
        gpu_common.hip_forward_backward(bad)


def test_full_size_properties():
    """1080p, 1M Gaussians (BASELINE configs[1] shape): properties that need no oracle run.
    sum of blend weights + final_T = 1 is checked through a white-on-black render; count/score
    consistency through score == seqsum32(opacity, count) recomputed on the host for a sample."""
    import gpu_common
    W, H, N = 1920, 1080, 1_000_000
    g = syn.make_gaussians(N)
    cam = syn.orbit_camera(0, 200, W, H)
    kw = common.scene_kwargs(g, cam, W, H, deg=3, as_torch=True)
    out = gpu_common.hip_forward_backward(kw, count=True)
    assert np.isfinite(out["color"]).all() and out["color"].min() >= 0.0
    # precomputed white colours on black bg and white bg: C_white - C_black = T_final * 1
    kw_w = dict(kw); kw_w.pop("shs"); kw_w["colors_precomp"] = torch.ones(N, 3)
    blk = gpu_common.hip_forward_backward(kw_w)["color"]
    kw_w["bg"] = torch.ones(3)
    wht = gpu_common.hip_forward_backward(kw_w)["color"]
    T_final = wht - blk
    assert np.all(T_final >= -1e-6) and np.all(T_final <= 1 + 1e-6)
    assert np.allclose(wht, 1.0, atol=2e-5)  # sum(w) + T_final = 1 for unit colours
    # idempotence
    again = gpu_common.hip_forward_backward(kw, count=True)
    assert np.array_equal(again["count"], out["count"]) and np.array_equal(again["color"], out["color"])
    # score consistency on a sample
    op = g.get_opacity.numpy().reshape(-1)
    idx = np.random.RandomState(0).choice(N, 2000, replace=False)
    for i in idx:
        assert np.float32(out["score"][i]).tobytes() == np.float32(oracle.seqsum(op[i], int(out["count"][i]))).tobytes()
    assert ((out["radii"] > 0) | (out["count"] == 0)).all()


def test_sharded_prune_pass_collectives_on_rccl():
    """prune_list_sharded through the real RCCL code path (backend nccl) at world size 1 with the collectives
    forced: int all-reduce, all_to_all_single, all_gather_into_tensor on device tensors.  Must equal the plain loop."""
    import socket
    import torch.distributed as dist
    from lightgaussian_amd import prune as lg_prune
    from lightgaussian_amd.gaussian_renderer import count_render
    dev = torch.device("cuda:0")
    g = syn.make_gaussians(4000, seed=13, log_scale_mean=math.log(0.04), opacity_mean=0.5, extent=(2, 1.2, 2)).to(dev)
    cams = [syn.orbit_camera(k, 5, 96, 64, radius=5.0).to(dev) for k in range(5)]
    bg = torch.zeros(3, device=dev)
    pipe = syn.PipelineParams()
    with torch.no_grad():
        c1, s1 = lg_prune.prune_list(g, cams, pipe, bg)
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        for mode in ("ordered", "allreduce"):
            with torch.no_grad():
                c2, s2 = lg_prune.prune_list_sharded(g, cams, pipe, bg, mode=mode, force_collectives=True)
            assert torch.equal(c1, c2) and torch.equal(s1, s2), mode
    finally:
        dist.destroy_process_group()
    m = lg_prune.prune_mask(0.66, lg_prune.calculate_v_imp_score(g, s1, 0.1))
    assert 0 < int(m.sum()) < 4000


@pytest.mark.parametrize("streams", [1, 2, 3, 5])
def test_significance_pass_with_views_in_flight_equals_the_sequential_loop(streams):
    """prune_list_sharded renders several views concurrently (host threads x HIP streams); counts are integers and the
    per-view scores are summed afterwards in the reference's order, so the result is bit-identical to prune_list."""
    from lightgaussian_amd import prune as lg_prune
    dev = torch.device("cuda:0")
    g = syn.make_gaussians(20000, seed=17, log_scale_mean=math.log(0.03), opacity_mean=0.0, extent=(2, 1.2, 2)).to(dev)
    cams = [syn.orbit_camera(k, 11, 160, 96, radius=5.0).to(dev) for k in range(11)]
    bg = torch.zeros(3, device=dev)
    pipe = syn.PipelineParams()
    with torch.no_grad():
        c1, s1 = lg_prune.prune_list(g, cams, pipe, bg)
        c2, s2 = lg_prune.prune_list_sharded(g, cams, pipe, bg, streams=streams)
    assert torch.equal(c1.to(torch.int32), c2.to(torch.int32)) and torch.equal(s1, s2)
    assert int(c1.sum()) > 0


def test_backward_over_views_equals_the_one_by_one_loop():
    """parallel.backward_over_views (camera batch > 1: views rendered concurrently on their own streams, per-thread leaf
    views of the parameters) accumulates the same gradients as rendering the views one after the other."""
    from lightgaussian_amd import parallel
    from lightgaussian_amd.gaussian_renderer import render
    dev = torch.device("cuda:0")
    W, H, N, V = 160, 96, 8000, 7
    cams = [syn.orbit_camera(k, V, W, H, radius=5.0).to(dev) for k in range(V)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev); pipe = syn.PipelineParams()
    gen = torch.Generator().manual_seed(5)
    targets = [torch.rand(3, H, W, generator=gen).to(dev) for _ in range(V)]
    loss_fn = lambda img, gt: (img - gt).abs().mean()
    mk = lambda: syn.make_gaussians(N, seed=23, log_scale_mean=math.log(0.04), opacity_mean=0.0, extent=(2, 1.2, 2)).to(dev).requires_grad_(True)
    a = mk()
    seq_losses = []
    for k in range(V):
        l = loss_fn(render(cams[k], a, pipe, bg)["render"], targets[k]); l.backward(); seq_losses.append(float(l.detach()))
    for streams in (1, 3):
        b = mk()
        losses = parallel.backward_over_views(b, cams, targets, pipe, bg, loss_fn, streams=streams)
        assert [float(x) for x in losses] == seq_losses                      # every view's loss is bit-identical
        for n in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
            ga, gb = getattr(a, n).grad, getattr(b, n).grad
            assert gb is not None and float((ga - gb).abs().max()) <= 1e-5 * float(ga.abs().max()) + 1e-12, (streams, n)
    # same number of streams twice: bit-identical (fixed summation order)
    c = mk(); parallel.backward_over_views(c, cams, targets, pipe, bg, loss_fn, streams=3)
    assert all(torch.equal(getattr(b, n).grad, getattr(c, n).grad) for n in ("_xyz", "_features_rest", "_opacity"))


@pytest.mark.parametrize("deg", [3, 1, 0])
def test_fused_getters_match_unfused_render(deg):
    """render_fused (activations + cat inside the kernels) vs render() on the same raw parameters:
    image within 1e-5, gradients w.r.t. the RAW parameters within 1e-4 (different exp/sigmoid implementations only)."""
    import gpu_common
    from lightgaussian_amd import rasterizer
    from lightgaussian_amd.gaussian_renderer import render as render_auto, render_fused, _render_unfused as render
    assert rasterizer._OPTIONS["fuse_getters"] is True
    dev = torch.device("cuda:0")
    W, H, N = 200, 120, 5000
    cam = syn.orbit_camera(1, 5, W, H, radius=5.0).to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = syn.PipelineParams()
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(2)).to(dev)
    outs = []
    for fn in (render, render_fused, render_auto):
        g = syn.make_gaussians(N, sh_degree=deg, seed=4, log_scale_mean=math.log(0.04), opacity_mean=0.5, extent=(2, 1.2, 2)).to(dev)
        g.requires_grad_(True)
        pkg = fn(cam, g, pipe, bg)
        (pkg["render"] * gimg).sum().backward()
        outs.append((pkg["render"].detach().cpu().numpy(), pkg["radii"].cpu().numpy(), pkg["viewspace_points"].grad.cpu().numpy(),
                     [t.grad.cpu().numpy() if t.grad is not None else None
                      for t in (g._xyz, g._features_dc, g._features_rest, g._scaling, g._rotation, g._opacity)]))
    (ia, ra, va, ga), (ib, rb, vb, gb), (ic, rc, vc, gc) = outs
    # render() itself takes the fused path for a model with the reference's activations (option fuse_getters):
    # bit-identical to the explicit render_fused call
    assert np.array_equal(ic, ib) and np.array_equal(vc, vb) and all(
        (x is None and y is None) or np.array_equal(x, y) for x, y in zip(gb, gc))
    # round 2: the in-kernel activations reproduce torch.exp / torch.sigmoid / F.normalize bit for bit on this GPU
    # (tools/activation_probe.py), so the forward of the fused path IS the literal path's forward: radii, image and the
    # screen-space gradient (which involves no activation) are bit-identical
    assert np.array_equal(ra, rb)
    assert np.array_equal(ia, ib), f"image differs: {gpu_common.rel_err(ib, ia):.3e}"
    assert gpu_common.rel_err(vb, va) <= 1e-6
    for name, x, y in zip(("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"), ga, gb):
        if x is None or x.size == 0:
            continue
        assert y is not None, name
        assert gpu_common.rel_err(y, x) <= TOL, f"{name}: {gpu_common.rel_err(y, x):.3e}"


def test_fuse_getters_option_and_foreign_models_keep_the_literal_pattern():
    """set_option('fuse_getters', False) and models without the reference's activation attributes go through the
    reference's literal getter pattern (bit-identical to _render_unfused)."""
    from lightgaussian_amd import rasterizer
    from lightgaussian_amd.gaussian_renderer import render, _render_unfused, _has_reference_getters
    from lightgaussian_amd.prune import _FrozenGetters
    dev = torch.device("cuda:0")
    cam = syn.orbit_camera(0, 5, 160, 96, radius=5.0).to(dev)
    bg = torch.zeros(3, device=dev); pipe = syn.PipelineParams()
    g = syn.make_gaussians(3000, sh_degree=3, seed=9, log_scale_mean=math.log(0.04)).to(dev)
    ref = _render_unfused(cam, g, pipe, bg)["render"]
    assert _has_reference_getters(g) and not _has_reference_getters(_FrozenGetters(g))
    assert torch.equal(render(cam, _FrozenGetters(g), pipe, bg)["render"], ref)
    rasterizer.set_option("fuse_getters", False)
    try:
        assert torch.equal(render(cam, g, pipe, bg)["render"], ref)
    finally:
        rasterizer.set_option("fuse_getters", True)
    fused = render(cam, g, pipe, bg)["render"]
    assert float((fused - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("deg", [3, 2, 1, 0])
def test_direct_and_lds_staged_sh_reads_agree(deg, monkeypatch):
    """K1 reads SH rows with dword-aligned dwordx4 loads (rows of 3M / 3(M-1) floats are not 16-byte aligned in
    general); the LDS-staged reader (option k1_lds) must give bit-identical images, for activated tensors and for the raw
    dc/rest pair, including the last rows of the tensors (N not a multiple of 64)."""
    from lightgaussian_amd.gaussian_renderer import render_fused, _render_unfused
    dev = torch.device("cuda:0")
    cam = syn.orbit_camera(2, 7, 176, 112, radius=5.0).to(dev)
    bg = torch.tensor([0.3, 0.1, 0.2], device=dev); pipe = syn.PipelineParams()
    g = syn.make_gaussians(4099, sh_degree=deg, seed=11, log_scale_mean=math.log(0.04), rest_std=0.3).to(dev)
    from lightgaussian_amd import rasterizer
    for fn in (_render_unfused, render_fused):
        a = fn(cam, g, pipe, bg)["render"].clone()
        with rasterizer.options(k1_lds=True):
            b = fn(cam, g, pipe, bg)["render"].clone()
        assert torch.equal(a, b), fn.__name__
        assert float(a.abs().max()) > 0


def test_weight_policies_alpha_and_alpha_t():
    """The float per-hit weights (ALPHA, ALPHA_T) are order-dependent sums even in the reference; tolerance 1e-4.
    ONE gives score == count exactly."""
    import gpu_common
    from lightgaussian_amd import _lib, rasterizer
    kw = _scene(CASES[1])
    try:
        for pol, opol in ((_lib.WEIGHT_ONE, oracle.W_ONE), (_lib.WEIGHT_ALPHA, oracle.W_ALPHA), (_lib.WEIGHT_ALPHA_T, oracle.W_ALPHA_T)):
            rasterizer.set_option("weight_policy", pol)
            out = gpu_common.hip_forward_backward(kw, count=True)
            ref = oracle.forward(count=True, weight_policy=opol, **_np(kw))
            assert np.array_equal(out["count"], ref.count)
            if pol == _lib.WEIGHT_ONE:
                assert np.array_equal(out["score"], ref.count.astype(np.float32))
            else:
                assert gpu_common.rel_err(out["score"], ref.score) <= TOL
    finally:
        rasterizer.set_option("weight_policy", _lib.WEIGHT_OPACITY)


def test_debug_flag_prefiltered_error_and_stale_count_api():
    import gpu_common
    from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    kw = _scene(CASES[4])
    a = gpu_common.hip_forward_backward(kw, count=True)
    b = gpu_common.hip_forward_backward(kw, count=True, debug=True)     # debug: sync + check after every kernel
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["color"], b["color"])
    dev = torch.device("cuda:0")
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    N = t["means3D"].shape[0]

    def settings(**over):
        base = dict(image_height=t["H"], image_width=t["W"], tanfovx=t["tanfovx"], tanfovy=t["tanfovy"], bg=t["bg"], scale_modifier=1.0,
                    viewmatrix=t["viewmatrix"], projmatrix=t["projmatrix"], sh_degree=t["sh_degree"], campos=t["campos"],
                    prefiltered=False, debug=False, f_count=False)
        base.update(over)
        return GaussianRasterizationSettings(**base)
    args = dict(means3D=t["means3D"], means2D=torch.zeros(N, 3, device=dev), opacities=t["opacities"], colors_precomp=t["colors_precomp"],
                scales=t["scales"], rotations=t["rotations"])
    # stale API of gaussian_renderer/gaussian_count.py:69,112
    cnt, score, color, radii = GaussianRasterizer(settings(), f_count=True).forward_counter(**args)
    assert np.array_equal(cnt.cpu().numpy(), a["count"]) and np.array_equal(score.cpu().numpy(), a["score"])
    # prefiltered=True promises that nothing fails the frustum test: a Gaussian behind the camera is an error
    bad = dict(args); bad["means3D"] = t["means3D"].clone(); bad["means3D"][0] = t["campos"] - 10.0 * (t["means3D"].mean(0) - t["campos"])
    with pytest.raises(RuntimeError, match="filtered"):
        GaussianRasterizer(settings(prefiltered=True))(**bad)
    # markVisible: frustum (near plane) test only
    vis = GaussianRasterizer(settings()).markVisible(bad["means3D"])
    assert not bool(vis[0]) and bool(vis[1:].all())


def test_full_size_prune_mask_parity_at_a_ranks_share_of_c4():
    """BASELINE configs[3] at the size one rank sees it: 3 M Gaussians, 1080p, 25 views (200 cameras / 8 GPUs) through
    prune_list_sharded with the RCCL collectives FORCED at world size 1 (int32 count all-reduce, round-wise ordered all_to_all of
    the scores, all_gather): summed hit counts and the view-ordered fp32 score sums bit-identical to the oracle's sequential sum in
    the reference's order (prune.py:144-155: pop from the END of the list), prune mask (v_pow 0.1, prune_ratio 0.66) Hamming
    distance 0.  (r4 verdict, missing #4: the round-4 test summed three views through the single-process loop.)"""
    import socket
    import torch.distributed as dist
    from lightgaussian_amd import prune as lg_prune
    dev = torch.device("cuda:0")
    N, W, H, V = 3_000_000, 1920, 1080, 25
    g = syn.make_gaussians(N)
    cams = [syn.orbit_camera(8 * k + 3, 200, W, H) for k in range(V)]          # rank 3's share of the 200-camera orbit
    # activations evaluated ONCE on the CPU so that oracle and HIP path see identical inputs
    with torch.no_grad():
        frozen = syn.SyntheticGaussians(g.get_xyz, g._features_dc, g._features_rest, g.get_scaling, g.get_rotation, g.get_opacity, 3, 3)
    class _PC:
        get_xyz = frozen._xyz.to(dev); get_scaling = frozen._scaling.to(dev); get_rotation = frozen._rotation.to(dev)
        get_opacity = frozen._opacity.to(dev); get_features = torch.cat((frozen._features_dc, frozen._features_rest), 1).to(dev)
        active_sh_degree = 3; max_sh_degree = 3
    bg = torch.zeros(3, device=dev)
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        st = {}
        with torch.no_grad():
            cnt, imp = lg_prune.prune_list_sharded(_PC, [c.to(dev) for c in cams], syn.PipelineParams(), bg, force_collectives=True, stats=st)
        assert st.get("collectives", 0) >= 3, st                       # the exchange really ran
    finally:
        dist.destroy_process_group()
    shs = _PC.get_features.cpu().numpy()
    cnt_o = None
    for cam in cams[::-1]:                       # the reference loop pops from the end
        kw = dict(means3D=frozen._xyz.numpy(), opacities=frozen._opacity.numpy(), W=W, H=H, tanfovx=math.tan(cam.FoVx * 0.5),
                  tanfovy=math.tan(cam.FoVy * 0.5), bg=np.zeros(3, np.float32), viewmatrix=cam.world_view_transform.numpy(),
                  projmatrix=cam.full_proj_transform.numpy(), campos=cam.camera_center.numpy(), sh_degree=3,
                  shs=shs, scales=frozen._scaling.numpy(), rotations=frozen._rotation.numpy())
        f = oracle.forward(count=True, **kw)
        if cnt_o is None:
            cnt_o, imp_o = f.count.copy(), f.score.copy()
        else:
            cnt_o += f.count; imp_o += f.score
    assert np.array_equal(cnt.cpu().numpy(), cnt_o)
    assert np.array_equal(imp.cpu().numpy().view(np.uint32), imp_o.view(np.uint32))
    v = lg_prune.calculate_v_imp_score(_PC, imp, 0.1)
    mask = lg_prune.prune_mask(0.66, v).cpu().numpy()
    v_o = lg_prune.calculate_v_imp_score(_PC, torch.from_numpy(imp_o).to(dev), 0.1)
    mask_o = lg_prune.prune_mask(0.66, v_o).cpu().numpy()
    assert int(np.count_nonzero(mask != mask_o)) == 0
    assert 0.6 < mask.mean() < 0.8


def test_render_pipe_alternates_match():
    """PipelineParams.convert_SHs_python / compute_cov3D_python (arguments/__init__.py:72-77): the four input
    variants of render() (shs vs colors_precomp, scales+rotations vs cov3D_precomp) give the same image and radii,
    and gradients reach the raw parameters in every variant (gaussian_renderer/__init__.py:79-99)."""
    import gpu_common
    from lightgaussian_amd.gaussian_renderer import render
    dev = torch.device("cuda:0")
    W, H, N = 160, 120, 3000
    cam = syn.orbit_camera(2, 7, W, H, radius=5.0).to(dev)
    bg = torch.tensor([0.2, 0.1, 0.0], device=dev)
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    ref = None
    for sh_py in (False, True):
        for cov_py in (False, True):
            g = syn.make_gaussians(N, seed=9, log_scale_mean=math.log(0.05), opacity_mean=0.0, extent=(2, 1.2, 2)).to(dev)
            g.requires_grad_(True)
            pipe = syn.PipelineParams(convert_SHs_python=sh_py, compute_cov3D_python=cov_py)
            pkg = render(cam, g, pipe, bg)
            (pkg["render"] * gimg).sum().backward()
            out = (pkg["render"].detach().cpu().numpy(), pkg["radii"].cpu().numpy(), g._xyz.grad.cpu().numpy(),
                   g._features_dc.grad.cpu().numpy(), g._scaling.grad.cpu().numpy(), pkg["viewspace_points"].grad.cpu().numpy())
            assert set(pkg.keys()) == {"render", "viewspace_points", "visibility_filter", "radii"}
            assert pkg["visibility_filter"].dtype == torch.bool
            # gaussian_renderer/__init__.py:121; the fused path reads it in place from the forward's geom buffer (K1's visibility bytes)
            assert torch.equal(pkg["visibility_filter"], pkg["radii"] > 0) and bool(pkg["visibility_filter"].any())
            # every view gets its own screen-space leaf (its own .grad) although the leaves share one zero buffer
            pkg2 = render(cam, g, pipe, bg)
            assert pkg2["viewspace_points"] is not pkg["viewspace_points"] and pkg2["viewspace_points"].grad is None
            assert float(pkg2["viewspace_points"].abs().sum()) == 0.0 and pkg["viewspace_points"].grad is not None
            if ref is None:
                ref = out
                continue
            assert np.array_equal(out[1], ref[1])
            assert gpu_common.rel_err(out[0], ref[0]) <= 1e-5
            for a, b in zip(out[2:], ref[2:]):
                assert gpu_common.rel_err(a, b) <= TOL


def test_fuzz_count_and_image_parity():
    """Seeded sweep over scene statistics (size, splat scale, opacity, anisotropy, image shape, SH degree, background):
    hit counts, scores, radii and the count-render image must be bit-identical to the float oracle every time; the
    training render must agree to 1e-5 (its include/exclude decisions are guarded to equal the canonical path's)."""
    import gpu_common
    rs = np.random.RandomState(2025)
    for trial in range(14):
        N = int(rs.choice([200, 1500, 6000]))
        W, H = int(rs.randint(40, 260)), int(rs.randint(40, 200))
        deg = int(rs.randint(0, 4))
        c = dict(N=N, W=W, H=H, seed=100 + trial, scale=float(np.exp(rs.uniform(np.log(0.003), np.log(0.4)))),
                 opm=float(rs.uniform(-4.0, 3.0)), ext=(float(rs.uniform(0.5, 3)), float(rs.uniform(0.5, 2)), float(rs.uniform(0.5, 3))),
                 deg=deg, aniso=bool(rs.rand() < 0.3), precov=bool(rs.rand() < 0.2))
        kw = _scene(c)
        kw["bg"] = torch.tensor(rs.rand(3).astype(np.float32))
        ref = oracle.forward(count=True, **_np(kw))
        out = gpu_common.hip_forward_backward(kw, count=True)
        tag = f"trial {trial}: {c}"
        assert np.array_equal(out["radii"], ref.radii), tag
        assert np.array_equal(out["count"], ref.count), tag
        assert np.array_equal(out["score"].view(np.uint32), ref.score.view(np.uint32)), tag
        assert np.array_equal(out["color"].view(np.uint32), ref.color.view(np.uint32)), tag
        fast = gpu_common.hip_forward_backward(kw, count=False)
        assert np.abs(fast["color"] - ref.color).max() <= 1e-5, tag


def test_skip_color_leaves_counts_and_scores_untouched():
    """LG_FLAG_SKIP_COLOR (significance-only pass): same counts / scores / radii bit for bit, image not evaluated."""
    import gpu_common
    from lightgaussian_amd import rasterizer
    kw = _scene(CASES[0])
    a = gpu_common.hip_forward_backward(kw, count=True)
    rasterizer.set_option("skip_color_in_count", True)
    try:
        b = gpu_common.hip_forward_backward(kw, count=True)
        c = gpu_common.hip_forward_backward(kw, count=False)     # render() is never affected
    finally:
        rasterizer.set_option("skip_color_in_count", False)
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["score"], b["score"]) and np.array_equal(a["radii"], b["radii"])
    assert gpu_common.rel_err(c["color"], a["color"]) <= 1e-5


@pytest.mark.parametrize("scale,aspect", [(0.01, 1.5), (0.03, 1.5), (0.03, 0.8), (0.1, 1.2)])
def test_elongated_diagonal_splats_and_the_block_reach_test(scale, aspect):
    """The blend kernels drop an 8x8 block of a tile instance when the alpha >= 1/255 ELLIPSE cannot reach it (lg_block_hit: two
    clamped 1-D maximisations of the concave exponent over the block, behind the box test).  Elongated splats at random
    rotations -- aspect ratios of e^0.8 ... e^1.5, well conditioned, so culling stays on -- are the scenes where the ellipse
    drops blocks the box keeps.  Nothing that contributes may be lost: counts, scores, radii and the count-render image
    bit-identical to the oracle (which enumerates every pixel of every tile of the 3-sigma square), the training render within
    1e-5, gradients within the north_star tolerance of the float64 oracle."""
    import gpu_common
    N, W, H = 4000, 160, 112
    g = syn.make_gaussians(N, seed=31, log_scale_mean=math.log(scale), log_scale_std=0.2, opacity_mean=0.5, extent=(2, 1.2, 2))
    g._scaling[:, 0] += aspect                                   # one long axis; the random quaternions turn it every way
    kw = common.scene_kwargs(g, syn.orbit_camera(2, 7, W, H, radius=4.5), W, H, deg=2, bg=(0.2, 0.1, 0.0), as_torch=True)
    ref = oracle.forward(count=True, **_np(kw))
    out = gpu_common.hip_forward_backward(kw, count=True)
    assert ref.count.sum() > 10000
    assert np.array_equal(out["radii"], ref.radii)
    assert np.array_equal(out["count"], ref.count)
    assert np.array_equal(out["score"].view(np.uint32), ref.score.view(np.uint32))
    assert np.array_equal(out["color"].view(np.uint32), ref.color.view(np.uint32))
    gimg = np.random.RandomState(5).randn(3, H, W).astype(np.float32)
    ref32 = oracle.forward(**_np(kw)); g32 = oracle.backward(ref32, gimg)
    ref64 = oracle.forward(dtype=np.float64, **_np(kw)); g64 = oracle.backward(ref64, gimg)
    fast = gpu_common.hip_forward_backward(kw, grad_image=gimg)
    assert np.abs(fast["color"] - ref.color).max() <= 1e-5
    for name, gr in fast["grads"].items():
        r = g64[name]
        floor = gpu_common.rel_err(g32[name], r)
        assert gpu_common.rel_err(gr.reshape(r.shape), r) <= tolerance.rule3_bound(floor), name
