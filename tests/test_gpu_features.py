"""-m gpu: lg_blend_features / lg_blend_features_backward (features.blend_features, gaussian_renderer.render_features) against
the CPU oracle, which blends arbitrary precomputed channels three at a time (colors_precomp, unclamped) and whose colors_precomp
gradient is dL/dfeatures.  Canonical mode is pinned bit for bit, hardware-exp mode by the project's element-wise contract."""
import functools
import math

import numpy as np
import pytest
import torch

import common
import gpu_common
from common import bits, syn
from lightgaussian_amd import features as lg_features
from lightgaussian_amd import gaussian_renderer, vectree
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CMAX = 64
CHANNELS = (1, 3, 7, 16, 17, 64)

# name -> (N, W, H, make_gaussians keywords, rasterizer options)
SCENES = {
    "n300_70x45": (300, 70, 45, dict(log_scale_mean=math.log(0.06), opacity_mean=0.0), {}),
    "n64_33x17": (64, 33, 17, dict(log_scale_mean=math.log(0.1), opacity_mean=0.0), {}),
    "n400_48x48_seg64": (400, 48, 48, dict(log_scale_mean=math.log(0.25), opacity_mean=-2.0), {"segment_length": 64}),
    "n400_48x48": (400, 48, 48, dict(log_scale_mean=math.log(0.25), opacity_mean=-2.0), {}),
}
MODES = {"canonical": {"fast_exp": False}, "hardware_exp": {"fast_exp": True}}


def settings(kw, bg):
    return GaussianRasterizationSettings(
        image_height=kw["H"], image_width=kw["W"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"], bg=bg, scale_modifier=1.0,
        viewmatrix=kw["viewmatrix"].to(DEV), projmatrix=kw["projmatrix"].to(DEV), sh_degree=kw["sh_degree"], campos=kw["campos"].to(DEV),
        prefiltered=False, debug=False, f_count=False)


@functools.lru_cache(maxsize=None)
def scene(name):
    """Inputs and the oracle's results for all 64 channels of a scene, computed once and shared (read-only) by every test."""
    N, W, H, gkw, _opts = SCENES[name]
    g = syn.make_gaussians(N, seed=3, extent=(1.5, 1.0, 1.5), **gkw)
    cam = syn.orbit_camera(1, 7, W, H, radius=4.0)
    gen = torch.Generator().manual_seed(17)
    F = torch.randn(N, CMAX, generator=gen)                              # negative values included
    bgf = torch.randn(CMAX, generator=gen)
    dout = torch.randn(CMAX, H, W, generator=gen)
    colors = torch.rand(N, 3, generator=gen)
    Fp = torch.cat([F, torch.zeros(N, 2)], 1).numpy()                    # 66 columns: 22 whole triples
    bgp = torch.cat([bgf, torch.zeros(2)]).numpy()
    dp = torch.cat([dout, torch.zeros(2, H, W)]).numpy()
    out0 = np.zeros((CMAX + 2, H, W), np.float32); outbg = np.zeros_like(out0); dF = np.zeros((N, CMAX + 2), np.float32)
    radii = None
    for c0 in range(0, CMAX, 3):
        kw = common.scene_kwargs(g, cam, W, H, precolor=torch.from_numpy(Fp[:, c0:c0 + 3].copy()))
        f0 = oracle.forward(**kw)
        out0[c0:c0 + 3] = f0.color
        dF[:, c0:c0 + 3] = oracle.backward(f0, dp[c0:c0 + 3])["colors_precomp"]
        kw["bg"] = bgp[c0:c0 + 3].copy()
        outbg[c0:c0 + 3] = oracle.forward(**kw).color
        radii = f0.radii
    ones = torch.zeros(N, 3); ones[:, 0] = 1.0
    alpha = oracle.forward(**common.scene_kwargs(g, cam, W, H, precolor=ones)).color[0]
    kwt = common.scene_kwargs(g, cam, W, H, as_torch=True)
    t = {k: v.to(DEV) for k, v in kwt.items() if torch.is_tensor(v) and k in ("means3D", "opacities", "shs", "scales", "rotations")}
    return dict(N=N, W=W, H=H, kw=kwt, t=t, F=F.to(DEV), bgf=bgf.to(DEV), dout=dout.to(DEV), colors=colors.to(DEV), out0=out0[:CMAX],
                outbg=outbg[:CMAX], dF=dF[:, :CMAX], alpha=alpha, radii=radii, instances=f0.num_rendered)


def blend(s, feats, bg_features=None, options=None, colors=None, bg=None):
    rs = settings(s["kw"], torch.zeros(3, device=DEV) if bg is None else bg)
    t = s["t"]
    return lg_features.blend_features(rs, feats, means3D=t["means3D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"],
                                      shs=None if colors is not None else t["shs"], colors_precomp=colors, bg_features=bg_features, options=options)


def options_of(name, mode):
    return dict(SCENES[name][4], **MODES[mode])


def test_the_listed_scene_has_long_lists():
    s = scene("n400_48x48_seg64")
    assert s["instances"] > 64 * 9                  # 9 tiles: lists of several 64-entry segments


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_forward_against_the_oracle(name, mode):
    s = scene(name)
    opts = options_of(name, mode)
    for C in CHANNELS:
        feats = s["F"][:, :C].contiguous()
        for bgf, ref in ((None, s["out0"]), (s["bgf"][:C].contiguous(), s["outbg"])):
            out, alpha, _color, radii = blend(s, feats, bgf, opts)
            out, alpha = out.cpu().numpy(), alpha.cpu().numpy()
            assert out.shape == (C, s["H"], s["W"]) and alpha.shape == (s["H"], s["W"])
            assert np.array_equal(radii.cpu().numpy(), s["radii"])
            if mode == "canonical":
                assert np.array_equal(bits(out), bits(ref[:C])), (name, C, np.abs(out - ref[:C]).max())
                assert np.array_equal(bits(alpha), bits(s["alpha"])), (name, C, np.abs(alpha - s["alpha"]).max())
            else:
                eo, _ = gpu_common.elem_excess(out, ref[:C], rtol=1e-4, atol_frac=2e-5)
                ea, _ = gpu_common.elem_excess(alpha, s["alpha"], rtol=1e-4, atol_frac=2e-5)
                print(f"{name} C={C} bg={'yes' if bgf is not None else 'no'}: excess out {eo:.3g} alpha {ea:.3g}")
                assert eo <= 1.0 and ea <= 1.0, (name, C, eo, ea)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_colours_as_features_reproduce_the_colour_image(name, mode):
    s = scene(name)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    out, _alpha, color, _radii = blend(s, s["colors"], bg, options_of(name, mode), colors=s["colors"], bg=bg)
    assert float(color.abs().max()) > 0.05
    assert torch.equal(out.view(torch.int32), color.view(torch.int32)), float((out - color).abs().max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_alpha_is_the_blended_ones_channel(name, mode):
    s = scene(name)
    for C in (1, 3, 17):
        feats = torch.cat([s["F"][:, :C - 1], torch.ones(s["N"], 1, device=DEV)], 1).contiguous()
        out, alpha, _c, _r = blend(s, feats, None, options_of(name, mode))
        assert float(alpha.max()) > 0.3
        assert torch.equal(out[C - 1].view(torch.int32), alpha.view(torch.int32)), (name, C)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_backward_against_the_oracle(name, mode):
    s = scene(name)
    opts = options_of(name, mode)
    hidden = torch.from_numpy(s["radii"] == 0).to(DEV)
    assert 0 < int((~hidden).sum())
    for C in CHANNELS:
        feats = s["F"][:, :C].clone().requires_grad_(True)
        out, alpha, color, radii = blend(s, feats, s["bgf"][:C].contiguous(), opts)
        assert out.requires_grad and not alpha.requires_grad and not color.requires_grad and not radii.requires_grad
        loss = (out * s["dout"][:C]).sum()
        (g1,) = torch.autograd.grad(loss, feats, retain_graph=True)
        (g2,) = torch.autograd.grad(loss, feats)
        assert g1.shape == (s["N"], C)
        assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), "two backward calls differ"
        assert not g1[hidden].any(), "rows of Gaussians with radii == 0 must be exact zeros"
        e, i = gpu_common.elem_excess(g1.cpu().numpy(), s["dF"][:, :C], rtol=1e-4, atol_frac=2e-5)
        print(f"{name} {mode} C={C}: dF excess {e:.3g}")
        assert e <= 1.0, (name, mode, C, e, i)


@pytest.mark.parametrize("mode", MODES)
def test_empty_model(mode):
    s = scene("n64_33x17")
    rs = settings(s["kw"], torch.zeros(3, device=DEV))
    e = lambda *shape: torch.zeros(*shape, device=DEV)  # noqa: E731
    for C in (1, 17):
        feats = e(0, C).requires_grad_(True)
        bgf = s["bgf"][:C].contiguous()
        out, alpha, color, radii = lg_features.blend_features(rs, feats, means3D=e(0, 3), opacities=e(0, 1), scales=e(0, 3), rotations=e(0, 4),
                                                              shs=e(0, 16, 3), bg_features=bgf, options=MODES[mode])
        assert radii.shape == (0,) and not alpha.any() and not color.any()
        assert torch.equal(out, bgf[:, None, None].expand(C, s["H"], s["W"]))
        (g,) = torch.autograd.grad((out * s["dout"][:C]).sum(), feats)
        assert g.shape == (0, C)


@pytest.mark.parametrize("mode", MODES)
def test_camera_that_sees_nothing(mode):
    s = scene("n300_70x45")
    away = syn.orbit_camera(1, 7, s["W"], s["H"], radius=4.0, target=(2 * 4.0 * math.sin(2 * math.pi / 7), 0.0, -2 * 4.0 * math.cos(2 * math.pi / 7)))
    g = syn.make_gaussians(s["N"], seed=3, extent=(1.5, 1.0, 1.5), **SCENES["n300_70x45"][3])
    kw = common.scene_kwargs(g, away, s["W"], s["H"], as_torch=True)
    rs = settings(kw, torch.zeros(3, device=DEV))
    t = s["t"]
    for C in (3, 17):
        feats = s["F"][:, :C].clone().requires_grad_(True)
        bgf = s["bgf"][:C].contiguous()
        out, alpha, _color, radii = lg_features.blend_features(rs, feats, means3D=t["means3D"], opacities=t["opacities"], scales=t["scales"],
                                                               rotations=t["rotations"], shs=t["shs"], bg_features=bgf, options=MODES[mode])
        assert not radii.any() and not alpha.any()
        assert torch.equal(out, bgf[:, None, None].expand(C, s["H"], s["W"]))
        (gr,) = torch.autograd.grad((out * s["dout"][:C]).sum(), feats)
        assert gr.shape == (s["N"], C) and not gr.any()


def test_geometry_inputs_are_constants_and_warn_once():
    s = scene("n64_33x17")
    t = dict(s["t"])
    t["means3D"] = t["means3D"].clone().requires_grad_(True)
    rs = settings(s["kw"], torch.zeros(3, device=DEV))
    feats = s["F"][:, :3].clone().requires_grad_(True)
    lg_features._warned[0] = False
    with pytest.warns(UserWarning, match="constants of this function"):
        out = lg_features.blend_features(rs, feats, means3D=t["means3D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"],
                                         shs=t["shs"])[0]
    out.sum().backward()
    assert feats.grad is not None and t["means3D"].grad is None


def test_render_features_depth_compressed_equals_dense():
    from test_gpu_vq_render import packed_scene
    cg = vectree.CompressedGaussians.from_packed(packed_scene(2113, 3, 0.6, scale=0.05), DEV)
    dense = cg.to_dense()
    pipe = syn.PipelineParams()
    cam = syn.orbit_camera(1, 8, 160, 120).to(DEV)
    opts = {"fast_exp": False, "fuse_getters": False}
    a = gaussian_renderer.render_features(cam, cg, pipe, "depth", options=opts)
    b = gaussian_renderer.render_features(cam, dense, pipe, "depth", options=opts)
    assert set(a) == set(b) == {"features", "alpha", "render", "radii", "visibility_filter", "depth"}
    assert a["features"].shape == (1, 120, 160) and a["depth"].shape == (1, 120, 160) and a["alpha"].shape == (120, 160)
    assert float(a["alpha"].max()) > 0.5 and int(a["visibility_filter"].sum()) > 100
    for k in ("features", "alpha", "depth", "render"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(a["radii"], b["radii"]) and torch.equal(a["visibility_filter"], b["visibility_filter"])
    # expected depth lies between the nearest and the farthest visible Gaussian wherever something was hit
    vm = cam.world_view_transform
    z = (cg.get_xyz @ vm[:3, 2:3] + vm[3, 2])[a["visibility_filter"]]
    hit = a["alpha"] > 0.5
    d = a["depth"][0][hit]
    assert float(d.min()) >= float(z.min()) * 0.999 and float(d.max()) <= float(z.max()) * 1.001
    # a tensor of features goes the same way, and a trainable compressed model is accepted
    f = torch.randn(cg.num, 5, device=DEV)
    c = gaussian_renderer.render_features(cam, cg.trainable(), pipe, f, bg_features=torch.ones(5, device=DEV), options=opts)
    d2 = gaussian_renderer.render_features(cam, dense, pipe, f, bg_features=torch.ones(5, device=DEV), options=opts)
    assert torch.equal(c["features"].view(torch.int32), d2["features"].view(torch.int32)) and "depth" not in c
