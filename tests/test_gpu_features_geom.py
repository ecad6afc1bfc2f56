"""-m gpu: the geometry gradient of feature / depth / alpha maps -- lg_backward_features through features.blend_features(geometry_grad=True)
and gaussian_renderer.render_features(geometry_grad=True) -- against the oracle's backward summed over channel triples (float64),
under the rule of tests/test_gpu_parity.py::test_backward_parity; references are computed once per (scene, channels, background, loss)
and shared by both arithmetic modes (tests/features_geom_common.py)."""
import math

import numpy as np
import pytest
import torch

import common
import features_geom_common as fg
import tolerance
from common import syn
from lightgaussian_amd import features as lg_features
from lightgaussian_amd import gaussian_renderer
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = {"canonical": {"fast_exp": False}, "hardware_exp": {"fast_exp": True}}
CHANNELS = (1, 3, 7, 16, 17, 64)
COLOR_BG = (0.1, 0.2, 0.3)
INPUTS = ("means2D", "means3D", "opacities", "scales", "rotations", "shs")


def settings(kw, bg):
    return GaussianRasterizationSettings(
        image_height=kw["H"], image_width=kw["W"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"], bg=bg, scale_modifier=1.0,
        viewmatrix=kw["viewmatrix"].to(DEV), projmatrix=kw["projmatrix"].to(DEV), sh_degree=kw["sh_degree"], campos=kw["campos"].to(DEV),
        prefiltered=False, debug=False, f_count=False)


def options_of(name, mode):
    seg = fg.SCENES[name].get("seg")
    return dict(MODES[mode], **({"segment_length": seg} if seg else {}))


class Case:
    """One scene on the device with fresh leaves, the loss inputs of (C, bg), and the differentiable maps of one forward."""

    def __init__(self, name, Cn, bg, mode, colors=None, cam=None):
        c, g, cam0 = fg.scene(name)
        self.N, self.W, self.H = c["N"], c["W"], c["H"]
        kw = common.scene_kwargs(g, cam or cam0, self.W, self.H, as_torch=True)
        self.t = {k: kw[k].detach().to(DEV).clone().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        self.t["means2D"] = torch.zeros(self.N, 3, device=DEV, requires_grad=True)
        F, bgf, dout, dalpha, dcolor = fg.loss_inputs(self.N, Cn, self.H, self.W, bg)
        dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)  # noqa: E731
        self.feats = (dev(F) if colors is None else colors.clone()).requires_grad_(True)
        self.bgf, self.dout, self.dalpha, self.dcolor = dev(bgf), dev(dout), dev(dalpha), dev(dcolor)
        self.rs = settings(kw, torch.tensor(COLOR_BG, device=DEV))
        self.opts = options_of(name, mode)
        self.colors = colors
        self.kw = kw

    def maps(self, geometry_grad=True):
        t = self.t
        return lg_features.blend_features(self.rs, self.feats, means3D=t["means3D"], opacities=t["opacities"], scales=t["scales"],
                                          rotations=t["rotations"], shs=None if self.colors is not None else t["shs"],
                                          colors_precomp=self.colors, bg_features=self.bgf, options=self.opts, geometry_grad=geometry_grad,
                                          means2D=t["means2D"] if geometry_grad else None)

    def loss(self, maps, kind):
        out, alpha, color, _radii = maps
        terms = []
        if "o" in kind:
            terms.append((out * self.dout).sum())
        if "a" in kind:
            terms.append((alpha * self.dalpha).sum())
        if "c" in kind:
            terms.append((color * self.dcolor).sum())
        return sum(terms)

    def grads(self, loss, retain=False):
        names = [n for n in INPUTS if not (n == "shs" and self.colors is not None)]
        gs = torch.autograd.grad(loss, [self.t[n] for n in names] + [self.feats], retain_graph=retain, allow_unused=True)
        return dict(zip(names + ["features"], gs))


def to_np(gr):
    return {k: v.detach().cpu().numpy() for k, v in gr.items() if v is not None}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# (scene, C, non-zero bg_features, maps in the loss): every C on the first scene with zero and non-zero backgrounds, every scene at C = 17
# with all three maps (colour over a non-black background), and out alone / alpha alone
PARITY = ([("N300_70x45", C, C % 2 == 1, "oac") for C in CHANNELS]
          + [(n, 17, True, "oac") for n in fg.SCENES if n != "N300_70x45"]
          + [("N300_70x45", 7, True, "o"), ("N64_33x17", 7, False, "o"), ("N300_70x45", 7, True, "a"), ("N200_40x40_opaque", 7, True, "a")])


def test_the_opaque_scene_terminates_pixels_before_their_list_ends():
    assert fg.early_pixels("N200_40x40_opaque") > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name, Cn, bg, kind", PARITY, ids=lambda v: str(v))
def test_geometry_gradients_against_the_summed_oracle_backward(name, Cn, bg, kind, mode):
    case = Case(name, Cn, bg, mode)
    maps = case.maps()
    out, alpha, color, radii = maps
    assert out.requires_grad and alpha.requires_grad and color.requires_grad and not radii.requires_grad
    loss = case.loss(maps, kind)
    g1 = case.grads(loss, retain=True)
    g2 = case.grads(loss)
    for n, v in g1.items():
        if n == "features" and "o" not in kind:
            assert v is None
            continue
        assert v is not None and bool(torch.isfinite(v).all()), n
        assert same_bits(v, g2[n]), f"{n}: two backward calls differ"
        assert not v[radii == 0].any(), f"{n}: rows of Gaussians with radii == 0 must be exact zeros"
    fg.assert_within(to_np(g1), fg.reference(name, Cn, bg, kind, COLOR_BG), f"{name} C={Cn} {kind} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Cn", (1, 17, 64))
def test_feature_gradient_is_the_default_modes_bit_for_bit(Cn, mode):
    case = Case("N300_70x45", Cn, True, mode)
    g_geom = case.grads(case.loss(case.maps(), "oac"))["features"]
    feats = case.feats.detach().clone().requires_grad_(True)
    t = {k: v.detach() for k, v in case.t.items()}
    out = lg_features.blend_features(case.rs, feats, means3D=t["means3D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"],
                                     shs=t["shs"], bg_features=case.bgf, options=case.opts)[0]
    (g_def,) = torch.autograd.grad((out * case.dout).sum(), feats)
    assert float(g_def.abs().max()) > 0 and same_bits(g_geom, g_def)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["N300_70x45", "N400_48x48_seg64"])
def test_colours_as_a_feature_triple_match_the_rasterizer_backward(name, mode):
    """features = the colours themselves, loss on `out` only: the geometry gradient through lg_features_bwd_geom against the project's
    own K7 + K9 backward of render(override_color=...) with the same dL/dimage -- 1e-4 relative and the element-wise bound, unwidened."""
    N = fg.SCENES[name]["N"]
    colors = torch.rand(N, 3, generator=torch.Generator().manual_seed(7)).to(DEV)
    case = Case(name, 3, True, mode, colors=colors)
    case.bgf = torch.tensor(COLOR_BG, device=DEV)
    new = to_np(case.grads(case.loss(case.maps(), "o")))
    ref = Case(name, 3, True, mode, colors=colors)
    t = ref.t
    cols = colors.clone().requires_grad_(True)
    image, _radii = GaussianRasterizer(raster_settings=ref.rs, options=ref.opts)(
        means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], colors_precomp=cols, scales=t["scales"], rotations=t["rotations"])
    gs = torch.autograd.grad((image * ref.dout).sum(), [t[n] for n in fg.GEOMETRY])
    for n, r in zip(fg.GEOMETRY, gs):
        r = r.cpu().numpy()
        err, ex = fg.rel_err(new[n], r), tolerance.elem_excess(new[n], r)[0]
        print(f"{name} {mode} {n}: rel_err {err:.3e} elem_excess {ex:.3f}")
        assert np.abs(r).max() > 0 and err <= fg.TOL and ex <= 1.0, (n, err, ex)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["N300_70x45", "N400_48x48_seg64"])
def test_a_zero_feature_gradient_leaves_the_colour_backward_bit_identical(name, mode):
    """Linearity where it is exact: dL_dout = 0 adds exact zeros to K7's rows."""
    case = Case(name, 17, True, mode)
    out, alpha, color, _r = case.maps()
    new = case.grads((out * 0.0).sum() + (color * case.dcolor).sum())
    ref = Case(name, 17, True, mode)
    t = ref.t
    image, _radii = GaussianRasterizer(raster_settings=ref.rs, options=ref.opts)(
        means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    assert same_bits(image, color)
    gs = torch.autograd.grad((image * ref.dcolor).sum(), [t[n] for n in INPUTS])
    for n, r in zip(INPUTS, gs):
        assert float(r.abs().max()) > 0 and same_bits(new[n], r), n
    assert not new["features"].any()


@pytest.mark.parametrize("mode", MODES)
def test_empty_model(mode):
    c, _g, cam = fg.scene("N64_33x17")
    kw = common.scene_kwargs(syn.make_gaussians(4), cam, c["W"], c["H"], as_torch=True)
    rs = settings(kw, torch.tensor(COLOR_BG, device=DEV))
    e = lambda *shape: torch.zeros(*shape, device=DEV, requires_grad=True)  # noqa: E731
    for Cn in (1, 17):
        ins = dict(means3D=e(0, 3), opacities=e(0, 1), scales=e(0, 3), rotations=e(0, 4), shs=e(0, 16, 3))
        feats, m2 = e(0, Cn), e(0, 3)
        out, alpha, color, radii = lg_features.blend_features(rs, feats, bg_features=torch.ones(Cn, device=DEV), options=MODES[mode],
                                                              geometry_grad=True, means2D=m2, **ins)
        assert radii.shape == (0,) and not alpha.any() and bool((out == 1).all())
        gs = torch.autograd.grad(out.sum() + alpha.sum() + color.sum(), list(ins.values()) + [feats, m2], allow_unused=True)
        for v, g in zip(list(ins.values()) + [feats, m2], gs):
            assert g is None or g.shape == v.shape
        assert gs[0].shape == (0, 3) and gs[1].shape == (0, 1) and gs[-2].shape == (0, Cn)


@pytest.mark.parametrize("mode", MODES)
def test_camera_that_sees_nothing(mode):
    name = "N300_70x45"
    c = fg.SCENES[name]
    away = syn.orbit_camera(1, 7, c["W"], c["H"], radius=4.0, target=(2 * 4.0 * math.sin(2 * math.pi / 7), 0.0, -2 * 4.0 * math.cos(2 * math.pi / 7)))
    for Cn in (3, 17):
        case = Case(name, Cn, True, mode, cam=away)
        maps = case.maps()
        assert not maps[3].any() and not maps[1].any()
        for n, v in case.grads(case.loss(maps, "oac")).items():
            want = case.feats.shape if n == "features" else case.t[n].shape
            assert v.shape == want and not v.any(), n


def test_render_features_depth_moves_the_raw_parameters():
    name = "N64_33x17"
    c, g, cam = fg.scene(name)
    W, H = c["W"], c["H"]
    gd, ga = (torch.from_numpy(a).float().to(DEV) for a in fg.depth_loss_maps(H, W))
    pipe = syn.PipelineParams()
    model = g.to(DEV)
    for n in fg.RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    pkg = gaussian_renderer.render_features(cam.to(DEV), model, pipe, "depth", geometry_grad=True, options={"fast_exp": False})
    assert set(pkg) == {"features", "alpha", "render", "radii", "visibility_filter", "depth", "viewspace_points"}
    assert pkg["depth"].requires_grad and pkg["alpha"].requires_grad and pkg["render"].requires_grad
    (pkg["depth"][0] * gd + pkg["alpha"] * ga).sum().backward()
    got = {}
    for n in fg.RAW:
        v = getattr(model, n).grad
        assert v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, n
        got[n] = v.cpu().numpy()
    assert pkg["viewspace_points"].grad is not None and float(pkg["viewspace_points"].grad.abs().max()) > 0
    fg.assert_within(got, fg.dense_depth_reference(name), "depth", names=fg.RAW)
    # the colour background reaches the by-product
    bgc = torch.tensor(COLOR_BG, device=DEV)
    with torch.no_grad():
        over = gaussian_renderer.render_features(cam.to(DEV), model, pipe, "depth", geometry_grad=True, bg_color=bgc, options={"fast_exp": False})
    assert same_bits(over["alpha"], pkg["alpha"].detach()) and not over["alpha"].requires_grad
    empty = over["alpha"] == 0
    assert bool(empty.any()) and bool((over["render"][:, empty] == bgc[:, None]).all())


def test_the_default_call_still_treats_the_geometry_as_a_constant():
    case = Case("N64_33x17", 3, False, "hardware_exp")
    lg_features._warned[0] = True
    out, alpha, color, _radii = case.maps(geometry_grad=False)
    assert out.requires_grad and not alpha.requires_grad and not color.requires_grad
    out.sum().backward()
    assert case.feats.grad is not None and case.t["means3D"].grad is None and case.t["opacities"].grad is None


CAMERA = "pitched_rolled"     # tests/camera_common.py: every entry of the view rotation is non-zero (every orbit camera has four zeros and a one)


@pytest.mark.parametrize("mode", MODES)
def test_geometry_gradients_under_a_pitched_and_rolled_camera(mode):
    """A feature + alpha loss under a camera whose view rotation has no zero entry: lg_backward_features' chain back to means3D, scales
    and rotations multiplies by entries that are exactly 0 or 1 in every other test of this file.  The reference is verified on the host
    by tests/test_features_geom_host.py."""
    name, Cn = "N300_70x45", 17
    cam = fg.scene(name, CAMERA)[2]
    assert float(cam.world_view_transform[:3, :3].abs().min()) >= 0.03
    case = Case(name, Cn, True, mode, cam=cam)
    maps = case.maps()
    radii = maps[3]
    assert int((radii > 0).sum()) >= 100
    g1 = case.grads(case.loss(maps, "oa"))
    for n in fg.GEOMETRY + ("features",):
        v = g1[n]
        assert v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, n
        assert not v[radii == 0].any(), f"{n}: rows of Gaussians with radii == 0 must be exact zeros"
    fg.assert_within(to_np(g1), fg.reference(name, Cn, True, "oa", COLOR_BG, camera=CAMERA), f"{name} {CAMERA} C={Cn} oa {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_render_features_depth_under_a_pitched_and_rolled_camera(mode):
    """The "depth" map and its gradient with respect to the raw parameters against the dense autograd twin.  vm[6] is not 0 here: the
    view-space depth, and with it the gradient of a depth loss, has a world-y component for the first time."""
    name = "N300_70x45"
    c, g, cam = fg.scene(name, CAMERA)
    W, H = c["W"], c["H"]
    assert abs(float(cam.world_view_transform[1, 2])) >= 0.03
    ref = fg.dense_depth_reference(name, CAMERA)
    gd, ga = (torch.from_numpy(a).float().to(DEV) for a in fg.depth_loss_maps(H, W))
    model = g.to(DEV)
    for n in fg.RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    pkg = gaussian_renderer.render_features(cam.to(DEV), model, syn.PipelineParams(), "depth", geometry_grad=True, options=MODES[mode])
    assert np.array_equal(pkg["radii"].cpu().numpy(), ref["maps"][2])
    fg.assert_depth_maps(pkg["features"][0].detach().cpu().numpy(), pkg["alpha"].detach().cpu().numpy(), ref["maps"], f"{name} {CAMERA} {mode}")
    assert same_bits(pkg["depth"].detach(), (pkg["features"] / pkg["alpha"].clamp_min(1e-6)).detach())
    (pkg["depth"][0] * gd + pkg["alpha"] * ga).sum().backward()
    got = {}
    for n in fg.RAW:
        v = getattr(model, n).grad
        assert v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, n
        got[n] = v.cpu().numpy()
    assert np.abs(got["_xyz"][:, 1]).max() > 0
    fg.assert_within(got, ref, f"depth {CAMERA} {mode}", names=fg.RAW)
