"""-m gpu: depth distortion and median depth (lg_blend_distortion / lg_backward_distortion, lightgaussian_amd.distortion.blend_geometry,
gaussian_renderer.render_geometry(distortion=True)).

Bit identity (canonical mode) with the g++ harness's full-view walk of the same lg_math.h text, run to run, across streams and on
poisoned memory; the value of D against the float64 dense twin; the median against a float64 per-pixel walk of the oracle's state; the
gradients against the dense autograd twin from the raw parameters; the argument refusals of the C ABI."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import common
import dense_twin
import distortion_common as dc
import features_geom_common as fg
import poison_common as pz
import tolerance
from common import syn
from lightgaussian_amd import _lib, distortion, features as lg_features, gaussian_renderer, normals
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = {"canonical": {"fast_exp": False}, "hardware_exp": {"fast_exp": True}}
SCENES = ("N64_33x17", "N400_48x48", "N400_48x48_seg64", "N200_40x40_opaque")
GEOMETRY = ("means2D", "means3D", "opacities", "scales", "rotations")
M_COLUMN, CHANNELS = 2, 5
SHIFT = 4.0                     # the camera radius of the scenes: the float32 twin's m is taken about it


def settings(kw):
    return GaussianRasterizationSettings(
        image_height=kw["H"], image_width=kw["W"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"], bg=torch.zeros(3, device=DEV), scale_modifier=1.0,
        viewmatrix=kw["viewmatrix"].to(DEV), projmatrix=kw["projmatrix"].to(DEV), sh_degree=kw["sh_degree"], campos=kw["campos"].to(DEV),
        prefiltered=False, debug=False, f_count=False)


def options_of(name, mode):
    seg = fg.SCENES[name].get("seg")
    return dict(MODES[mode], **({"segment_length": seg} if seg else {}))


def view_z(kw):
    """float32 view-space z of the scene's Gaussians, evaluated on the CPU: the m both the library and the harness are handed."""
    vm = kw["viewmatrix"].float()
    return (kw["means3D"].float() @ vm[:3, 2] + vm[3, 2]).contiguous()


@functools.lru_cache(maxsize=None)
def abi_case(name, W=None, H=None):
    """The scene's rasterizer kwargs (CPU torch), a feature tensor whose column M_COLUMN is view_z, and the two loss maps."""
    c, g, cam = fg.scene(name)
    W, H = W or c["W"], H or c["H"]
    if (W, H) != (c["W"], c["H"]):
        cam = syn.orbit_camera(1, 7, W, H, radius=4.0)
    kw = common.scene_kwargs(g, cam, W, H, as_torch=True)
    rs = np.random.RandomState(17)
    feats = torch.from_numpy(rs.randn(c["N"], CHANNELS).astype(np.float32))
    feats[:, M_COLUMN] = view_z(kw)
    gD, gM = (torch.from_numpy(rs.randn(H, W).astype(np.float32)) for _ in range(2))
    # colours are handed over precomputed: with SH inputs K9 adds the view-direction term of the colours to dL/dmeans3D, an exact zero
    # here that turns a -0.0 of the chain into +0.0, which the harness (it has no colours) would have to imitate
    kw["colors_precomp"] = torch.from_numpy(rs.rand(c["N"], 3).astype(np.float32))
    return dict(kw=kw, feats=feats, gD=gD, gM=gM, N=c["N"], W=W, H=H)


def run_abi(case, opts, gD=True, gM=True):
    """blend_geometry on fresh leaves + the backward of sum(D gD + median gM): every output of the two C calls."""
    kw = case["kw"]
    t = {k: kw[k].detach().to(DEV).clone().requires_grad_(True) for k in ("means3D", "opacities", "colors_precomp", "scales", "rotations")}
    t["means2D"] = torch.zeros(case["N"], 3, device=DEV, requires_grad=True)
    feats = case["feats"].to(DEV).clone().requires_grad_(True)
    out, alpha, color, radii, D, med = distortion.blend_geometry(
        settings(kw), feats, m_column=M_COLUMN, means3D=t["means3D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"],
        colors_precomp=t["colors_precomp"], options=opts, means2D=t["means2D"])
    loss = (D * case["gD"].to(DEV)).sum() * float(gD) + (med * case["gM"].to(DEV)).sum() * float(gM)
    gs = torch.autograd.grad(loss, [t[n] for n in GEOMETRY] + [feats])
    res = dict(zip(GEOMETRY + ("features",), gs))
    res.update(D=D.detach(), median=med.detach(), radii=radii, features_image=out.detach(), alpha=alpha.detach(), render=color.detach())
    return res


def same_bits(a, b):
    return np.array_equal(common.bits(a), common.bits(b))


# ---- the walk covers more than two batches ------------------------------------------------------------------------------------------
def test_a_tile_list_of_the_large_scene_is_longer_than_two_batches():
    case = abi_case("N400_48x48")
    call, _feats, _outputs, _geom, binning, _img, R = _forward(case)
    T = ((case["W"] + 15) // 16) * ((case["H"] + 15) // 16)
    ranges = torch.empty(T * 2, dtype=torch.int32, device=DEV)
    entries = torch.empty(max(R, 1), dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().lg_debug_tile_lists(C.byref(call.view), binning.data_ptr(), R, ranges.data_ptr(), entries.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    ranges = ranges.cpu().numpy().reshape(T, 2).astype(np.int64)
    longest = int((ranges[:, 1] - ranges[:, 0]).max())
    print(f"N400_48x48: longest tile list {longest} entries, {R} instances")
    assert longest > 128
    assert dc.view(common.to_numpy(case["kw"]), case["feats"][:, M_COLUMN].numpy())["longest"] == longest


# ---- bit identity -------------------------------------------------------------------------------------------------------------------
def _assert_harness_bits(got, want, what):
    assert np.array_equal(got["radii"].cpu().numpy(), want["radii"]), what
    for n in ("D", "median") + GEOMETRY:
        g, w = common.f32(got[n]), want[n]
        diff = int((common.bits(g).reshape(-1) != common.bits(w).reshape(-1)).sum())
        print(f"{what} {n}: {diff} of {w.size} words differ from the harness (max |.| {np.abs(w).max():.3e})")
        assert diff == 0, f"{what}: {n} differs from the harness in {diff} words"
    gf = common.f32(got["features"])
    assert same_bits(gf[:, M_COLUMN], want["dm"]), f"{what}: dL_dm differs from the harness"
    assert not np.delete(gf, M_COLUMN, axis=1).any(), f"{what}: a feature column other than m received a gradient"


@pytest.mark.parametrize("name", SCENES)
def test_bit_identical_to_the_harness_walk(name):
    case = abi_case(name)
    opts = options_of(name, "canonical")
    got = run_abi(case, opts)
    want = dc.view(common.to_numpy(case["kw"]), case["feats"][:, M_COLUMN].numpy(), case["gD"].numpy(), case["gM"].numpy())
    print(f"{name}: {want['instances']} instances, longest list {want['longest']}, {want['early']} pixels end early, {want['mid']} medians before the last contributor")
    assert float(np.abs(want["D"]).max()) > 0 and float(np.abs(want["dm"]).max()) > 0 and float(np.abs(want["means3D"]).max()) > 0
    if name == "N200_40x40_opaque":
        assert want["early"] > 0 and want["mid"] > 100
    _assert_harness_bits(got, want, name)
    again = run_abi(case, opts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run_abi(case, opts)
    side.synchronize()
    pz.assert_identical([("first", got), ("again", again), ("second stream", other)], f"{name} run to run")


@pytest.mark.parametrize("which", ["distortion_only", "median_only"])
def test_each_loss_alone_is_bit_identical_to_the_harness(which):
    case = abi_case("N200_40x40_opaque")
    use_d, use_m = which == "distortion_only", which == "median_only"
    got = run_abi(case, MODES["canonical"], gD=use_d, gM=use_m)
    zero = np.zeros((case["H"], case["W"]), np.float32)
    want = dc.view(common.to_numpy(case["kw"]), case["feats"][:, M_COLUMN].numpy(), case["gD"].numpy() if use_d else zero, case["gM"].numpy() if use_m else zero)
    _assert_harness_bits(got, want, which)
    if use_m:       # the median passes its gradient to m only: the geometry receives nothing
        assert not any(want[n].any() for n in GEOMETRY) and float(np.abs(want["dm"]).max()) > 0


def test_one_pixel_image():
    case = abi_case("N64_33x17", 1, 1)
    got = run_abi(case, MODES["canonical"])
    want = dc.view(common.to_numpy(case["kw"]), case["feats"][:, M_COLUMN].numpy(), case["gD"].numpy(), case["gM"].numpy())
    assert got["D"].shape == (1, 1) and want["instances"] > 0
    _assert_harness_bits(got, want, "1x1")


@pytest.mark.parametrize("mode", MODES)
def test_empty_model(mode):
    case = abi_case("N64_33x17")
    e = lambda *shape: torch.zeros(*shape, device=DEV, requires_grad=True)  # noqa: E731
    ins = dict(means3D=e(0, 3), opacities=e(0, 1), scales=e(0, 3), rotations=e(0, 4), shs=e(0, 16, 3))
    feats, m2 = e(0, CHANNELS), e(0, 3)
    with pz.poisoned(pz.SENTINEL):
        out, alpha, color, radii, D, med = distortion.blend_geometry(settings(case["kw"]), feats, m_column=M_COLUMN, options=MODES[mode], means2D=m2, **ins)
        torch.cuda.synchronize()
    assert radii.shape == (0,) and D.shape == (case["H"], case["W"]) and not D.any() and not med.any() and not alpha.any()
    gs = torch.autograd.grad(D.sum() + med.sum() + out.sum(), list(ins.values()) + [feats, m2], allow_unused=True)
    assert gs[0].shape == (0, 3) and gs[-2].shape == (0, CHANNELS)


# ---- poisoned memory ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["N64_33x17", "N400_48x48_seg64", "N200_40x40_opaque"])
def test_outputs_do_not_depend_on_what_memory_held(name):
    case = abi_case(name)
    opts = options_of(name, "canonical")
    runs = pz.run_all(lambda: run_abi(case, opts))
    pz.assert_identical(runs, f"blend_geometry {name}")
    assert float(runs[0][1]["D"].abs().max()) > 0


# ---- D against the float64 dense twin -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_distortion(name):
    """(D64, D32): A M2 - M1^2 from the dense twin rendering colors_precomp = [m, m m, 1], in float64, and in float32 with m taken about
    SHIFT (D does not depend on the shift; unshifted, float32 would cancel)."""
    name = name.replace("_seg64", "")
    case = abi_case(name)
    kw = dict(case["kw"], bg=torch.zeros(3))
    kw.pop("shs")
    kw.pop("colors_precomp")
    out = []
    for dd, shift in ((torch.float64, 0.0), (torch.float32, SHIFT)):
        m = view_z(case["kw"]).to(dd)[:, None] - shift
        with torch.no_grad():
            color, _radii, _cnt = dense_twin.render(dict(kw, colors_precomp=torch.cat([m, m * m, torch.ones_like(m)], 1)), dd, front_only=False)
        out.append((color[2] * color[1] - color[0] * color[0]).numpy().astype(np.float64))
    return tuple(out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_distortion_against_the_float64_twin(name, mode):
    case = abi_case(name)
    got = run_abi(case, options_of(name, mode))
    D64, D32 = twin_distortion(name)
    tolerance.assert_rule3(got["D"].cpu().numpy(), D64, D32, f"{name} {mode} D")
    assert float(got["D"].min()) >= -1e-6 * float(D64.max())


# ---- the median against a float64 walk of the oracle's state ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def median_walk(name):
    """(sel [H,W]: id of the Gaussian whose incoming T is the last above 0.5, -1 without a contributor; near [H,W]: some incoming T of
    the pixel's walk lies within 1e-5 of 0.5), from the float64 oracle's saved state, lists rebuilt as fg.early_pixels does."""
    name = name.replace("_seg64", "")
    c, g, cam = fg.scene(name)
    W, H = c["W"], c["H"]
    f = oracle.forward(dtype=np.float64, **common.scene_kwargs(g, cam, W, H))
    s = f.saved
    x, y = s["xy"][:, 0].astype(np.float64), s["xy"][:, 1].astype(np.float64)
    A, B, Cc, op = (s["conic_opacity"][:, k].astype(np.float64) for k in range(4))
    rad = f.radii.astype(np.float64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rx0 = np.clip(np.trunc((x - rad) / 16), 0, gx); rx1 = np.clip(np.trunc((x + rad + 15) / 16), 0, gx)
    ry0 = np.clip(np.trunc((y - rad) / 16), 0, gy); ry1 = np.clip(np.trunc((y + rad + 15) / 16), 0, gy)
    n_contrib = s["n_contrib"].reshape(H, W)
    sel, near = np.full((H, W), -1, np.int64), np.zeros((H, W), bool)
    for ty in range(gy):
        for tx in range(gx):
            ids = np.nonzero((f.radii > 0) & (rx0 <= tx) & (tx < rx1) & (ry0 <= ty) & (ty < ry1))[0]
            order = ids[np.argsort(s["depth"][ids], kind="stable")]
            for py in range(ty * 16, min(H, ty * 16 + 16)):
                for px in range(tx * 16, min(W, tx * 16 + 16)):
                    T = 1.0
                    for j in order[:n_contrib[py, px]]:
                        dx, dy = x[j] - px, y[j] - py
                        power = -0.5 * (A[j] * dx * dx + Cc[j] * dy * dy) - B[j] * dx * dy
                        alpha = min(0.99, op[j] * np.exp(min(power, 0.0)))
                        if power > 0 or alpha < 1.0 / 255.0:
                            continue
                        near[py, px] |= abs(T - 0.5) < 1e-5
                        if T > 0.5:
                            sel[py, px] = j
                        T *= 1.0 - alpha
    return sel, near


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_median_against_the_float64_walk(name, mode):
    case = abi_case(name)
    got = run_abi(case, options_of(name, mode))["median"].cpu().numpy()
    sel, near = median_walk(name)
    has = sel >= 0
    left_out = int((near & has).sum())
    print(f"{name} {mode}: {int(has.sum())} pixels have a median, {left_out} left out (an incoming T within 1e-5 of 0.5)")
    assert has.sum() > 100 and left_out <= 0.01 * has.sum()
    z = view_z(case["kw"]).numpy()
    want = np.where(has, z[np.maximum(sel, 0)], np.float32(0.0))
    keep = ~near
    wrong = int((got[keep] != want[keep]).sum())
    print(f"{name} {mode}: {wrong} of {int(keep.sum())} medians differ from the walk's")
    assert wrong == 0                   # the median is a copy of the selected Gaussian's m


# ---- gradients through render_geometry(distortion=True) against the dense twin from the raw parameters ----------------------------------
def twin_rows(raw, vm):
    """normals.gaussian_normals' contract in raw's dtype: (view-space normal facing the camera, view-space z)."""
    q = torch.nn.functional.normalize(raw["_rotation"], dim=1, eps=1e-12)
    k = torch.argmin(raw["_scaling"], dim=1)
    n_w = normals._rotation_of_unit(q)[torch.arange(q.shape[0]), :, k]
    n_v = n_w @ vm[:3, :3]
    p_v = raw["_xyz"] @ vm[:3, :3] + vm[3, :3]
    sign = torch.where((n_v * p_v).sum(1) > 0, -1.0, 1.0).to(n_v.dtype).detach()
    return n_v * sign[:, None], p_v[:, 2:3]


def loss_maps(name):
    c = fg.SCENES[name.replace("_seg64", "")]
    rs = np.random.RandomState(29)
    m = {k: rs.randn(c["H"], c["W"]) for k in ("gD", "gM", "gd", "ga")}
    m["gn"] = rs.randn(3, c["H"], c["W"])
    m["gM"] = np.where(median_walk(name)[1], 0.0, m["gM"])        # a pixel whose selection is a near tie takes no part
    return m


@functools.lru_cache(maxsize=None)
def twin_gradients(name):
    """{dtype name: {raw parameter: gradient}} of sum(D gD + median gM + depth gd + alpha ga + normal . gn) by the dense twin from the RAW
    parameters (as fg.dense_depth_reference): three renders -- the normals, [z, 1, 0] and [z - SHIFT, (z - SHIFT)^2, 1] -- in float64 and
    in float32; the median term is z of the Gaussian the float64 walk selected."""
    name = name.replace("_seg64", "")
    c, g, cam = fg.scene(name)
    kw = common.scene_kwargs(g, cam, c["W"], c["H"], precolor=torch.zeros(c["N"], 3), as_torch=True)
    lm = loss_maps(name)
    sel, _near = median_walk(name)
    has = torch.from_numpy(sel >= 0)
    idx = torch.from_numpy(np.maximum(sel, 0))
    out = {}
    for dd, dname in dense_twin.DTYPES:
        raw = {n: getattr(g, n).to(dd).detach().clone().requires_grad_() for n in fg.RAW}
        vm = cam.world_view_transform.to(dd)
        nrm, z = twin_rows(raw, vm)
        act = dict(means3D=raw["_xyz"], opacities=torch.sigmoid(raw["_opacity"]), scales=torch.exp(raw["_scaling"]),
                   rotations=torch.nn.functional.normalize(raw["_rotation"]))
        one, zs = torch.ones_like(z), z - SHIFT
        render = lambda cols: dense_twin.render(kw, dd, leaves=dict(act, colors_precomp=cols), front_only=False)[0]  # noqa: E731
        n_img, d_img, m_img = render(nrm), render(torch.cat([z, one, torch.zeros_like(z)], 1)), render(torch.cat([zs, zs * zs, one], 1))
        t = {k: torch.from_numpy(v).to(dd) for k, v in lm.items()}
        D = m_img[2] * m_img[1] - m_img[0] * m_img[0]
        depth = d_img[0] / d_img[1].clamp_min(1e-6)
        median = torch.where(has, z[:, 0][idx], torch.zeros((), dtype=dd))
        ((D * t["gD"]).sum() + (median * t["gM"]).sum() + (depth * t["gd"]).sum() + (d_img[1] * t["ga"]).sum() + (n_img * t["gn"]).sum()).backward()
        out[dname] = {n: raw[n].grad.numpy().astype(np.float64) for n in fg.RAW}
    return out


def leaf_model(name):
    _c, g, cam = fg.scene(name)
    pc = syn.SyntheticGaussians(*[t.detach().clone().to(DEV).requires_grad_(True) for t in
                                  (g._xyz, g._features_dc, g._features_rest, g._scaling, g._rotation, g._opacity)], g.active_sh_degree, g.max_sh_degree)
    return pc, cam.to(DEV)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_gradients_through_render_geometry_against_the_dense_twin(name, mode):
    pc, cam = leaf_model(name)
    pkg = gaussian_renderer.render_geometry(cam, pc, syn.PipelineParams(), options=options_of(name, mode), distortion=True)
    assert pkg["distortion"].requires_grad and pkg["median_depth"].requires_grad
    t = {k: torch.from_numpy(v).float().to(DEV) for k, v in loss_maps(name).items()}
    loss = ((pkg["distortion"] * t["gD"]).sum() + (pkg["median_depth"] * t["gM"]).sum() + (pkg["depth"] * t["gd"]).sum()
            + (pkg["alpha"] * t["ga"]).sum() + (pkg["normal"] * t["gn"]).sum())
    params = [getattr(pc, n) for n in fg.RAW]
    g1 = torch.autograd.grad(loss, params, retain_graph=True)
    g2 = torch.autograd.grad(loss, params)
    ref = twin_gradients(name)
    for n, a, b in zip(fg.RAW, g1, g2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{n}: two backward calls differ"
        tolerance.assert_rule3(a.cpu().numpy(), ref["float64"][n], ref["float32"][n], f"{name} {mode} {n}")


@pytest.mark.parametrize("name", ["N64_33x17", "N400_48x48_seg64"])
def test_render_geometry_without_distortion_is_unchanged(name):
    """distortion=False takes the blend_features path as before; distortion=True returns the same shared maps, and a loss that leaves
    the two new maps out has the same gradient bits (the distortion walk adds exact zeros to the moment rows)."""
    t = {k: torch.from_numpy(v).float().to(DEV) for k, v in loss_maps(name).items()}
    res = []
    for flag in (False, True):
        pc, cam = leaf_model(name)
        pkg = gaussian_renderer.render_geometry(cam, pc, syn.PipelineParams(), options=options_of(name, "canonical"), distortion=flag)
        assert ("distortion" in pkg) == flag and ("median_depth" in pkg) == flag
        ((pkg["depth"] * t["gd"]).sum() + (pkg["alpha"] * t["ga"]).sum() + (pkg["normal"] * t["gn"]).sum() + pkg["render"].sum()).backward()
        res.append(dict(maps={k: pkg[k].detach() for k in ("render", "alpha", "normal", "depth", "radii")}, grads={n: getattr(pc, n).grad for n in fg.RAW},
                        viewspace=pkg["viewspace_points"].grad))
    pz.assert_identical([("distortion=False", res[0]), ("distortion=True", res[1])], name)
    with torch.no_grad():
        pc, cam = leaf_model(name)
        pkg = gaussian_renderer.render_geometry(cam, pc, syn.PipelineParams(), options=options_of(name, "canonical"), geometry_grad=False, distortion=True)
    assert not pkg["distortion"].requires_grad and float(pkg["distortion"].abs().max()) > 0


def test_segment_length_other_than_the_forwards_gives_zero_gradients():
    """The backward of a view handed another segment length: K9 refuses the moment rows, and dL_dm must come out as zeros too."""
    case = abi_case("N400_48x48")
    for other in (64, 1024):          # the forward ran under the default, 512: a layout with more and with fewer checkpoint records
        got = _direct(case, segment_length_bwd=other)
        assert not got["dm"].any() and not got["means3D"].any() and not got["opacity"].any(), other
    ok = _direct(case, segment_length_bwd=None)
    assert float(ok["dm"].abs().max()) > 0 and float(ok["means3D"].abs().max()) > 0


# ---- the C ABI directly: refusals -----------------------------------------------------------------------------------------------------
def _forward(case, opts=None):
    kw = case["kw"]
    t = {k: kw[k].to(DEV) for k in ("means3D", "opacities", "colors_precomp", "scales", "rotations")}
    feats = case["feats"].to(DEV)
    _opts, call, _bg, outputs, (geom, binning, img), R = lg_features._forward_then_blend(
        feats, None, t["means3D"], t["opacities"], t["scales"], t["rotations"], None, None, t["colors_precomp"], settings(kw), opts or MODES["canonical"],
        differentiated=True)
    return call, feats, outputs, geom, binning, img, R


def _direct(case, segment_length_bwd=None):
    """lg_blend_distortion + lg_backward_distortion by hand (C = 0: no feature loss), optionally with another segment length in the
    backward's view."""
    lib = distortion.load()
    call, feats, outputs, geom, binning, img, R = _forward(case)
    N, H, W = case["N"], case["H"], case["W"]
    D, med = torch.empty(H, W, device=DEV), torch.empty(H, W, device=DEV)
    state = _lib.scratch(lib.lg_distortion_state_bytes(W, H), DEV)
    m = C.c_void_p(feats.data_ptr() + 4 * M_COLUMN)
    _lib.check(lib.lg_blend_distortion(C.byref(call.view), N, _lib.ptr(geom), _lib.ptr(binning), C.c_int64(R), m, CHANNELS, _lib.ptr(D), _lib.ptr(med),
                                       _lib.ptr(state), _lib.stream()))
    if segment_length_bwd is not None:
        call.view.segment_length = segment_length_bwd
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    g = dict(means2D=nan(N, 3), means3D=nan(N, 3), colors=nan(N, 3), opacity=nan(N, 1), scales=nan(N, 3), rotations=nan(N, 4), dm=nan(N))
    scratch = _lib.scratch(lib.lg_backward_distortion_scratch_bytes(N, R, 0), DEV)
    scratch.fill_(0xFF)
    gD, gM = case["gD"].to(DEV), case["gM"].to(DEV)
    _lib.check(lib.lg_backward_distortion(
        C.byref(call.view), C.byref(call.g), _lib.ptr(outputs[3]), _lib.ptr(geom), _lib.ptr(binning), _lib.ptr(img), C.c_int64(R), None, None, 0, None,
        None, None, _lib.ptr(g["means2D"]), _lib.ptr(g["means3D"]), None, _lib.ptr(g["colors"]), _lib.ptr(g["opacity"]), _lib.ptr(g["scales"]),
        _lib.ptr(g["rotations"]), None, None, None, m, CHANNELS, _lib.ptr(state), _lib.ptr(gD), _lib.ptr(gM), _lib.ptr(g["dm"]), _lib.ptr(scratch),
        _lib.stream()))
    torch.cuda.synchronize()
    return g


def test_argument_refusals():
    lib = distortion.load()
    case = abi_case("N64_33x17")
    call, feats, outputs, geom, binning, img, R = _forward(case)
    N, H, W = case["N"], case["H"], case["W"]
    D, med = torch.empty(H, W, device=DEV), torch.empty(H, W, device=DEV)
    state = _lib.scratch(lib.lg_distortion_state_bytes(W, H), DEV)
    m = C.c_void_p(feats.data_ptr() + 4 * M_COLUMN)
    view, P, st = C.byref(call.view), _lib.ptr, _lib.stream()

    def fwd(m=m, stride=CHANNELS, D=D, state=state):
        return lib.lg_blend_distortion(view, N, P(geom), P(binning), C.c_int64(R), m, stride, P(D) if D is not None else None, P(med),
                                       P(state) if state is not None else None, st)

    for kwargs, word in ((dict(m=None), "missing m"), (dict(stride=0), "m_stride"), (dict(state=None), "state"), (dict(D=None), "distortion map")):
        with pytest.raises(Exception, match=word):
            _lib.check(fwd(**kwargs))
    _lib.check(fwd())
    _lib.check(lib.lg_blend_distortion(view, N, P(geom), P(binning), C.c_int64(R), m, CHANNELS, P(D), None, P(state), st))       # median is optional
    g = dict(means2D=torch.empty(N, 3, device=DEV), means3D=torch.empty(N, 3, device=DEV), colors=torch.empty(N, 3, device=DEV),
             opacity=torch.empty(N, 1, device=DEV), scales=torch.empty(N, 3, device=DEV), rotations=torch.empty(N, 4, device=DEV))
    dm = torch.empty(N, device=DEV)
    scratch = _lib.scratch(lib.lg_backward_distortion_scratch_bytes(N, R, CHANNELS), DEV)
    gD = case["gD"].to(DEV)

    def bwd(Cn=0, m=m, stride=CHANNELS, state=state, dm=dm, scratch=scratch):
        return lib.lg_backward_distortion(
            view, C.byref(call.g), P(outputs[3]), P(geom), P(binning), P(img), C.c_int64(R), None, None, Cn, None, None, None, P(g["means2D"]),
            P(g["means3D"]), None, P(g["colors"]), P(g["opacity"]), P(g["scales"]), P(g["rotations"]), None, None, None, m, stride,
            P(state) if state is not None else None, P(gD), None, P(dm) if dm is not None else None, P(scratch) if scratch is not None else None, st)

    for kwargs, word in ((dict(Cn=65), "C must be"), (dict(Cn=-1), "C must be"), (dict(m=None), "missing m"), (dict(stride=0), "m_stride"),
                         (dict(state=None), "state"), (dict(dm=None), "dL_dm"), (dict(scratch=None), "scratch")):
        with pytest.raises(Exception, match=word):
            _lib.check(bwd(**kwargs))
    _lib.check(bwd())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dm).all()) and float(dm.abs().max()) > 0
