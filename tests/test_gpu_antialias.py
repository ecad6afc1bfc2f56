"""-m gpu: antialiased splatting (option "antialiasing", LG_FLAG_ANTIALIAS): K1 scales every opacity by rho = sqrt(max(0.000025,
det S / det(S + 0.3 I))) of its 2D covariance, K9 and lg_camera_bwd carry the gradient through rho.

References (tests/antialias_common.py): the CPU oracle called with opacities = sigma rho32 (rho32: the float32 value of the g++ build
of the product's lg_math.h) for everything that is bit-pinned, and the dense autograd twin with opacities = sigma rho, rho recomputed
differentiably, for the gradients -- by the rule of tests/camera_grad_common.py, per tensor in the max norm:
    rel_err(got, d64) <= max(1e-4, 3 rel_err(d32, d64)).
Scenes: "N300_70x45" (with six hand-placed Gaussians: rho at the floor, a rank-one covariance, behind the camera, the EWA clamp
active, one removed by the compensation alone, one ten times the mean size) and "N64_33x17".  Every reference is computed once.

The "opacity" weight policy keeps the RAW sigma (a property of the model, not of the view): its expected score is the oracle's
sequential sum of sigma over the oracle's antialiased hit count, not the score of the oracle call that was handed sigma rho32."""
import ctypes as C

import numpy as np
import pytest
import torch

import antialias_common as aa
import camera_grad_common as cg
import dense_twin
import features_geom_common as fg
import gpu_common
from common import bits as _bits
from common import syn
from common import to_numpy as _np
from lightgaussian_amd import _lib, gaussian_renderer, rasterizer, vectree
from oracle import oracle
from test_gpu_full_size import _last_contributor
from test_gpu_vq_render import packed_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENES = ("N300_70x45", "N64_33x17")
PER_GAUSSIAN = dense_twin.PER_GAUSSIAN
ON = {"antialiasing": True}


def run(kw, gimg, options, camera_grad=False):
    """gpu_common.run_rasterizer, the graph kept (the forward's saved state is read after the backward), as (image, radii, grads, camera)."""
    out = gpu_common.run_rasterizer(kw, gimg, options, camera_grad=camera_grad, retain_graph=True)
    return out["image"], out["radii"], out["grads"], out["camera"]


_ORACLE = {}


def oracle_antialiased(name):
    """(kw, rho32, {policy: float32 oracle forward of opacities = sigma rho32 with counts}); computed once per scene."""
    if name not in _ORACLE:
        kw = aa.combo_kwargs(name, "sh3")
        rho32 = aa.rho32_harness(kw)
        k = _np(kw)
        k["opacities"] = (k["opacities"].reshape(-1) * rho32).astype(np.float32)[:, None]
        _ORACLE[name] = (kw, rho32, {p: oracle.forward(count=True, weight_policy=w, **k) for p, w in
                                     (("opacity", oracle.W_OPACITY), ("alpha_t", oracle.W_ALPHA_T))})
    return _ORACLE[name]


def _opacity_score(sigma, count):
    """important_score of the "opacity" policy: count sequential float32 additions of the raw sigma."""
    return np.array([oracle.seqsum(s, c) for s, c in zip(sigma.reshape(-1), count)], np.float32)


# ---- 1. forward, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_forward_is_bit_identical_to_the_oracle_with_compensated_opacities(name):
    if name == "N300_70x45":
        aa.assert_scene_conditions()
    kw, rho32, ref = oracle_antialiased(name)
    sigma = aa.f32(kw["opacities"]).reshape(-1)
    H, W = kw["H"], kw["W"]
    canonical = dict(ON, fast_exp=False)
    color, radii, _g, _c = run(kw, cg.image_gradient(H, W), canonical)
    plain = run(kw, cg.image_gradient(H, W), {"fast_exp": False})
    assert np.array_equal(_bits(color), _bits(ref["opacity"].color))
    assert not np.array_equal(_bits(color), _bits(plain[0]))
    assert torch.equal(radii, plain[1]) and np.array_equal(radii.cpu().numpy(), ref["opacity"].radii)        # radii do not depend on the option
    ids, final_T = _last_contributor(color, W, H)
    assert np.array_equal(ids, oracle.last_contributor_ids(ref["opacity"]))
    assert np.array_equal(final_T.view(np.uint32), ref["opacity"].saved["final_T"].view(np.uint32))
    for pol in ("opacity", "alpha_t"):
        with rasterizer.options(antialiasing=True, weight_policy=pol):
            out = gpu_common.hip_forward_backward(kw, count=True)
        assert np.array_equal(out["count"], ref[pol].count), pol
        assert np.array_equal(_bits(out["color"]), _bits(ref[pol].color)) and np.array_equal(out["radii"], ref[pol].radii)
        want = _opacity_score(sigma, ref[pol].count) if pol == "opacity" else ref[pol].score
        assert np.array_equal(_bits(out["score"]), _bits(want)), pol
    with rasterizer.options(weight_policy="opacity"):
        off = gpu_common.hip_forward_backward(kw, count=True)
    print(f"{name}: {int(off['count'].sum())} hits without, {int(ref['opacity'].count.sum())} with the compensation")
    assert ref["opacity"].count.sum() < off["count"].sum()


# ---- 2. backward against the twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["sh3", "precolor", "precov"])
@pytest.mark.parametrize("name", SCENES)
def test_backward_against_the_dense_twin(name, combo):
    kw = aa.combo_kwargs(name, combo)
    gimg = cg.image_gradient(kw["H"], kw["W"])
    ref = aa.dense_reference((name, combo), kw, gimg)
    _color, radii, grads, _c = run(kw, gimg, dict(ON, fast_exp=False))
    names = tuple(n for n in PER_GAUSSIAN if n in grads)
    got = {n: grads[n].cpu().numpy() for n in names}
    aa.assert_rule(got, ref, names, f"{name} {combo}")
    for n in names:
        assert not got[n][radii.cpu().numpy() == 0].any(), n
    _color, _r, fast, _c = run(kw, gimg, ON)          # the hardware-exp blend kernels read the same records
    aa.assert_rule({n: fast[n].cpu().numpy() for n in names}, ref, names, f"{name} {combo} fast_exp")
    if combo == "sh3":
        # the opacity gradient is rho32 x the oracle's gradient with respect to the compensated opacity it was handed
        _kw, rho32, _ref = oracle_antialiased(name)
        k = _np(kw)
        k["opacities"] = (k["opacities"].reshape(-1) * rho32).astype(np.float32)[:, None]
        via = {}
        for dt in (np.float64, np.float32):
            g = oracle.backward(oracle.forward(dtype=dt, **k), gimg.numpy())
            via[np.dtype(dt).name] = {"opacities": np.asarray(g["opacities"], np.float64).reshape(-1) * rho32.astype(np.float64)}
        aa.assert_rule({"opacities": got["opacities"].reshape(-1)}, via, ("opacities",), f"{name} rho32 x oracle")


_RAW = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")


def _raw_reference(name, g, kw, gimg):
    out = {}
    for dd, dname in dense_twin.DTYPES:
        raw = {n: getattr(g, n).to(dd).detach().clone().requires_grad_() for n in _RAW}
        act = dict(means3D=raw["_xyz"], opacities=torch.sigmoid(raw["_opacity"]), scales=torch.exp(raw["_scaling"]),
                   rotations=torch.nn.functional.normalize(raw["_rotation"]), shs=torch.cat([raw["_features_dc"], raw["_features_rest"]], 1))
        (dense_twin.render(kw, dd, leaves=act, antialias=True)[0] * gimg.to(dd)).sum().backward()
        out[dname] = {n: raw[n].grad.numpy().astype(np.float64) for n in _RAW}
    return out


@pytest.mark.parametrize("name", SCENES)
def test_backward_of_the_raw_path_against_the_dense_twin(name):
    g, cam, W, H = aa.small_scene(name)
    kw = aa.combo_kwargs(name, "sh3")
    gimg = cg.image_gradient(H, W)
    ref = _raw_reference(name, g, kw, gimg)
    model = g.to(DEV)
    for n in _RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    bg = torch.tensor(cg.BG, device=DEV)
    pkg = gaussian_renderer.render(cam.to(DEV), model, syn.PipelineParams(), bg, options=ON)
    assert pkg["render"].grad_fn is not None and "Raw" in type(pkg["render"].grad_fn).__name__       # the fused getters
    (pkg["render"] * gimg.to(DEV)).sum().backward()
    aa.assert_rule({n: getattr(model, n).grad.cpu().numpy() for n in _RAW}, ref, _RAW, f"{name} raw")


# ---- 3. the significance-only pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_significance_only_pass(name):
    kw, _rho32, ref = oracle_antialiased(name)
    sigma = aa.f32(kw["opacities"]).reshape(-1)
    with rasterizer.options(antialiasing=True, skip_color_in_count=True, weight_policy="opacity"):
        out = gpu_common.hip_forward_backward(kw, count=True)
    assert np.array_equal(out["count"], ref["opacity"].count) and np.array_equal(out["radii"], ref["opacity"].radii)
    lib = _lib.load()
    cnt = torch.from_numpy(out["count"]).to(DEV)
    score = torch.empty(cnt.shape[0], dtype=torch.float32, device=DEV)
    _lib.check(lib.lg_score_from_count(cnt.shape[0], cnt.data_ptr(), torch.from_numpy(sigma).to(DEV).data_ptr(), score.data_ptr(),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(_bits(out["score"]), _bits(score)) and out["score"].max() > 0
    with rasterizer.options(antialiasing=True, skip_color_in_count=True, weight_policy="alpha_t"):
        per_hit = gpu_common.hip_forward_backward(kw, count=True)
    assert np.array_equal(per_hit["count"], ref["alpha_t"].count) and np.array_equal(_bits(per_hit["score"]), _bits(ref["alpha_t"].score))


# ---- 4. camera gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["sh3", "precov"])
def test_camera_gradients_against_the_dense_twin(combo):
    name = "N64_33x17"
    kw = aa.combo_kwargs(name, combo)
    gimg = cg.image_gradient(kw["H"], kw["W"])
    ref = aa.dense_reference((name, combo, "camera"), kw, gimg, camera=True)
    _color, _radii, grads, camera = run(kw, gimg, dict(ON, fast_exp=False), camera_grad=True)
    cg.assert_rule3(camera, ref, f"{name} {combo} antialiased")
    cg.assert_unused_columns_zero(camera, name)
    # ... and not the gradients of the uncompensated render
    plain = cg.dense_camera_reference((name, combo), kw, gimg)
    assert cg.rel_err(camera["viewmatrix"], plain["float64"]["viewmatrix"]) > 1e-2
    # the per-Gaussian gradients of the same backward are those of a backward without camera_grad, bit for bit
    _c, _r, alone, _n = run(kw, gimg, dict(ON, fast_exp=False))
    for n in grads:
        assert np.array_equal(_bits(grads[n]), _bits(alone[n])), n


# ---- 5. feature maps -----------------------------------------------------------------------------------------------------------------
def test_render_features_depth_with_geometry_gradients():
    name = "N64_33x17"
    c, g, cam = fg.scene(name)
    W, H = c["W"], c["H"]
    ref = fg.dense_depth_reference(name, antialias=True)
    gd, ga = (torch.from_numpy(a).float().to(DEV) for a in fg.depth_loss_maps(H, W))
    model = g.to(DEV)
    for n in fg.RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    pkg = gaussian_renderer.render_features(cam.to(DEV), model, syn.PipelineParams(), "depth", geometry_grad=True,
                                            options=dict(ON, fast_exp=False))
    assert np.array_equal(pkg["radii"].cpu().numpy(), ref["maps"][2])
    fg.assert_depth_maps(pkg["features"][0].detach().cpu().numpy(), pkg["alpha"].detach().cpu().numpy(), ref["maps"], f"{name} antialiased")
    (pkg["depth"][0] * gd + pkg["alpha"] * ga).sum().backward()
    got = {n: getattr(model, n).grad.cpu().numpy() for n in fg.RAW}
    fg.assert_within(got, ref, "depth antialiased", names=fg.RAW)
    with torch.no_grad():
        off = gaussian_renderer.render_features(cam.to(DEV), model, syn.PipelineParams(), "depth", options={"fast_exp": False})
    assert float((off["alpha"] - pkg["alpha"].detach()).abs().max()) > 1e-2          # the option is in the maps


# ---- 6. compressed models ------------------------------------------------------------------------------------------------------------
class _Pipe(syn.PipelineParams):
    antialiasing = True


def test_compressed_render_equals_the_dense_render_bit_for_bit():
    N = 3001
    cgm = vectree.CompressedGaussians.from_packed(packed_scene(N, 3, 0.6, scale=0.02), DEV)
    dense = cgm.to_dense()
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    cam = syn.orbit_camera(1, 8, 320, 240).to(DEV)
    unfused = {"fuse_getters": False}
    a = gaussian_renderer.render_compressed(cam, cgm, _Pipe(), bg, options=unfused)              # through pipe.antialiasing
    with torch.no_grad():
        b = gaussian_renderer.render(cam, dense, syn.PipelineParams(), bg, options=dict(unfused, antialiasing=True))
        plain = gaussian_renderer.render(cam, dense, syn.PipelineParams(), bg, options=unfused)
    assert int((b["radii"] > 0).sum()) > N // 20
    assert torch.equal(a["radii"], b["radii"]) and torch.equal(a["visibility_filter"], b["visibility_filter"])
    assert np.array_equal(_bits(a["render"]), _bits(b["render"]))
    assert torch.equal(plain["radii"], b["radii"]) and not np.array_equal(_bits(plain["render"]), _bits(b["render"]))
    assert set(a) == set(b) and not any(torch.is_tensor(v) and v.requires_grad for v in a.values())


# ---- 7. off is off, and runs repeat ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_exp", [True, False])
def test_off_equals_a_call_without_the_key_and_two_runs_give_the_same_bits(fast_exp):
    kw = aa.combo_kwargs("N300_70x45", "sh3")
    gimg = cg.image_gradient(kw["H"], kw["W"])
    absent, off = run(kw, gimg, {"fast_exp": fast_exp}), run(kw, gimg, {"fast_exp": fast_exp, "antialiasing": False})
    on, again = run(kw, gimg, dict(ON, fast_exp=fast_exp)), run(kw, gimg, dict(ON, fast_exp=fast_exp))
    for (x, y, same) in ((absent, off, True), (on, again, True), (on, off, False)):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) == same
        assert torch.equal(x[1], y[1])
        for n in x[2]:
            assert float(x[2][n].abs().max()) > 0
            assert np.array_equal(_bits(x[2][n]), _bits(y[2][n])) == same, n
