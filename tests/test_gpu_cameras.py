"""-m gpu: the HIP path against the CPU oracle under general cameras (tests/camera_common.py): pitched, rolled, and inside the scene.

Every other GPU test renders from synthetic.orbit_camera, whose view rotation is a rotation about world y (vm[1], vm[4], vm[6], vm[9]
exactly 0, vm[5] exactly 1) and which keeps every splat at depths of 1 .. 9.  Here every entry of the rotation is at least 0.03 in
magnitude, and the two inside cameras put Gaussians between the camera plane and the 0.2 near plane, behind the camera, and on both
clamps of t.x / t.z and t.y / t.z; radii reach 320 px next to 3 px ones and the sort key's depth field starts at 0.207.

All tests use CAMERA_SCENE (2000 Gaussians, 161 x 83, degree 3).  References are computed once per (camera, input variant) and shared.

FLOAT32_FLOORS
The float32 oracle's own error against the float64 oracle on these inputs, measured on the CPU (gradient image RandomState(11)):
tensor-level relative error / worst element in units of the element bound 1e-4 |b| + 2e-5 max|b|.  These are the floors the rule of
test_backward_parity (gpu_common.assert_backward_parity) widens by 3x; they are recomputed by the test, the table is for the reader.

  camera            means2D           means3D           opacities         shs               scales            rotations
  pitched_rolled    7.62e-05 / 2.85   5.29e-05 / 2.04   1.85e-05 / 0.77   4.39e-06 / 0.19   7.32e-05 / 3.55   9.65e-06 / 0.48
  steep_offcentre   9.21e-06 / 0.25   6.95e-06 / 0.32   2.77e-06 / 0.07   2.67e-06 / 0.10   5.60e-05 / 2.17   2.14e-04 / 3.89
  inside            1.09e-05 / 0.30   5.98e-06 / 0.20   2.17e-06 / 0.03   5.97e-07 / 0.02   1.50e-05 / 0.66   4.31e-05 / 1.02
  inside_wide       2.68e-06 / 0.08   6.90e-05 / 2.35   1.57e-06 / 0.07   1.96e-06 / 0.06   7.76e-05 / 0.65   8.49e-05 / 1.15

The element excess reaches 3.9 (and exceeds 1 under every camera), so none of them belongs to test_gpu_parity.WELL_CONDITIONED.
"""

import numpy as np
import pytest
import torch

import camera_common as cc
import common
from common import bits as _bits
from common import syn
from common import to_numpy as _np
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
GIMG_SEED = 11


def _kw(name, variant="sh"):
    return cc.scene_kwargs(name, precolor=variant == "precolor", precov=variant == "precov", as_torch=True)


def _gimg():
    return np.random.RandomState(GIMG_SEED).randn(3, cc.H, cc.W).astype(np.float32)


_REF = {}


def count_reference(name, variant="sh"):
    """The float32 oracle's count forward of (camera, variant): computed once, never modified."""
    key = ("count", name, variant)
    if key not in _REF:
        _REF[key] = oracle.forward(count=True, **_np(_kw(name, variant)))
    return _REF[key]


def backward_reference(name):
    """(float32 image, float32 gradients, float64 gradients) of the oracle for sum(image * _gimg()): computed once per camera."""
    key = ("bwd", name)
    if key not in _REF:
        kw = _np(_kw(name))
        f32 = oracle.forward(**kw); g32 = oracle.backward(f32, _gimg())
        f64 = oracle.forward(dtype=np.float64, **kw); g64 = oracle.backward(f64, _gimg())
        _REF[key] = (f32.color, g32, g64)
    return _REF[key]


def test_the_cameras_exercise_what_they_are_here_for():
    """camera_common.check_preconditions() asserts the conditions; print what this scene gives."""
    for name, fa in cc.check_preconditions().items():
        print(name, fa)
        assert fa["min_rot"] >= 0.03 and fa["visible"] >= 200
    assert min(cc.check_preconditions()[n]["min_depth"] for n in cc.INSIDE) < 0.25      # the key's depth field starts at the near plane


# ---- a. forward / count parity -----------------------------------------------------------------------------------------------------------
FORWARD = [(n, "sh") for n in cc.NAMES] + [("inside", "precov"), ("inside", "precolor")]


@pytest.mark.parametrize("name, variant", FORWARD, ids=lambda v: str(v))
def test_forward_count_parity(name, variant):
    import gpu_common
    kw = _kw(name, variant)
    ref = count_reference(name, variant)
    out = gpu_common.hip_forward_backward(kw, count=True)
    print(f"{name} {variant}: radii differ in {np.count_nonzero(out['radii'] != ref.radii)}, counts in {np.count_nonzero(out['count'] != ref.count)}, "
          f"scores in {np.count_nonzero(_bits(out['score']) != _bits(ref.score))} Gaussians; image differs in "
          f"{np.count_nonzero(_bits(out['color']) != _bits(ref.color))} values (max {np.abs(out['color'] - ref.color).max():.3e}); "
          f"{ref.num_rendered} instances, {int(ref.count.sum())} hits")
    assert np.array_equal(out["radii"], ref.radii)
    assert np.array_equal(out["count"], ref.count), f"hit counts differ in {np.count_nonzero(out['count'] != ref.count)} Gaussians"
    assert np.array_equal(_bits(out["score"]), _bits(ref.score)), "significance score not bit-identical"
    assert np.array_equal(_bits(out["color"]), _bits(ref.color)), "count-render image not bit-identical"
    fast = gpu_common.hip_forward_backward(kw, count=False)
    err = float(np.abs(fast["color"] - ref.color).max())
    print(f"{name} {variant}: training render max abs error {err:.3e}")
    assert np.array_equal(fast["radii"], ref.radii) and err <= 1e-5
    assert int(ref.count.sum()) > 10000


# ---- b. backward parity ------------------------------------------------------------------------------------------------------------------
def _backward_parity(name, what):
    import gpu_common
    color32, g32, g64 = backward_reference(name)
    out = gpu_common.hip_forward_backward(_kw(name), grad_image=_gimg())
    err = gpu_common.rel_err(out["color"], color32)
    print(f"{what}: image rel err {err:.3e}")
    assert err <= TOL
    assert set(out["grads"]) == {"means2D", "means3D", "opacities", "shs", "scales", "rotations"}
    for n, g in out["grads"].items():
        assert np.isfinite(g).all(), n
    gpu_common.assert_backward_parity(out["grads"], g32, g64, what=what)          # (not well-conditioned: see FLOAT32_FLOORS)


@pytest.mark.parametrize("name", cc.NAMES)
def test_backward_parity(name):
    """Gradients against the float64 oracle under the rule of tests/test_gpu_parity.py::test_backward_parity: rel_err <= max(1e-4, 3 floor),
    elem_excess <= max(1, 3 ex32), the 0.5 / 0.99 / 0.999 quantiles of the element error <= max(0.1, 3 x the float32 oracle's)."""
    _backward_parity(name, name)


def test_backward_parity_canonical_arithmetic_inside():
    """The same with fast_exp off (canonical exp / IEEE division in the backward) where the depths are smallest."""
    from lightgaussian_amd import rasterizer
    with rasterizer.options(fast_exp=False):
        _backward_parity("inside", "inside canonical")


# ---- c. K1 variants and the key layout at small depths -----------------------------------------------------------------------------------
RAW = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


@pytest.mark.parametrize("name", ["inside", "pitched_rolled"])
def test_k1_variants_agree(name):
    """render() (fused getters), render_fused and _render_unfused: bit-identical images and radii, raw-parameter gradients within 1e-4;
    the LDS-staged SH reader (k1_lds) gives a bit-identical image in both."""
    import gpu_common
    from lightgaussian_amd import rasterizer
    from lightgaussian_amd.gaussian_renderer import render, render_fused, _render_unfused
    assert rasterizer._OPTIONS["fuse_getters"] is True
    cc.check_preconditions()
    cam = cc.camera(name).to(DEV)
    bg = torch.tensor(cc.BG, device=DEV); pipe = syn.PipelineParams()
    gimg = torch.from_numpy(_gimg()).to(DEV)
    outs = {}
    for fn in (_render_unfused, render_fused, render):
        g = cc.gaussians().to(DEV).requires_grad_(True)
        pkg = fn(cam, g, pipe, bg)
        (pkg["render"] * gimg).sum().backward()
        with rasterizer.options(k1_lds=True), torch.no_grad():
            lds = fn(cam, g, pipe, bg)["render"]
        assert torch.equal(lds, pkg["render"].detach()), f"{fn.__name__}: k1_lds changes the image"
        outs[fn.__name__] = (pkg["render"].detach().cpu().numpy(), pkg["radii"].cpu().numpy(), pkg["viewspace_points"].grad.cpu().numpy(),
                             {n: getattr(g, n).grad.cpu().numpy() for n in RAW})
    ia, ra, va, ga = outs["_render_unfused"]
    assert np.abs(ia).max() > 0 and (ra > 0).sum() >= 200
    for other in ("render_fused", "render"):
        ib, rb, vb, gb = outs[other]
        print(f"{name} {other}: image differs from _render_unfused in {np.count_nonzero(_bits(ia) != _bits(ib))} values, radii in {np.count_nonzero(ra != rb)}")
        assert np.array_equal(ra, rb), other
        assert np.array_equal(_bits(ia), _bits(ib)), other
        print(f"{name} {other}: viewspace gradient rel err {gpu_common.rel_err(vb, va):.3e}")
        assert gpu_common.rel_err(vb, va) <= TOL
        for n in RAW:
            err = gpu_common.rel_err(gb[n], ga[n])
            print(f"{name} {other} {n}: rel err against _render_unfused {err:.3e}")
            assert np.abs(ga[n]).max() > 0 and err <= TOL, (other, n, err)
    # the oracle on the activations torch evaluates on the CPU sees the same radii
    assert np.array_equal(ra, count_reference(name).radii)


@pytest.mark.parametrize("name", ["inside", "pitched_rolled"])
def test_key_layouts_give_the_same_order_at_small_depths(name):
    """The assertions of test_gpu_parity.py::test_keys_beyond_64_bits_give_the_same_order on depths that start at the 0.2 near plane
    (LG_DEPTH_BIAS, the narrow key's dropped depth bits, the max_depth guard of the bounded forward): narrow_key, the bounded forward on
    the second view of the shape, and both together give count, score, image, radii and gradients bit-identical to the full key on the
    exact path; sort_all_bits gives the same count, score and image."""
    import gpu_common
    from lightgaussian_amd import rasterizer
    gimg = _gimg()
    ref = count_reference(name)
    modes = {"full": dict(narrow_key=False, sync_free=False), "narrow": dict(narrow_key=True, sync_free=False),
             "bounded": dict(narrow_key=False, sync_free="validated"), "narrow_bounded": dict(narrow_key=True, sync_free="validated")}
    res = {}
    for mode, opt in modes.items():
        with rasterizer.options(**opt):
            res[mode] = (gpu_common.hip_forward_backward(_kw(name), count=True),
                         gpu_common.hip_forward_backward(_kw(name), grad_image=gimg),
                         gpu_common.hip_forward_backward(_kw(name), count=True))      # (second view of the shape: bounded when enabled)
    a = res["full"]
    assert np.array_equal(a[0]["count"], ref.count) and np.array_equal(_bits(a[0]["score"]), _bits(ref.score))
    assert np.array_equal(_bits(a[0]["color"]), _bits(ref.color)) and np.array_equal(a[0]["radii"], ref.radii)
    for mode in ("narrow", "bounded", "narrow_bounded"):
        b = res[mode]
        for k in (0, 2):
            assert np.array_equal(a[0]["count"], b[k]["count"]) and np.array_equal(_bits(a[0]["color"]), _bits(b[k]["color"])), (mode, k)
            assert np.array_equal(_bits(a[0]["score"]), _bits(b[k]["score"])) and np.array_equal(a[0]["radii"], b[k]["radii"]), (mode, k)
        assert np.array_equal(_bits(a[1]["color"]), _bits(b[1]["color"])), mode
        for n in a[1]["grads"]:
            assert np.array_equal(_bits(a[1]["grads"][n]), _bits(b[1]["grads"][n])), (mode, n)
    with rasterizer.options(sort_all_bits=True):
        out = gpu_common.hip_forward_backward(_kw(name), count=True)
    assert np.array_equal(out["count"], ref.count) and np.array_equal(_bits(out["score"]), _bits(ref.score))
    assert np.array_equal(_bits(out["color"]), _bits(ref.color))


# ---- d. significance pass over mixed cameras ---------------------------------------------------------------------------------------------
def test_significance_pass_over_mixed_cameras():
    """prune_list over the four cameras and one orbit camera: summed hit counts equal the oracle's, the view-ordered float32 score sums
    are bit-identical to the oracle's sequential sum in the reference's order (prune.py:144-155 pops from the END of the list), and
    prune_list_sharded(streams=3) is bit-identical to prune_list."""
    from lightgaussian_amd import prune as lg_prune
    cc.check_preconditions()
    g = cc.gaussians()
    cams = [cc.camera(n) for n in cc.NAMES] + [syn.orbit_camera(1, 5, cc.W, cc.H, radius=5.0)]
    # activations evaluated ONCE on the CPU so that oracle and HIP path see identical inputs
    with torch.no_grad():
        xyz, sc, rot, op, feat = g.get_xyz, g.get_scaling, g.get_rotation, g.get_opacity, g.get_features.contiguous()

    class _PC:
        get_xyz = xyz.to(DEV); get_scaling = sc.to(DEV); get_rotation = rot.to(DEV); get_opacity = op.to(DEV); get_features = feat.to(DEV)
        active_sh_degree = 3; max_sh_degree = 3
    bg = torch.zeros(3, device=DEV); pipe = syn.PipelineParams()
    dcams = [c.to(DEV) for c in cams]
    with torch.no_grad():
        cnt, imp = lg_prune.prune_list(_PC, dcams, pipe, bg)
        cnt, imp = cnt.clone(), imp.clone()
        cnt3, imp3 = lg_prune.prune_list_sharded(_PC, dcams, pipe, bg, streams=3)
    cnt_o = imp_o = None
    for cam in cams[::-1]:
        kw = common.scene_kwargs(_Frozen(xyz, sc, rot, op, feat), cam, cc.W, cc.H)
        f = oracle.forward(count=True, **kw)
        if cnt_o is None:
            cnt_o, imp_o = f.count.copy(), f.score.copy()
        else:
            cnt_o += f.count; imp_o += f.score
    print(f"counts differ in {np.count_nonzero(cnt.cpu().numpy() != cnt_o)} Gaussians, score sums in "
          f"{np.count_nonzero(_bits(imp.cpu().numpy()) != _bits(imp_o))}; {int(cnt_o.sum())} hits over {len(cams)} views")
    assert int(cnt_o.sum()) > 50000
    assert np.array_equal(cnt.cpu().numpy(), cnt_o)
    assert np.array_equal(_bits(imp.cpu().numpy()), _bits(imp_o))
    assert torch.equal(cnt.to(torch.int32), cnt3.to(torch.int32)) and torch.equal(imp.view(torch.int32), imp3.view(torch.int32))


class _Frozen:
    """Getter surface of common.scene_kwargs over tensors that are already activated."""

    def __init__(self, xyz, sc, rot, op, feat):
        self.get_xyz, self.get_scaling, self.get_rotation, self.get_opacity, self.get_features = xyz, sc, rot, op, feat
