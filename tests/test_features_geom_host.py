"""lg_backward_features without a GPU: the declarations and their binding, every argument refusal that comes before a device call
(C ABI and Python), and lg_feature_bwd_step -- the per-pixel step of lg_features_bwd_geom, compiled from the product's lg_math.h
with g++ -- replayed over whole images and chained with the product's lg_rows_to_grads / lg_backward_geom / lg_backward_cov3d
against (a) the oracle's backward summed over channel triples, under the rule of test_backward_parity, and (b) the float64 autograd
twin of oracle/torch_dense.py rendering [z, 1, 0] for the "depth" path, at the 1e-4 of tests/test_oracle.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import common
import features_common
import features_geom_common as fg
from common import syn
from lightgaussian_amd import _lib, features, gaussian_renderer
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings
from lightgaussian_amd.vectree import CompressedGaussians, TrainableCompressed
from oracle import oracle, torch_dense

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")


def test_symbols_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("lg_backward_features_scratch_bytes", 3), ("lg_backward_features", 25)):
        m = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, f"{name} is not declared in include/lightgaussian.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.EXPORTS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.lg_backward_features_scratch_bytes.restype is C.c_size_t and lib.lg_backward_features.restype is C.c_int
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.lg_abi_version() == 7      # purely additive
    # the moment rows of lg_backward, then the partial rows of lg_blend_features_backward
    assert lib.lg_backward_features_scratch_bytes(1000, 5000, 7) == lib.lg_backward_scratch_bytes(1000, 5000) + lib.lg_features_scratch_bytes(1000, 5000, 7)
    assert lib.lg_backward_features_scratch_bytes(1000, 5000, 0) == 0 and lib.lg_backward_features_scratch_bytes(1000, 5000, 65) == 0
    assert lib.lg_backward_features_scratch_bytes(1000, -1, 3) == 0


P = 0x1000      # a non-null pointer that must never be dereferenced


def _view(**kw):
    a = dict(H=32, W=32, flags=0, seg=0)
    a.update(kw)
    return _lib.lg_view(a["H"], a["W"], 1.0, 1.0, P, 1.0, P, P, 0, P, 0, a["flags"], a["seg"])


def _call(lib, **kw):
    a = dict(view=_view(), N=10, M=0, shs=None, colors=P, scales=P, rots=P, cov=None, radii=P, geom=P, binning=P, img=P, R=100, dcolor=P, feats=P,
             C=3, dout=P, dalpha=P, g_m2=P, g_m3=P, g_sh=None, g_col=P, g_op=P, g_sc=P, g_rot=P, g_cov=None, g_feat=P, scratch=P, gauss=True)
    a.update(kw)
    g = _lib.lg_gaussians(a["N"], a["M"], P, a["shs"], a["colors"], P, a["scales"], a["rots"], a["cov"], None)
    v = None if a["view"] is None else C.byref(a["view"])
    return lib.lg_backward_features(v, C.byref(g) if a["gauss"] else None, a["radii"], a["geom"], a["binning"], a["img"], a["R"], a["dcolor"],
                                    a["feats"], a["C"], None, a["dout"], a["dalpha"], a["g_m2"], a["g_m3"], a["g_sh"], a["g_col"], a["g_op"],
                                    a["g_sc"], a["g_rot"], a["g_cov"], None, a["g_feat"], a["scratch"], None)


@pytest.mark.parametrize("what, kw", [
    ("LG_FEATURES_MAX", dict(C=0)), ("LG_FEATURES_MAX", dict(C=65)), ("null view", dict(view=None)), ("null gaussians", dict(gauss=False)),
    ("N out of range", dict(N=-1)), ("num_rendered", dict(R=-1)), ("num_rendered", dict(R=1 << 30)), ("image size", dict(view=_view(H=0))),
    ("segment_length", dict(view=_view(seg=100))), ("geom", dict(geom=None)), ("binning", dict(binning=None)),
    ("missing features", dict(feats=None)), ("missing features", dict(feats=None, dout=None)), ("dL_dfeatures without dL_dout", dict(dout=None)),
    ("missing buffer", dict(radii=None)), ("missing buffer", dict(img=None)), ("missing buffer", dict(g_m2=None)), ("missing buffer", dict(g_m3=None)),
    ("missing buffer", dict(g_op=None)), ("missing buffer", dict(scratch=None)),
    ("missing gradient output", dict(g_col=None)), ("missing gradient output", dict(g_sc=None)), ("missing gradient output", dict(g_rot=None)),
    ("missing gradient output", dict(scales=None, rots=None, cov=P)), ("missing gradient output", dict(colors=None, shs=P, M=16, g_col=None)),
])
def test_c_abi_refuses_bad_arguments_before_any_device_call(what, kw):
    """This process has no GPU: a call that reached the HIP runtime would come back as LG_ERR_DEVICE."""
    lib = _lib.load()
    assert _call(lib, **kw) == _lib.LG_ERR_INVALID_ARGUMENT
    assert what in lib.lg_last_error().decode(), lib.lg_last_error().decode()


def test_c_abi_an_empty_model_is_ok_and_no_image_gradient_is_an_argument_set_of_its_own():
    lib = _lib.load()
    assert _call(lib, N=0) == _lib.LG_OK
    # all three image gradients NULL is a legal call (zero gradients): with every buffer in place it gets past the argument checks and only
    # then needs a device, which this process does not have
    assert _call(lib, dcolor=None, dout=None, dalpha=None, g_feat=None) == _lib.LG_ERR_DEVICE


def _rs():
    return GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False, False)


def _geometry(n=4):
    return dict(means3D=torch.zeros(n, 3), opacities=torch.ones(n, 1), scales=torch.ones(n, 3), rotations=torch.ones(n, 4),
                colors_precomp=torch.ones(n, 3))


@pytest.mark.parametrize("feats, bg, exc, match", [
    (torch.zeros(4, 0), None, ValueError, "0 channels"),
    (torch.zeros(4, 65), None, ValueError, "65 channels"),
    (torch.zeros(4, 3, dtype=torch.float64), None, TypeError, "float32"),
    (torch.zeros(3, 4).t(), None, ValueError, "contiguous"),
    (torch.zeros(4, 3, 1), None, ValueError, r"\[N, C\]"),
    (np.zeros((4, 3), np.float32), None, TypeError, "torch tensor"),
    (torch.zeros(4, 3), torch.zeros(4), ValueError, "bg_features"),
    (torch.zeros(4, 3), None, RuntimeError, "no CPU path"),
])
def test_python_refuses_bad_features_before_any_device_call(feats, bg, exc, match):
    with pytest.raises(exc, match=match):
        features.blend_features(_rs(), feats, bg_features=bg, geometry_grad=True, **_geometry())


def test_python_refuses_what_the_mode_does_not_cover():
    with pytest.raises(ValueError, match="f_count"):
        features.blend_features(_rs()._replace(f_count=True), torch.zeros(4, 3), geometry_grad=True, **_geometry())
    with pytest.raises(ValueError, match="geometry_grad=True"):
        features.blend_features(_rs(), torch.zeros(4, 3), means2D=torch.zeros(4, 3), **_geometry())
    cam = syn.orbit_camera(0, 4, 16, 16)
    for cls in (CompressedGaussians, TrainableCompressed):
        with pytest.raises(NotImplementedError, match="to_dense"):
            gaussian_renderer.render_features(cam, object.__new__(cls), syn.PipelineParams(), "depth", geometry_grad=True)
    g = syn.make_gaussians(8)
    with pytest.raises(ValueError, match="'depth'"):
        gaussian_renderer.render_features(cam, g, syn.PipelineParams(), "normals", geometry_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gaussian_renderer.render_features(cam, g, syn.PipelineParams(), "depth", geometry_grad=True)


def test_bwd_step_rejects_what_the_forward_rejects_and_computes_the_documented_recurrence():
    lib = fg.harness()
    f32 = np.float32

    def step(live, power, G, alpha, dx, dy, q, Tfb, T, S):
        t, s, w = C.c_float(T), C.c_float(S), C.c_float(-1.0)
        m = np.full(6, 0.5, np.float32)
        r = lib.h_feature_bwd_step(live, power, G, alpha, dx, dy, q, Tfb, C.byref(t), C.byref(s), m.ctypes.data_as(C.c_void_p), C.byref(w))
        return r, t.value, s.value, w.value, m

    untouched = (0, 0.5, 0.25, -1.0)
    for args in ((0, -1.0, 0.3, 0.3), (1, 1e-9, 0.3, 0.3), (1, float("nan"), 0.3, 0.3), (1, -1.0, 0.3, float(f32(1 / 255) - f32(1e-9)))):
        r = step(args[0], args[1], args[2], args[3], 1.0, 2.0, 3.0, 0.1, 0.5, 0.25)
        assert r[:4] == untouched and (r[4] == 0.5).all(), args
    # one step by hand, every operation rounded to float32 on its own (contraction is off)
    G, alpha, dx, dy, q, Tfb, T, S = f32(0.6), f32(0.3), f32(1.5), f32(-2.0), f32(3.0), f32(0.125), f32(0.35), f32(0.25)
    r, Tn, Sn, w, m = step(1, -0.5, G, alpha, dx, dy, q, Tfb, T, S)
    inv = f32(1) / (f32(1) - alpha); eTn = T * inv; d = q - S
    t = G * (d * eTn - Tfb * inv)
    assert r == 1 and Tn == eTn and Sn == S + alpha * d and w == alpha * eTn
    tdx, tdy = t * dx, t * dy
    assert np.array_equal(m, np.array([tdx, tdy, tdx * dx, tdx * dy, tdy * dy, t], np.float32) + f32(0.5))   # accumulated into m
    # alpha == 1/255 contributes; the 0.99 clamp is straight through (t uses G, not d alpha / d G)
    assert step(1, -1.0, 0.3, float(f32(1 / 255)), 1.0, 1.0, 1.0, 0.0, 0.5, 0.0)[0] == 1
    assert step(1, 0.0, 1.0, 0.99, 0.0, 0.0, 1.0, 0.0, 0.5, 0.0)[4][5] == f32(0.5) + f32(1.0) * (f32(1.0) * (f32(0.5) * (f32(1) / (f32(1) - f32(0.99)))))


HOST_SCENES = ["N300_70x45", "N64_33x17", "N400_48x48"]
CN = 17


@pytest.mark.parametrize("name", HOST_SCENES)
def test_whole_image_replay_matches_the_summed_oracle_backward(name):
    c, g, cam = fg.scene(name)
    N, W, H = c["N"], c["W"], c["H"]
    kw = common.scene_kwargs(g, cam, W, H)
    F, bgf, dout, dalpha, _dc = fg.loss_inputs(N, CN, H, W, True)
    gr, out, alpha, radii, _early = fg.harness_grads(kw, F, bgf, dout, dalpha)
    # the forward half of the harness is the one tests/test_features_host.py pins against the oracle
    out0, alpha0, radii0, _n = features_common.blend_features(kw, F, bgf)
    assert np.array_equal(out, out0) and np.array_equal(alpha, alpha0) and np.array_equal(radii, radii0)
    fg.assert_within(gr, fg.reference(name, CN, True, "oa"), name)
    for n in fg.GEOMETRY:
        assert not gr[n][radii == 0].any(), n
        assert np.abs(gr[n]).max() > 0, n
    # linearity: out alone and alpha alone add up to both (separate walks, each with its own S and Tfb)
    go = fg.harness_grads(kw, F, bgf, dout, None)[0]
    ga = fg.harness_grads(kw, F, bgf, None, dalpha)[0]
    fg.assert_within(go, fg.reference(name, CN, True, "o"), name + " out")
    fg.assert_within(ga, fg.reference(name, CN, True, "a"), name + " alpha")
    for n in fg.GEOMETRY:
        s = go[n].astype(np.float64) + ga[n]
        assert np.abs(s - gr[n]).max() <= 1e-5 * np.abs(gr[n]).max(), n


def test_the_opaque_scene_has_pixels_that_end_before_their_list():
    name = "N200_40x40_opaque"
    c, g, cam = fg.scene(name)
    N, W, H = c["N"], c["W"], c["H"]
    assert fg.early_pixels(name) > 0
    kw = common.scene_kwargs(g, cam, W, H)
    F, bgf, dout, dalpha, _dc = fg.loss_inputs(N, CN, H, W, True)
    gr, _o, _a, _r, early = fg.harness_grads(kw, F, bgf, dout, dalpha)
    assert early > 0
    fg.assert_within(gr, fg.reference(name, CN, True, "oa"), name)


def test_depth_and_alpha_gradients_match_the_float64_autograd_twin():
    """"depth": features = view-space z of means3D.  The dense twin renders colors_precomp = [z(means3D), 1, 0] in float64 with autograd:
    channel 0 is the depth numerator, channel 1 alpha, and autograd carries a loss on depth = num / alpha.clamp_min(1e-6) and on alpha to
    every input -- through the blending weights AND through z.  The harness chain gets the same loss as dL_dout = gd / alpha,
    dL_dalpha = ga - gd num / alpha^2 (where alpha > 1e-6), plus dF z'(means3D) for the feature's own dependence on the mean."""
    name = "N64_33x17"
    c, g, cam = fg.scene(name)
    N, W, H = c["N"], c["W"], c["H"]
    dd = torch.float64
    rs = np.random.RandomState(5)
    gd, ga = rs.randn(H, W), rs.randn(H, W)
    t = dict(means3D=g.get_xyz.to(dd).detach().requires_grad_(), opacities=g.get_opacity.to(dd).detach().requires_grad_(),
             scales=g.get_scaling.to(dd).detach().requires_grad_(), rotations=g.get_rotation.to(dd).detach().requires_grad_())
    vm = cam.world_view_transform.to(dd)
    z = t["means3D"] @ vm[:3, 2:3] + vm[3, 2]
    import math
    means2D = torch.zeros(N, 3, dtype=dd, requires_grad=True)
    color, radii, _cnt = torch_dense.render_dense(means2D=means2D, W=W, H=H, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                                  bg=torch.zeros(3, dtype=dd), viewmatrix=vm, projmatrix=cam.full_proj_transform.to(dd),
                                                  campos=cam.camera_center.to(dd), colors_precomp=torch.cat([z, torch.ones_like(z), torch.zeros_like(z)], 1), **t)
    depth = color[0] / color[1].clamp_min(1e-6)
    (depth * torch.from_numpy(gd) + color[1] * torch.from_numpy(ga)).sum().backward()

    kw = common.scene_kwargs(g, cam, W, H)
    vm32 = cam.world_view_transform.numpy().astype(np.float32)
    zf = (kw["means3D"].astype(np.float32) @ vm32[:3, 2:3] + vm32[3, 2]).astype(np.float32)
    out, alpha, radii_h, _n = features_common.blend_features(kw, zf)
    assert np.array_equal(radii_h, radii.numpy())
    assert np.abs(out[0] - color[0].detach().numpy()).max() <= 1e-5 * np.abs(out).max() and np.abs(alpha - color[1].detach().numpy()).max() <= 1e-5
    a64, n64 = alpha.astype(np.float64), out[0].astype(np.float64)
    ac = np.maximum(a64, 1e-6)
    dout = (gd / ac)[None].astype(np.float32)
    dalpha = (ga - np.where(a64 > 1e-6, gd * n64 / (ac * ac), 0.0)).astype(np.float32)
    gr = fg.harness_grads(kw, zf, None, dout, dalpha)[0]
    dF = features_common.blend_features(kw, zf, dL_dout=dout)[4]
    gr["means3D"] = gr["means3D"].astype(np.float64) + dF * vm32[:3, 2].astype(np.float64)[None]
    ref = dict(t, means2D=means2D)
    for n in fg.GEOMETRY:
        r = ref[n].grad.numpy().reshape(gr[n].shape)
        err = fg.rel_err(gr[n], r)
        print(f"{n}: rel err against the dense twin {err:.3e}")
        assert np.abs(r).max() > 0 and err < 1e-4, f"{n}: {err}"


CAMERA = "pitched_rolled"     # tests/camera_common.py: every entry of the view rotation is non-zero, the depth gradient gets a y component


def test_whole_image_replay_under_a_pitched_and_rolled_camera():
    """The reference side of tests/test_gpu_features_geom.py's camera test, verified here first: the replay of lg_feature_bwd_step and the
    per-Gaussian chain against the summed oracle backward under a camera whose view rotation has no zero entry."""
    name = "N300_70x45"
    c, g, cam = fg.scene(name, CAMERA)
    N, W, H = c["N"], c["W"], c["H"]
    kw = common.scene_kwargs(g, cam, W, H)
    assert np.abs(kw["viewmatrix"][:3, :3]).min() >= 0.03
    F, bgf, dout, dalpha, _dc = fg.loss_inputs(N, CN, H, W, True)
    gr, out, alpha, radii, _early = fg.harness_grads(kw, F, bgf, dout, dalpha)
    out0, alpha0, radii0, _n = features_common.blend_features(kw, F, bgf)
    assert np.array_equal(out, out0) and np.array_equal(alpha, alpha0) and np.array_equal(radii, radii0)
    assert (radii > 0).sum() >= 100
    fg.assert_within(gr, fg.reference(name, CN, True, "oa", camera=CAMERA), f"{name} {CAMERA}")
    # the orbit reference is another key of the cache, not this one
    assert fg.reference(name, CN, True, "oa", camera=CAMERA) is not fg.reference(name, CN, True, "oa")
    for n in fg.GEOMETRY:
        assert not gr[n][radii == 0].any(), n
        assert np.abs(gr[n]).max() > 0, n


def test_depth_map_and_gradient_under_a_pitched_and_rolled_camera():
    """fg.dense_depth_reference (the GPU test's reference: gradients with respect to the RAW parameters, through the activations) against
    the harness chain of test_depth_and_alpha_gradients_match_the_float64_autograd_twin, carried through the activations by hand in
    float64: exp for scales, sigmoid for opacities, normalisation for rotations.  With this camera vm[6] is not 0: z depends on world y."""
    name = "N300_70x45"
    c, g, cam = fg.scene(name, CAMERA)
    N, W, H = c["N"], c["W"], c["H"]
    ref = fg.dense_depth_reference(name, CAMERA)
    gd, ga = fg.depth_loss_maps(H, W)
    kw = common.scene_kwargs(g, cam, W, H)
    vm32 = cam.world_view_transform.numpy().astype(np.float32)
    assert abs(float(vm32[1, 2])) >= 0.03
    zf = (kw["means3D"].astype(np.float32) @ vm32[:3, 2:3] + vm32[3, 2]).astype(np.float32)
    out, alpha, radii_h, _n = features_common.blend_features(kw, zf)
    assert np.array_equal(radii_h, ref["maps"][2])
    fg.assert_depth_maps(out[0], alpha, ref["maps"], f"{name} {CAMERA}")
    a64, n64 = alpha.astype(np.float64), out[0].astype(np.float64)
    ac = np.maximum(a64, 1e-6)
    dout = (gd / ac)[None].astype(np.float32)
    dalpha = (ga - np.where(a64 > 1e-6, gd * n64 / (ac * ac), 0.0)).astype(np.float32)
    gr = fg.harness_grads(kw, zf, None, dout, dalpha)[0]
    dF = features_common.blend_features(kw, zf, dL_dout=dout)[4]
    g_xyz = gr["means3D"].astype(np.float64) + dF * vm32[:3, 2].astype(np.float64)[None]
    s = g._scaling.double().exp().numpy(); o = torch.sigmoid(g._opacity.double()).numpy(); r = g._rotation.double().numpy()
    nr = np.linalg.norm(r, axis=1, keepdims=True); q = r / nr
    g_rot = gr["rotations"].astype(np.float64)
    got = {"_xyz": g_xyz, "_opacity": gr["opacities"].astype(np.float64) * o * (1.0 - o), "_scaling": gr["scales"].astype(np.float64) * s,
           "_rotation": (g_rot - q * (q * g_rot).sum(1, keepdims=True)) / nr}
    assert np.abs(got["_xyz"][:, 1]).max() > 0
    fg.assert_within(got, ref, f"depth {CAMERA}", names=fg.RAW)
    # the default camera is another key, with today's values
    assert fg.dense_depth_reference(name) is not ref
