"""lg_blend_features without a GPU: the declarations and their binding, the argument checks that come before any device call
(C ABI and Python), and lg_feature_step -- the per-pixel step the kernels run, compiled from the product's lg_math.h with g++ --
over whole small images against the oracle, bit for bit, channel triple by channel triple."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import common
import features_common
from common import bits as _bits
from common import syn
from lightgaussian_amd import _lib, features, gaussian_renderer
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings
from oracle import oracle

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")


def test_symbols_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("lg_features_scratch_bytes", 3), ("lg_blend_features", 11), ("lg_blend_features_backward", 10)):
        m = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, f"{name} is not declared in include/lightgaussian.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.EXPORTS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == nargs
    assert int(re.search(r"#define LG_FEATURES_MAX (\d+)", src).group(1)) == _lib.FEATURES_MAX == features.FEATURES_MAX == 64
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.lg_abi_version() == 7
    assert callable(gaussian_renderer.render_features) and callable(features.blend_features)


def test_scratch_size_covers_the_rows_and_chunks_over_channels():
    lib = _lib.load()
    assert lib.lg_features_scratch_bytes(1000, 5000, 7) >= 5000 * 7 * 4
    assert lib.lg_features_scratch_bytes(1000, 5000, 64) >= 5000 * 64 * 4
    assert lib.lg_features_scratch_bytes(0, 0, 3) > 0
    assert lib.lg_features_scratch_bytes(1000, 5000, 0) == 0 and lib.lg_features_scratch_bytes(1000, 5000, 65) == 0
    # beyond 1 GiB of rows the channels go in chunks (at least 16 at a time): the scratch stops growing with C
    R = 20_000_000
    assert lib.lg_features_scratch_bytes(1, R, 64) < R * 64 * 4
    assert lib.lg_features_scratch_bytes(1, R, 64) >= R * 16 * 4


def _view(**kw):
    a = dict(H=32, W=32, flags=0, seg=0)
    a.update(kw)
    return _lib.lg_view(a["H"], a["W"], 1.0, 1.0, None, 1.0, None, None, 0, None, 0, a["flags"], a["seg"])


P = 0x1000      # a non-null pointer that must never be dereferenced


@pytest.mark.parametrize("what, kw", [
    ("LG_FEATURES_MAX", dict(C=0)), ("LG_FEATURES_MAX", dict(C=65)), ("LG_FEATURES_MAX", dict(C=-3)),
    ("null view", dict(view=None)), ("N out of range", dict(N=-1)), ("num_rendered", dict(R=-1)), ("num_rendered", dict(R=1 << 30)),
    ("image size", dict(view=_view(W=0))), ("segment_length", dict(view=_view(seg=100))),
    ("geom", dict(geom=None)), ("binning", dict(binning=None)), ("missing", dict(feats=None)), ("missing", dict(out=None)),
])
def test_c_abi_refuses_bad_arguments_before_any_device_call(what, kw):
    """This process has no GPU: a call that reached the HIP runtime would come back as LG_ERR_DEVICE."""
    lib = _lib.load()
    a = dict(view=_view(), N=10, geom=P, binning=P, R=100, feats=P, C=3, out=P)
    a.update(kw)
    v = None if a["view"] is None else C.byref(a["view"])
    assert lib.lg_blend_features(v, a["N"], a["geom"], a["binning"], a["R"], a["feats"], a["C"], None, a["out"], None, None) == _lib.LG_ERR_INVALID_ARGUMENT
    msg = lib.lg_last_error().decode()
    assert "lg_blend_features" in msg and what in msg, msg
    if "feats" in kw or "out" in kw:
        return
    assert lib.lg_blend_features_backward(v, a["N"], a["geom"], a["binning"], a["R"], P, a["C"], P, P, None) == _lib.LG_ERR_INVALID_ARGUMENT
    msg = lib.lg_last_error().decode()
    assert "lg_blend_features_backward" in msg and what in msg, msg


def test_c_abi_backward_needs_its_buffers_and_an_empty_model_is_ok():
    lib = _lib.load()
    v = _view()
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.lg_blend_features_backward(C.byref(v), 10, P, P, 100, args[0], 3, args[1], args[2], None) == _lib.LG_ERR_INVALID_ARGUMENT
        assert "missing" in lib.lg_last_error().decode()
    assert lib.lg_blend_features_backward(C.byref(v), 0, P, None, 0, None, 3, None, None, None) == _lib.LG_OK


def _rs():
    return GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False, False)


def _geometry(n=4):
    return dict(means3D=torch.zeros(n, 3), opacities=torch.ones(n, 1), scales=torch.ones(n, 3), rotations=torch.ones(n, 4),
                colors_precomp=torch.ones(n, 3))


@pytest.mark.parametrize("feats, bg, exc, match", [
    (torch.zeros(4, 0), None, ValueError, "0 channels"),
    (torch.zeros(4, 65), None, ValueError, "65 channels"),
    (torch.zeros(4, 3, dtype=torch.float64), None, TypeError, "float32"),
    (torch.zeros(4, 3, dtype=torch.float16), None, TypeError, "float32"),
    (torch.zeros(3, 4).t(), None, ValueError, "contiguous"),
    (torch.zeros(4, 6)[:, ::2], None, ValueError, "contiguous"),
    (torch.zeros(4, 3, 1), None, ValueError, r"\[N, C\]"),
    (np.zeros((4, 3), np.float32), None, TypeError, "torch tensor"),
    (torch.zeros(4, 3), torch.zeros(4), ValueError, "bg_features"),
    (torch.zeros(4, 3), torch.zeros(3, dtype=torch.float64), ValueError, "bg_features"),
    (torch.zeros(4, 3), None, RuntimeError, "no CPU path"),
])
def test_python_refuses_bad_features_before_any_device_call(feats, bg, exc, match):
    with pytest.raises(exc, match=match):
        features.blend_features(_rs(), feats, bg_features=bg, **_geometry())


def test_python_refuses_count_settings_and_unknown_feature_names():
    with pytest.raises(ValueError, match="f_count"):
        features.blend_features(_rs()._replace(f_count=True), torch.zeros(4, 3), **_geometry())
    g = syn.make_gaussians(8)
    cam = syn.orbit_camera(0, 4, 16, 16)
    with pytest.raises(ValueError, match="'depth'"):
        gaussian_renderer.render_features(cam, g, syn.PipelineParams(), "normals")
    with pytest.raises(RuntimeError, match="no CPU path"):
        gaussian_renderer.render_features(cam, g, syn.PipelineParams(), "depth")


def test_feature_step_is_the_three_tests_of_the_blend_pair():
    lib = features_common.harness()

    def step(power, alpha, T):
        t, w = C.c_float(T), C.c_float(-1.0)
        return lib.h_feature_step(power, alpha, C.byref(t), C.byref(w)), t.value, w.value

    assert step(1e-9, 0.5, 1.0) == (0, 1.0, -1.0)                         # power > 0
    assert step(float("nan"), 0.5, 1.0) == (0, 1.0, -1.0)                 # a NaN power is rejected
    assert step(-1.0, np.float32(1 / 255) - np.float32(1e-9), 1.0) == (0, 1.0, -1.0)
    r, T, w = step(-1.0, float(np.float32(1 / 255)), 1.0)                  # alpha == 1/255 contributes
    assert r == 1 and w == np.float32(1 / 255) and T == np.float32(1) - np.float32(1 / 255)
    assert step(-1.0, 0.99, 0.005)[0] == 2 and step(-1.0, 0.99, 0.005)[1:] == (np.float32(0.005), -1.0)   # T (1 - alpha) < 1e-4: done, state untouched
    r, T, w = step(0.0, 0.5, 0.25)
    assert (r, T, w) == (1, 0.125, 0.125)


# the scenes of tests/test_gpu_features.py, plus one with a last contributor beyond list position 500
SCENES = [dict(N=300, W=70, H=45, scale=0.06, opm=0.0), dict(N=64, W=33, H=17, scale=0.1, opm=0.0),
          dict(N=400, W=48, H=48, scale=0.25, opm=-2.0), dict(N=3000, W=128, H=128, scale=0.03, opm=1.0, seed=5, full=True)]


@pytest.mark.parametrize("c", SCENES, ids=lambda c: f"N{c['N']}_{c['W']}x{c['H']}")
def test_whole_images_equal_the_oracle_triple_by_triple(c):
    if c.get("full"):
        g = syn.make_gaussians(c["N"], seed=c["seed"], log_scale_mean=math.log(c["scale"]), opacity_mean=c["opm"])
    else:
        g = syn.make_gaussians(c["N"], seed=3, extent=(1.5, 1.0, 1.5), log_scale_mean=math.log(c["scale"]), opacity_mean=c["opm"])
    W, H = c["W"], c["H"]
    cam = syn.orbit_camera(1, 7, W, H, radius=4.0)
    kw = common.scene_kwargs(g, cam, W, H)
    Cn = 7
    rs = np.random.RandomState(11)
    F = rs.randn(c["N"], Cn).astype(np.float32)
    bg = rs.randn(Cn).astype(np.float32)
    dout = rs.randn(Cn, H, W).astype(np.float32)
    out0, alpha, radii, ninst, dF = features_common.blend_features(kw, F, dL_dout=dout)
    outb, alpha_b, _r, _n = features_common.blend_features(kw, F, bg)
    assert np.array_equal(_bits(alpha), _bits(alpha_b))
    Fp = np.concatenate([F, np.zeros((c["N"], 2), np.float32)], 1)
    dp = np.concatenate([dout, np.zeros((2, H, W), np.float32)], 0)
    bgp = np.concatenate([bg, np.zeros(2, np.float32)])
    final_T = None
    for c0 in range(0, Cn, 3):
        k = min(3, Cn - c0)
        kwc = common.scene_kwargs(g, cam, W, H, precolor=torch.from_numpy(Fp[:, c0:c0 + 3].copy()))
        f0 = oracle.forward(**kwc)
        assert np.array_equal(radii, f0.radii) and ninst <= f0.num_rendered
        assert np.array_equal(_bits(out0[c0:c0 + k]), _bits(f0.color[:k])), c0
        # the gradient with respect to the channels is linear in the weights: sum_pixels w dL/dout is the oracle's colors_precomp gradient
        ref = oracle.backward(f0, dp[c0:c0 + 3])["colors_precomp"][:, :k]
        bound = 1e-4 * np.abs(ref) + 2e-5 * np.abs(ref).max()
        assert (np.abs(dF[:, c0:c0 + k] - ref) <= bound).all(), c0
        assert not dF[radii == 0].any()
        kwc["bg"] = bgp[c0:c0 + 3].copy()
        assert np.array_equal(_bits(outb[c0:c0 + k]), _bits(oracle.forward(**kwc).color[:k])), c0
        final_T = f0.saved["final_T"].reshape(H, W)
    ones = np.zeros((c["N"], 3), np.float32); ones[:, 0] = 1.0
    fo = oracle.forward(**common.scene_kwargs(g, cam, W, H, precolor=torch.from_numpy(ones)))
    assert np.array_equal(_bits(alpha), _bits(fo.color[0]))               # alpha IS the blended channel of ones ...
    assert np.abs(alpha - (1.0 - final_T)).max() <= 6e-7                  # ... and 1 - T up to rounding
    assert float(alpha.max()) > 0.5
