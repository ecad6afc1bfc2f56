"""CPU tests of the 3D smoothing filter (lightgaussian_amd/filter3d.py, csrc/lg_filter3d.h).

1. The g++ build of the per-camera term of lg_math.h (tests/cpu_harness/lg_filter3d_harness.cpp) against the float64 formula on the
   same float32 inputs: identical seen sets -- over EVERY row, the generator of tests/filter3d_common.py having dropped in float64 what
   lies within its margins of a decision -- and
       |t32 - t64| <= 4 * 2^-24 * (sum_k |vm_k2 p_k| + |vm_32|) / fx + 2^-23 t64
   (three fused multiply-adds, each rounding at most 2^-24 of a partial sum bounded by the sum of magnitudes; then fx = W / (2 tanfovx)
   and z / fx, one division each).
2. The apply formulas in float32 torch against float64 (this is err32, the float32 formula's own error, which the GPU test scales),
   and the closed-form backward against float64 autograd by the rule of tests/camera_grad_common.py.
3. The Python surface: option validation, the stale-filter ValueError, NotImplementedError with compute_cov3D_python, and that a model
   without the attribute never reaches the filter code."""
import math

import numpy as np
import pytest
import torch

import antialias_common as aa
import camera_grad_common as cg
import filter3d_common as fc
from common import syn
from lightgaussian_amd import filter3d, gaussian_renderer, rasterizer


# ---- 1. harness vs float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", fc.SIZES)
@pytest.mark.parametrize("V", fc.VS)
@pytest.mark.parametrize("N", fc.NS)
def test_harness_term_against_float64(N, V, size):
    W, H = size
    means, rows = fc.points(N, V, W, H)
    ref = fc.reference64(means, rows)
    assert ref["margin_ok"].all()
    if N >= 63:
        fc.assert_categories(ref, V, f"N{N} V{V} {W}x{H}")
    got = fc.run_harness(means, rows)
    assert np.array_equal(got["seen_nv"], ref["seen"]), "seen sets differ"          # every row, every camera
    err = np.abs(got["t"].astype(np.float64) - ref["t"])
    worst = float((err / ref["bound"]).max())
    print(f"N{N} V{V} {W}x{H}: max |t32 - t64| / bound = {worst:.3f}")
    assert (err <= ref["bound"]).all()
    # the filter: sqrtf(0.2f) (the constant: 2^-24, its argument 0.2f: 2^-25) times t (one product: 2^-24) on top of t's bound
    f64, seen64 = fc.filter64(ref)
    assert np.array_equal(got["seen"], seen64)
    tb = np.where(ref["seen"], ref["bound"], 0.0).max(1)
    fb = math.sqrt(0.2) * tb + 3 * 2.0 ** -24 * f64
    fb = np.where(seen64, fb, fb[seen64].max() if seen64.any() else 0.0)
    assert (np.abs(got["filter"] - f64) <= fb).all()


def test_harness_unseen_rows_get_the_maximum_and_nobody_seen_gives_zeros():
    means, rows = fc.points(257, 3, 70, 45)
    got = fc.run_harness(means, rows)
    assert got["seen"].any() and not got["seen"].all()
    top = got["filter"][got["seen"]].max()
    assert (got["filter"][~got["seen"]] == top).all() and top > 0
    away = np.ascontiguousarray(means[~got["seen"]])
    nobody = fc.run_harness(away, rows)
    assert not nobody["seen"].any() and not nobody["filter"].any()
    nan = means.copy()
    nan[::2, 1] = np.nan                                                               # a NaN compares false: unseen
    assert not fc.run_harness(nan, rows)["seen"][::2].any()


def test_one_focal_length_gives_min_depth_over_focal():
    """With cameras that share one focal length the filter is the published code's sqrt(0.2) * min depth / max focal."""
    cams = [syn.orbit_camera(k, 5, 70, 45) for k in range(5)]
    rows = fc.camera_rows(cams)
    means, _ = fc.points(257, 3, 70, 45)
    ref = fc.reference64(means, rows)
    seen = ref["seen"].any(1)
    depth = np.where(ref["seen"], ref["z"], np.inf).min(1)
    focal = (rows[:, 18].astype(np.float64) / (2.0 * rows[:, 16].astype(np.float64))).max()
    f64, _ = fc.filter64(ref)
    assert seen.any() and np.allclose(f64[seen], math.sqrt(0.2) * depth[seen] / focal, rtol=1e-12)


# ---- 2. apply: float32 formula vs float64; backward formulas vs float64 autograd -----------------------------------------------
@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("N", fc.NS)
def test_float32_formula_against_float64(N, raw):
    e = fc.err32(N, raw)
    print(f"N{N} raw={raw}: err32 scales {e['scaling']:.3e}, opacity {e['opacity']:.3e} (relative, activated domain)")
    # sanity only (the GPU test uses the figure itself): the chain is a few dozen float32 roundings of 2^-24 = 6e-8 each, the
    # logarithm's absolute error enters exp(0.5 log u) amplified by |log u| <= 12
    assert e["scaling"] <= 1e-5 and e["opacity"] <= 1e-5


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("N", [257, 1000])
def test_backward_formulas_against_float64_autograd(N, raw):
    ref = fc.grad_reference(N, raw)
    a_s, a_o, f = fc.err32(N, raw)["inputs"]
    gs, go = fc.upstream_gradients(N)
    for dd in (torch.float64, torch.float32):
        ds, do = fc.backward_formula(a_s.to(dd), a_o.to(dd), f.to(dd), gs.to(dd), go.to(dd), raw)
        got = {"scaling": ds.numpy(), "opacity": do.numpy()}
        if dd == torch.float64:
            for n in got:
                e = cg.rel_err(got[n], ref["float64"][n])
                print(f"N{N} raw={raw} float64 closed form d/d{n}: {e:.3e}")
                assert e <= 1e-12
        else:
            aa.assert_rule(got, ref, ("scaling", "opacity"), f"N{N} raw={raw} float32 closed form")


# ---- 3. the Python surface -----------------------------------------------------------------------------------------------------
def _model(n=16):
    return syn.make_gaussians(n, seed=3), syn.orbit_camera(0, 4, 33, 17), syn.PipelineParams(), torch.zeros(3)


def test_option_validation():
    assert rasterizer.resolve_options()["filter_3d"] is True
    assert rasterizer.resolve_options({"filter_3d": False})["filter_3d"] is False
    for bad in (1, "on", None):
        with pytest.raises(ValueError, match="filter_3d"):
            rasterizer.resolve_options({"filter_3d": bad})
        with pytest.raises(ValueError, match="filter_3d"):
            rasterizer.set_option("filter_3d", bad)
        with pytest.raises(ValueError, match="filter_3d"):
            rasterizer.options(filter_3d=bad)
    assert rasterizer.resolve_options()["filter_3d"] is True


@pytest.mark.parametrize("entry", ["render", "unfused", "count_render", "render_features"])
def test_a_stale_filter_raises_and_says_to_recompute(entry):
    g, cam, pipe, bg = _model()
    g.filter_3D = torch.full((g.num - 1, 1), 0.01)
    call = {"render": lambda o: gaussian_renderer.render(cam, g, pipe, bg, options=o),
            "unfused": lambda o: gaussian_renderer.render(cam, g, pipe, bg, options=dict(o or {}, fuse_getters=False)),
            "count_render": lambda o: gaussian_renderer.count_render(cam, g, pipe, bg, options=o),
            "render_features": lambda o: gaussian_renderer.render_features(cam, g, pipe, "depth", options=o)}[entry]
    with pytest.raises(ValueError, match="recompute"):
        call(None)
    with pytest.raises(ValueError, match="recompute"):
        filter3d.fuse_filter_3d(g)
    # with the option off the attribute is not looked at: the call gets as far as the rasterizer, which has no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        call({"filter_3d": False})


def test_compute_cov3d_python_with_a_filter_is_refused():
    g, cam, pipe, bg = _model()
    g.filter_3D = torch.full((g.num, 1), 0.01)
    pipe.compute_cov3D_python = True
    with pytest.raises(NotImplementedError, match="compute_cov3D_python"):
        gaussian_renderer.render(cam, g, pipe, bg)
    with pytest.raises(NotImplementedError, match="compute_cov3D_python"):
        gaussian_renderer.count_render(cam, g, pipe, bg)
    with pytest.raises(RuntimeError, match="HIP device"):
        gaussian_renderer.render(cam, g, pipe, bg, options={"filter_3d": False})


def test_a_model_without_the_attribute_takes_the_old_path(monkeypatch):
    calls = []

    class Reached(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            calls.append(name)
            raise Reached(name)
        return f

    monkeypatch.setattr(filter3d, "apply_filter_3d", spy("raw"))
    monkeypatch.setattr(filter3d, "apply_filter_3d_activated", spy("activated"))
    g, cam, pipe, bg = _model()
    assert not hasattr(g, "filter_3D")
    for opts in (None, {"fuse_getters": False}):
        with pytest.raises(RuntimeError, match="HIP device"):
            gaussian_renderer.render(cam, g, pipe, bg, options=opts)
    with pytest.raises(RuntimeError, match="HIP device"):
        gaussian_renderer.count_render(cam, g, pipe, bg)
    assert calls == []
    g.filter_3D = None                              # an attribute that holds nothing is no filter either
    with pytest.raises(RuntimeError, match="HIP device"):
        gaussian_renderer.render(cam, g, pipe, bg)
    assert calls == []
    # ... and with the attribute the fused path applies it raw -> raw, every other path on the activated getters
    g.filter_3D = torch.full((g.num, 1), 0.01)
    with pytest.raises(Reached):
        gaussian_renderer.render(cam, g, pipe, bg)
    with pytest.raises(Reached):
        gaussian_renderer.render(cam, g, pipe, bg, options={"fuse_getters": False})
    with pytest.raises(Reached):
        gaussian_renderer.count_render(cam, g, pipe, bg)
    assert calls == ["raw", "activated", "activated"]


def test_camera_table_layout():
    cams = fc.cameras(3, 70, 45)
    table = filter3d.camera_table(cams)
    assert table.dtype == torch.uint8 and tuple(table.shape) == (3, 80)
    rows = fc.camera_rows(cams)
    raw = table.numpy()
    assert np.array_equal(raw[:, :72].copy().view(np.float32), rows[:, :18])
    assert np.array_equal(raw[:, 72:].copy().view(np.int32), rows[:, 18:].astype(np.int32))
    with pytest.raises(ValueError):
        filter3d.camera_table([])
