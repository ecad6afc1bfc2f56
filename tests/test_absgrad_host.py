"""No GPU: the absolute mean-gradient arithmetic of lg_math.h (lg_abs_pair, lg_abs_rows_to_grad; g++ build of
tests/cpu_harness/lg_absgrad_harness.cpp) against float64, and the surface of the feature: header, binding, exported symbol, the
`absgrad` option, densify.accumulate_stats(absgrad=True) on CPU tensors and run.py's --absgrad.

Bounds.  Each helper is a handful of float32 operations on float32 inputs; the float64 reference is evaluated from the same float32
inputs, so its own error (2^-53 relative per operation) is nothing beside an ulp of float32.  ULPS = 4 float32 ulps of the result, as the
issue sets it.  lg_abs_pair's two terms 2 ha dx and nb dy have opposite signs for half of all pixels and cancel; the helper carries
the rounding error of one product through the sum (lg_two_prod_sum), which is what keeps the error at ulps of the RESULT."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import absgrad_common as ab
import common
from lightgaussian_amd import _lib, densify, rasterizer
from lightgaussian_amd import run as lg_run

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")
ULPS = 4.0


def _ulp32(x):
    """Spacing of float32 at |x| (x float64)."""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _pairs(n, seed):
    """Random pairs: t of both signs over 1e-6 .. 1e2 with exact zeros, offsets of +-20 pixels (a tenth placed where the x terms cancel) with dx = dy = 0 among them, conics
    (A, B, C) with A, C log-uniform over 1e-4 .. 1e2 and |B| < sqrt(A C) of both signs, opacities in (1/255, 1]."""
    r = np.random.default_rng(seed)
    t = (np.exp(r.uniform(np.log(1e-6), np.log(1e2), n)) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    t[::17] = 0.0
    dx, dy = r.uniform(-20, 20, n).astype(np.float32), r.uniform(-20, 20, n).astype(np.float32)
    dx[5::23] = 0.0; dy[5::23] = 0.0            # dx = dy = 0
    dx[7::29] = 0.0                              # and one of them alone
    A, Cc = np.exp(r.uniform(np.log(1e-4), np.log(1e2), n)), np.exp(r.uniform(np.log(1e-4), np.log(1e2), n))
    B = r.uniform(-0.99, 0.99, n) * np.sqrt(A * Cc)
    ha, nb, hc = (-0.5 * A).astype(np.float32), (-B).astype(np.float32), (-0.5 * Cc).astype(np.float32)
    op = r.uniform(1.0 / 255.0, 1.0, n).astype(np.float32)
    # every eleventh pair sits where the two x terms cancel 1e2- to 1e4-fold: nb dy = -2 ha dx (1 + delta), which random offsets
    # reach only a few times in 1e5 (a pixel on the line through the centre on which dL/dmean2D.x changes sign)
    k = np.arange(3, n, 11)
    k = k[(nb[k] != 0) & (dx[k] != 0)]
    delta = np.exp(r.uniform(np.log(1e-4), np.log(1e-2), len(k))) * r.choice([-1.0, 1.0], len(k))
    dy[k] = (-2.0 * ha[k].astype(np.float64) * dx[k] / nb[k] * (1.0 + delta)).astype(np.float32)
    return t, dx, dy, ha, nb, hc, op


def _abs_pair(t, dx, dy, ha, nb, hc):
    out = np.zeros((len(t), 2), np.float32)
    ab.harness().h_abs_pair(len(t), *(ab.ptr(a) for a in (t, dx, dy, ha, nb, hc, out)))
    return out


def _exact(t, dx, dy, ha, nb, hc):
    """float64, from the float32 inputs: the two signed per-pair terms (pixel units, without the opacity)."""
    t, dx, dy, ha, nb, hc = (a.astype(np.float64) for a in (t, dx, dy, ha, nb, hc))
    return np.stack([t * (2.0 * ha * dx + nb * dy), t * (2.0 * hc * dy + nb * dx)], 1)


def test_abs_pair_matches_float64_within_4_ulps():
    t, dx, dy, ha, nb, hc, _op = _pairs(200000, 1)
    got = _abs_pair(t, dx, dy, ha, nb, hc).astype(np.float64)
    want = np.abs(_exact(t, dx, dy, ha, nb, hc))
    err = np.abs(got - want) / _ulp32(want)
    cancel = np.abs(2.0 * ha.astype(np.float64) * dx + nb.astype(np.float64) * dy) < 1e-3 * np.abs(nb.astype(np.float64) * dy)
    print(f"lg_abs_pair: max error {err.max():.2f} float32 ulps of the result over {len(t)} pairs ({int(cancel.sum())} with a 1000-fold "
          f"cancellation of the two x terms, {int((want[:, 0] == 0).sum())} exact zeros)")
    assert cancel.sum() > 5000 and (t == 0).sum() > 1000 and ((dx == 0) & (dy == 0)).sum() > 1000
    assert (got >= 0).all()
    assert (got[t == 0] == 0).all() and (got[(dx == 0) & (dy == 0)] == 0).all()      # exact zeros stay exact
    assert err.max() <= ULPS


def test_abs_pair_accumulates_in_order():
    """k pairs of one Gaussian: every term within 4 ulps and k - 1 additions of non-negative numbers, each half an ulp of a partial sum
    that is no larger than the total: (4 + k / 2) ulps of the total."""
    lib = ab.harness()
    r = np.random.default_rng(2)
    for k in (1, 2, 16, 64):
        t, dx, dy, ha, nb, hc, _op = _pairs(k, 100 + k)
        ha[:], nb[:], hc[:] = ha[0], nb[0], hc[0]
        out = np.zeros(2, np.float32)
        lib.h_abs_pair_sum(k, ab.ptr(t), ab.ptr(dx), ab.ptr(dy), float(ha[0]), float(nb[0]), float(hc[0]), ab.ptr(out))
        want = np.abs(_exact(t, dx, dy, ha, nb, hc)).sum(0)
        err = np.abs(out.astype(np.float64) - want) / _ulp32(want)
        print(f"k = {k}: {err.max():.2f} ulps")
        assert err.max() <= ULPS + 0.5 * k
    del r


def test_abs_rows_to_grad_matches_float64_within_4_ulps():
    lib = ab.harness()
    r = np.random.default_rng(3)
    n = 100000
    sx = np.exp(r.uniform(np.log(1e-12), np.log(1e6), n)).astype(np.float32)
    sy = np.exp(r.uniform(np.log(1e-12), np.log(1e6), n)).astype(np.float32)
    sx[::13] = 0.0
    op = r.uniform(1.0 / 255.0, 1.0, n).astype(np.float32)
    for W, H in ((33, 17), (1920, 1080), (1, 7)):
        out = np.full((n, 3), np.nan, np.float32)
        lib.h_abs_rows_to_grad(n, ab.ptr(sx), ab.ptr(sy), ab.ptr(op), W, H, ab.ptr(out))
        want = np.stack([0.5 * W * op.astype(np.float64) * sx, 0.5 * H * op.astype(np.float64) * sy], 1)
        err = np.abs(out[:, :2].astype(np.float64) - want) / _ulp32(want)
        print(f"lg_abs_rows_to_grad {W} x {H}: max error {err.max():.2f} ulps")
        assert err.max() <= ULPS
        assert (out[:, 2] == 0).all() and (out[::13, 0] == 0).all()


def test_single_pair_absgrad_is_no_smaller_than_the_signed_gradient():
    """Per pair, |t (2 ha dx + nb dy)| op against the magnitude of the same pair's lg_rows_to_grads output (what K7's moments and K9 make
    of it).  Against the float64 value of the signed gradient the margin is the 4 ulps of the result (plus one for the product with op).
    lg_rows_to_grads itself evaluates op (2 ha m0 + nb m1) with a plain multiply-add per term, so ITS rounding error is up to an ulp of
    each term, not of the cancelled sum: the float32-to-float32 comparison allows 4 ulps of the larger term for it."""
    lib = ab.harness()
    t, dx, dy, ha, nb, hc, op = _pairs(200000, 4)
    a = _abs_pair(t, dx, dy, ha, nb, hc).astype(np.float64) * op.astype(np.float64)[:, None]
    signed = np.zeros((len(t), 2), np.float32)
    lib.h_pair_signed(len(t), *(ab.ptr(x) for x in (t, dx, dy, ha, nb, hc, op, signed)))
    exact = np.abs(_exact(t, dx, dy, ha, nb, hc)) * op.astype(np.float64)[:, None]
    u = 2.0 ** -23
    assert (a >= exact * (1.0 - (ULPS + 1.0) * u)).all()
    t64, dx64, dy64, op64 = (x.astype(np.float64) for x in (t, dx, dy, op))
    terms = np.stack([np.maximum(np.abs(2.0 * ha * t64 * dx64), np.abs(nb * t64 * dy64)),
                      np.maximum(np.abs(2.0 * hc * t64 * dy64), np.abs(nb * t64 * dx64))], 1) * op64[:, None]
    slack = ULPS * u * (a + terms)
    worst = (np.abs(signed.astype(np.float64)) - a - slack).max()
    print(f"max of |signed| - abs - slack: {worst:.3e} (must be <= 0)")
    assert worst <= 0.0


# ---- surface -----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_export():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"LG_FLAG_ABSGRAD = 32768\b", src) and _lib.FLAG_ABSGRAD == 32768
    assert not re.search(r"= 4096\b", src)                                                   # 4096 stays retired
    m = re.search(r"^int lg_backward_abs\((.*?)\);", src, flags=re.S | re.M)
    chunked = re.search(r"^int lg_backward_chunked\((.*?)\);", src, flags=re.S | re.M)
    assert m and chunked
    norm = lambda s: [" ".join(p.split()) for p in s.split(",")]  # noqa: E731
    assert norm(m.group(1))[:-1] == norm(chunked.group(1)) and norm(m.group(1))[-1] == "float* dL_dmeans2D_abs"
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", src).group(1)) == 7 and _lib.ABI_VERSION == 7       # purely additive
    lib = _lib.load()
    assert lib.lg_abi_version() == 7
    assert "lg_backward_abs" in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), "lg_backward_abs")
    assert lib.lg_backward_abs.restype is C.c_int and len(lib.lg_backward_abs.argtypes) == len(lib.lg_backward_chunked.argtypes) + 1


P = 0x1000      # a non-null pointer that must never be dereferenced


def _call_abs(lib, flags=_lib.FLAG_ABSGRAD, abs_ptr=P, dcolor=P, R=100, N=10):
    view = _lib.lg_view(32, 32, 1.0, 1.0, P, 1.0, P, P, 0, P, 0, flags, 0)
    g = _lib.lg_gaussians(N, 0, P, None, P, P, P, P, None, None)
    return lib.lg_backward_abs(C.byref(view), C.byref(g), P, P, P, P, R, dcolor, P, P, None, P, P, P, P, None, None, P, None, 1,
                               _lib.CHUNK_FN(), None, abs_ptr)


@pytest.mark.parametrize("what, kw", [("LG_FLAG_ABSGRAD", dict(flags=0)), ("LG_FLAG_ABSGRAD", dict(flags=_lib.FLAG_FAST_EXP)),
                                      ("dL_dmeans2D_abs", dict(abs_ptr=None)), ("dL_dmeans2D_abs", dict(abs_ptr=None, N=0)),
                                      ("dL_dcolor", dict(dcolor=None)), ("num_rendered", dict(R=-1)), ("num_rendered", dict(R=1 << 30))])
def test_c_abi_refuses_bad_arguments_before_any_device_call(what, kw):
    """This process has no GPU: a call that reached the HIP runtime would come back as LG_ERR_DEVICE."""
    lib = _lib.load()
    assert _call_abs(lib, **kw) == _lib.LG_ERR_INVALID_ARGUMENT
    assert what.lower() in lib.lg_last_error().decode().lower(), lib.lg_last_error().decode()


def test_option_is_validated_and_off_by_default():
    assert rasterizer.resolve_options()["absgrad"] is False
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="absgrad"):
            rasterizer.set_option("absgrad", bad)
        with pytest.raises(ValueError, match="absgrad"):
            rasterizer.options(absgrad=bad)
        with pytest.raises(ValueError, match="absgrad"):
            rasterizer.resolve_options({"absgrad": bad})
    with rasterizer.options(absgrad=True):
        assert rasterizer.resolve_options()["absgrad"] is True and rasterizer.option_value("absgrad") is True
    assert rasterizer.resolve_options()["absgrad"] is False
    prev = rasterizer.set_option("absgrad", True)
    try:
        assert prev is False and rasterizer.resolve_options()["absgrad"] is True
    finally:
        rasterizer.set_option("absgrad", False)
    assert "absgrad" in rasterizer.set_option.__doc__ and "absgrad" in inspect.getdoc(__import__("lightgaussian_amd.gaussian_renderer", fromlist=["render"]).render)


class _Stats:
    def __init__(self, n, seed):
        gen = torch.Generator().manual_seed(seed)
        self.xyz_gradient_accum = torch.rand(n, 1, generator=gen)
        self.denom = torch.randint(0, 9, (n, 1), generator=gen).float()
        self.max_radii2D = torch.randint(0, 30, (n,), generator=gen).float()


def test_accumulate_stats_reads_absgrad_on_cpu_tensors():
    n = 300
    gen = torch.Generator().manual_seed(0)
    vp = torch.zeros(n, 3)
    vp.grad = torch.randn(n, 3, generator=gen)
    f = torch.rand(n, generator=gen) < 0.5
    radii = torch.randint(0, 60, (n,), generator=gen, dtype=torch.int32)
    with pytest.raises(ValueError, match="absgrad"):
        densify.accumulate_stats(_Stats(n, 1), vp, f, absgrad=True)
    # .absgrad is what is read: with .absgrad = |.grad| the result is the absgrad=False result, bit for bit ...
    vp.absgrad = vp.grad.abs()
    a, b = _Stats(n, 1), _Stats(n, 1)
    densify.accumulate_stats(a, vp, f, radii=radii, absgrad=True)
    densify.accumulate_stats(b, vp, f, radii=radii)
    for name in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # ... and with another .absgrad it is that tensor's norm, not .grad's
    vp.absgrad = 3.0 * vp.grad.abs()
    c, first = _Stats(n, 1), _Stats(n, 1)
    densify.accumulate_stats(c, vp, f, absgrad=True)
    want = first.xyz_gradient_accum + torch.where(f[:, None], torch.linalg.vector_norm(vp.absgrad[:, :2], dim=-1, keepdim=True), torch.zeros(n, 1))
    assert torch.equal(c.xyz_gradient_accum, want) and not torch.equal(c.xyz_gradient_accum, b.xyz_gradient_accum)
    assert torch.equal(c.max_radii2D, first.max_radii2D)                    # no radii: not touched
    assert list(inspect.signature(densify.accumulate_stats).parameters) == ["model", "viewspace_points", "update_filter", "radii", "absgrad"]
    assert inspect.signature(densify.accumulate_stats).parameters["absgrad"].default is False


def test_runner_parses_the_flag(tmp_path):
    script = tmp_path / "trainer.py"
    script.write_text("raise AssertionError('the script must not run')\n")
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--absgrad", str(tmp_path / "missing.py")])
    assert "does not exist" in str(e.value) and "unknown option" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--absgrads", str(script)])
    assert "unknown option" in str(e.value) and "--absgrad " in str(e.value)            # the usage text lists the flag
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--distributed", "--absgrad", str(script)])
    assert "--absgrad" in str(e.value) and "--distributed" in str(e.value)
    assert "--absgrad" in lg_run.__doc__
    assert rasterizer.resolve_options()["absgrad"] is False                             # nothing was set on the way to the refusals
    src = inspect.getsource(lg_run.main)
    assert src.index("hip_densify()") < src.index("absgrad_densify()") < src.index("patch_reference(")


def test_runner_rebinds_add_densification_stats(monkeypatch):
    """absgrad_densify() on a stand-in scene.gaussian_model: the method reads .absgrad, the option becomes the process default."""
    import sys
    import types
    mod = types.ModuleType("scene.gaussian_model")

    class GaussianModel:
        def add_densification_stats(self, viewspace_point_tensor, update_filter):
            raise AssertionError("the reference's method must have been replaced")

    mod.GaussianModel = GaussianModel
    pkg = types.ModuleType("scene")
    pkg.gaussian_model = mod
    monkeypatch.setitem(sys.modules, "scene", pkg)
    monkeypatch.setitem(sys.modules, "scene.gaussian_model", mod)
    try:
        report = lg_run.absgrad_densify()
        assert any(k.endswith("add_densification_stats") for k in report)
        assert rasterizer.resolve_options()["absgrad"] is True
        n = 50
        model = GaussianModel()
        st = _Stats(n, 2)
        model.xyz_gradient_accum, model.denom, model.max_radii2D = st.xyz_gradient_accum, st.denom, st.max_radii2D
        vp = torch.zeros(n, 3)
        vp.grad = torch.zeros(n, 3)
        f = torch.ones(n, dtype=torch.bool)
        with pytest.raises(ValueError, match="absgrad"):
            model.add_densification_stats(vp, f)
        vp.absgrad = torch.ones(n, 3)
        before = model.xyz_gradient_accum.clone()
        model.add_densification_stats(vp, f)
        assert torch.equal(model.xyz_gradient_accum, before + torch.linalg.vector_norm(vp.absgrad[:, :2], dim=-1, keepdim=True))
    finally:
        lg_run.unpatch_reference()
        rasterizer.set_option("absgrad", False)
    assert GaussianModel.add_densification_stats.__qualname__.startswith("test_runner_rebinds")
