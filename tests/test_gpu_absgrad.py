"""-m gpu: absolute screen-space mean gradients (option "absgrad", LG_FLAG_ABSGRAD, lg_backward_abs): K7's ABS variants leave
sum_pixels |dL/dmean2D| terms in floats 9 and 10 of the gradient rows, lg_absgrad_rows sums them per Gaussian, and the backward sets
means2D.absgrad.

Reference, rule and scenes: tests/absgrad_common.py (the dense twin, one autograd.grad per pixel; rel_err(got, d64) <= max(1e-4,
3 rel_err(d32, d64)) in the max norm; scenes a-d)."""
import warnings

import numpy as np
import pytest
import torch

import absgrad_common as ab
import camera_grad_common as cg
import densify_common as dc
from common import bits as _bits
from lightgaussian_amd import densify, rasterizer

pytestmark = pytest.mark.gpu
DEV = ab.DEV
ON = {"absgrad": True}


def _run(path, name, options, **kw):
    return (ab.run_activated if path == "activated" else ab.run_render)(name, options, **kw)


def _absgrad(out):
    a = out["means2D"].absgrad
    assert a.dtype == torch.float32 and tuple(a.shape) == tuple(out["means2D"].shape) and a.device == out["means2D"].device
    return a.cpu().numpy()


def _scene_reaches_its_path(name, out):
    """What each scene is there for, read off the run itself."""
    radii = out["radii"].cpu().numpy()
    if name == "b":
        assert radii[-2] == 0 and radii[-1] == 0 and len(radii) % 64 != 0           # behind the camera, off screen
    if name == "c":
        assert (radii > 0).sum() >= 129                                               # one tile: a list of >= 3 segments of 64
    if name == "d":
        assert radii[-1] >= 112                                                       # its rectangle is the whole 7 x 7 grid: 49 rows > 48


# ---- 1. against the dense twin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["activated", "raw"])
@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("name", ab.SCENES)
def test_absgrad_against_the_dense_twin(name, fast_exp, path):
    ref = ab.abs_reference(name)
    out = _run(path, name, dict(ON, fast_exp=fast_exp))
    _scene_reaches_its_path(name, out)
    ab.assert_rule(_absgrad(out), ref, f"{name} {path} fast_exp={fast_exp}")
    # (the twin's own sanity, printed: its signed sum is the gradient the rasterizer has always returned)
    g = out["grads"]["means2D"].cpu().numpy()[:, :2]
    print(f"{name} {path} fast_exp={fast_exp} signed d/dmeans2D: rel_err {ab.rel_err(g, ref['float64']['grad']):.3e}")


@pytest.mark.parametrize("path", ["activated", "raw"])
@pytest.mark.parametrize("fast_exp", [True, False])
def test_absgrad_with_antialiasing_against_the_dense_twin(fast_exp, path):
    """The record's opacity is the compensated one: lg_absgrad_rows multiplies by what the blend kernels used."""
    ref = ab.abs_reference("a", antialias=True)
    plain = ab.abs_reference("a")
    assert ab.rel_err(plain["float64"]["absgrad"], ref["float64"]["absgrad"]) > 1e-2          # the compensation matters here
    out = _run(path, "a", dict(ON, fast_exp=fast_exp, antialiasing=True))
    ab.assert_rule(_absgrad(out), ref, f"a antialiased {path} fast_exp={fast_exp}")


# ---- 2. everything else keeps its bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["activated", "raw"])
@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("name", ["a", "c"])
def test_every_other_output_is_bit_identical_to_the_option_off(name, fast_exp, path):
    off, on = _run(path, name, {"fast_exp": fast_exp}), _run(path, name, dict(ON, fast_exp=fast_exp))
    assert np.array_equal(_bits(on["image"]), _bits(off["image"])) and torch.equal(on["radii"], off["radii"])
    assert set(on["grads"]) == set(off["grads"]) and "means2D" in on["grads"]
    for n, g in off["grads"].items():
        assert g is not None and g.abs().max() > 0, n
        assert np.array_equal(_bits(on["grads"][n]), _bits(g)), n


@pytest.mark.parametrize("name", ["a", "c"])
def test_camera_gradients_are_bit_identical_with_the_option_on(name):
    """lg_backward_camera after lg_backward_abs on the same scratch: it reads floats 0..8 of the rows only."""
    off, on = ab.run_activated(name, {}, camera_grad=True), ab.run_activated(name, ON, camera_grad=True)
    for n in cg.NAMES:
        assert np.abs(off["camera"][n]).max() > 0, n
        assert np.array_equal(_bits(on["camera"][n]), _bits(off["camera"][n])), n
    for n, g in off["grads"].items():
        assert np.array_equal(_bits(on["grads"][n]), _bits(g)), n
    plain = ab.run_activated(name, ON)
    assert np.array_equal(_bits(_absgrad(on)), _bits(_absgrad(plain)))


# ---- 3. absgrad >= |grad| ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["activated", "raw"])
@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("name", ab.SCENES)
def test_absgrad_dominates_the_signed_gradient(name, fast_exp, path):
    out = _run(path, name, dict(ON, fast_exp=fast_exp))
    a, g = _absgrad(out).astype(np.float64), out["grads"]["means2D"].cpu().numpy().astype(np.float64)
    radii = out["radii"].cpu().numpy()
    slack = a[:, :2] - (np.abs(g[:, :2]) * (1.0 - 1e-5) - 1e-12 * np.abs(a).max())
    print(f"{name} {path} fast_exp={fast_exp}: min slack {slack.min():.3e}, sum absgrad / sum |grad| = {a.sum() / np.abs(g).sum():.3f}")
    assert np.isfinite(a).all() and (a >= 0).all()
    assert (slack >= 0).all()
    assert not a[:, 2].any()
    assert not a[radii <= 0].any()                                                   # every row: no case is excluded above
    assert a[radii > 0].any() and a.sum() > 1.05 * np.abs(g[:, :2]).sum()          # and it is not merely |grad|: the pulls do cancel


# ---- 4, 5, 7: determinism, overwrite, absence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["activated", "raw"])
@pytest.mark.parametrize("name", ["b", "d"])
def test_two_runs_give_the_same_bits(name, path):
    one, two = _run(path, name, ON), _run(path, name, ON)
    assert _absgrad(one).any()
    assert np.array_equal(_bits(_absgrad(one)), _bits(_absgrad(two)))


def test_a_second_backward_overwrites_absgrad():
    once, twice = ab.run_activated("a", ON), ab.run_activated("a", ON, backwards=2)
    assert np.array_equal(_bits(_absgrad(twice)), _bits(_absgrad(once)))                            # not doubled ...
    assert np.array_equal(_bits(twice["grads"]["means2D"]), _bits(2.0 * once["grads"]["means2D"]))  # ... while .grad accumulates


@pytest.mark.parametrize("path", ["activated", "raw"])
def test_without_the_option_there_is_no_attribute(path):
    for options in ({}, {"absgrad": False}):
        assert not hasattr(_run(path, "a", options)["means2D"], "absgrad")
    assert rasterizer.resolve_options()["absgrad"] is False


# ---- with the hooks of the data-parallel step -----------------------------------------------------------------------------------------
def test_gradient_chunk_hook_and_sh_grad_sink():
    base = ab.run_activated("b", ON)
    seen = []
    rasterizer.set_grad_chunk_hook(lambda first, count, grads: seen.append((first, count, sorted(grads))), chunks=3)
    try:
        hooked = ab.run_activated("b", ON)
    finally:
        rasterizer.set_grad_chunk_hook(None)
    assert len(seen) == 3 and seen[0][0] == 0 and sum(c for _f, c, _n in seen) == base["means2D"].shape[0]
    assert np.array_equal(_bits(_absgrad(hooked)), _bits(_absgrad(base)))
    for n, g in base["grads"].items():
        assert np.array_equal(_bits(hooked["grads"][n]), _bits(g)), n

    class Sink:
        def __init__(self):
            self.calls = []

        def add(self, drgb, campos, sh_degree):
            self.calls.append((drgb.clone(), int(sh_degree)))

    sink = Sink()
    with rasterizer.options(sh_grad_sink=sink):
        sunk = ab.run_activated("b", ON)
    assert len(sink.calls) == 1 and sunk["grads"]["shs"] is None
    assert np.array_equal(_bits(_absgrad(sunk)), _bits(_absgrad(base)))
    assert np.array_equal(_bits(sunk["grads"]["means3D"]), _bits(base["grads"]["means3D"]))


# ---- 6. densification statistics through render() ----------------------------------------------------------------------------------------
def test_accumulate_stats_through_render():
    """accumulate_stats(..., absgrad=True) on the package of render(): denom and max_radii2D bit for bit; xyz_gradient_accum bit for bit
    against accum += sqrt(fma(ay, ay, ax ax)) over the filter -- lg_densify_stats' documented arithmetic, evaluated in torch in float64
    (the product and the sum of two float32 squares are exact there, the square root rounds once more, innocuously) -- and by the rule of
    the existing statistics test (tests/densify_common.py) against torch.norm in float32 and float64."""
    gen = torch.Generator().manual_seed(3)
    model = ab.gpu_model("b")
    n = model._xyz.shape[0]
    model.xyz_gradient_accum = torch.rand(n, 1, generator=gen).to(DEV)
    model.denom = torch.randint(0, 9, (n, 1), generator=gen).float().to(DEV)
    model.max_radii2D = torch.randint(0, 30, (n,), generator=gen).float().to(DEV)
    accum0, denom0, mr0 = model.xyz_gradient_accum.clone(), model.denom.clone(), model.max_radii2D.clone()
    out = ab.run_render("b", ON, model=model)
    pkg = out["pkg"]
    a, f, radii = pkg["viewspace_points"].absgrad, pkg["visibility_filter"].clone(), pkg["radii"]
    assert f.any() and not f.all()
    with pytest.raises(ValueError, match="absgrad"):
        densify.accumulate_stats(model, torch.zeros(n, 3, device=DEV), f, absgrad=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # (the torch fallback of an ineligible call warns: this is the lg_densify_stats launch)
        densify.accumulate_stats(model, pkg["viewspace_points"], f, radii=radii, absgrad=True)
    torch.cuda.synchronize()
    a64 = a.double()
    length = torch.sqrt((a64[:, 1] * a64[:, 1] + (a64[:, 0] * a64[:, 0]).float().double()).float().double()).float()[:, None]
    want = torch.where(f[:, None], accum0 + length, accum0)
    assert dc.same_bits(model.xyz_gradient_accum, want)
    assert dc.same_bits(model.denom, denom0 + f[:, None].float())
    assert dc.same_bits(model.max_radii2D, torch.where(f, torch.maximum(mr0, radii.float()), mr0))
    theirs, r64 = accum0.clone(), accum0.double().cpu().clone()
    theirs[f] += torch.norm(a[f, :2], dim=-1, keepdim=True)
    r64[f.cpu()] += torch.sqrt(a64[:, 0] ** 2 + a64[:, 1] ** 2).cpu()[f.cpu()][:, None]
    dc.rule("accum from absgrad", model.xyz_gradient_accum.cpu().numpy(), theirs.cpu().numpy(), r64.numpy())
    # and it is the absolute gradients that were read, not .grad
    other = accum0.clone()
    other[f] += torch.norm(pkg["viewspace_points"].grad[f, :2], dim=-1, keepdim=True)
    assert not torch.equal(other, model.xyz_gradient_accum)
