"""-m gpu: lg_mcmc_noise / lg_mcmc_plan / lg_mcmc_rows through lightgaussian_amd.mcmc.

backend="hip" against the float64 twin of tests/mcmc_common.py and against backend="torch" on the device with the same noise and the
same draws: the noise by the project's tolerance rule, row order, every copied row and every moment bit for bit, the recomputed
opacity and scaling rows by the 2^-23 bound of tests/mcmc_common.py."""
import numpy as np
import pytest
import torch

import densify_common as dc
import mcmc_common as mc
import tolerance
from lightgaussian_amd import _lib, mcmc, optim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROFILED = ("mcmc_noise", "mcmc_count", "mcmc_plan", "mcmc_rows")


def launches():
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    return {k: prof.get(k, (0.0, 0))[1] for k in PROFILED}


class profiled:
    def __enter__(self):
        mcmc.set_profile(True)
        _lib.profile_reset()

    def __exit__(self, *exc):
        mcmc.set_profile(False)


# ---- 1. the position noise ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 5000])
def test_add_noise(n):
    c = mc.noise_case(n, seed=60 + n)
    xyz_lr, noise_lr = 1e-5, 5e5                                    # c = 5: steps of the size of the scene (xyz ~ N(0, 1), s up to 1.2)
    noise = torch.from_numpy(c["noise"]).to(DEV)
    ours, theirs, again = (dc.model_of(c, device=DEV) for _ in range(3))
    mcmc.load()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                          # control: the mode is live on this build
        with profiled():
            version = ours._xyz._version
            mcmc.add_noise(ours, xyz_lr, noise_lr=noise_lr, noise=noise, backend="hip")
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert launches() == dict(mcmc_noise=1, mcmc_count=0, mcmc_plan=0, mcmc_rows=0) and ours._xyz._version > version
    mcmc.add_noise(theirs, xyz_lr, noise_lr=noise_lr, noise=noise, backend="torch")
    mcmc.add_noise(again, xyz_lr, noise_lr=noise_lr, noise=noise, backend="hip")
    assert dc.same_bits(ours._xyz, again._xyz)
    for name in dc.NAMES[1:]:
        assert dc.same_bits(ours.param(name), torch.from_numpy(c[f"in_{name}"])), name
    got, r32 = ours._xyz.detach().cpu().numpy(), theirs._xyz.detach().cpu().numpy()
    cc = float(np.float32(noise_lr * xyz_lr))
    r64 = mc.noise_r64(c["in_xyz"], c["in_scaling"], c["in_rotation"], c["in_opacity"], c["noise"], cc, 100.0, 0.995)
    tolerance.assert_rule3(got, r64, r32, f"add_noise N={n} xyz", ref="torch backend")
    tolerance.assert_elementwise(got, r64, r32, f"add_noise N={n} xyz", ref="torch backend")
    x_in = c["in_xyz"].astype(np.float64)
    tolerance.assert_rule3(got - x_in, r64 - x_in, r32 - x_in, f"add_noise N={n} step", ref="torch backend", nonzero=n > 1)
    # exp(-k ((1 - sigma) - x0)) overflows float32 above 88.73: those rows keep their bits
    sigma = 1.0 / (1.0 + np.exp(-c["in_opacity"].astype(np.float64).reshape(-1)))
    arg = -100.0 * ((1.0 - sigma) - float(np.float32(0.995)))
    still, moving = arg > 89.0, arg < 88.0                        # (every eighth row sits at 89.5)
    if n >= 63:
        assert still.any() and moving.any() and np.abs(r64 - x_in).max() > 0.5
    assert torch.equal(ours._xyz.detach().cpu()[torch.from_numpy(still)], torch.from_numpy(c["in_xyz"])[torch.from_numpy(still)])
    assert not np.array_equal(got[moving], c["in_xyz"][moving]) or not moving.any()


# ---- 2. the row movement ------------------------------------------------------------------------------------------------------------

def moved_pair(c, what, dst, src, cls=torch.optim.AdamW, **kw):
    """hip and torch on the device with the same draws; returns (hip model, torch model, hip's launches)."""
    ours, theirs = dc.model_of(c, device=DEV, cls=cls), dc.model_of(c, device=DEV, cls=cls)
    call = getattr(mcmc, what)
    with profiled():
        got = call(ours, draws=src.to(DEV), backend="hip", **kw)
        n_launch = launches()
    want = call(theirs, draws=src.to(DEV), backend="torch", **kw)
    assert got["backend"] == "hip" and want["backend"] == "torch"
    assert {k: int(v) for k, v in got.items() if k != "backend"} == {k: int(v) for k, v in want.items() if k != "backend"}
    assert int(got["n_sources"]) == torch.unique(src).numel()
    for name in dc.NAMES:
        if name not in ("opacity", "scaling"):
            assert dc.same_bits(ours.param(name), theirs.param(name)), name
        for key in ("exp_avg", "exp_avg_sq"):
            assert dc.same_bits(ours.optimizer.state[ours.param(name)][key], theirs.optimizer.state[theirs.param(name)][key]), (name, key)
    return ours, theirs, n_launch


@pytest.mark.parametrize("n, deg", [(257, 1), (1024, 1), (5000, 1), (5000, 0)])
def test_relocate(n, deg):
    c = mc.case(n, deg=deg, seed=200 + n + deg, dead=0.07 if n == 5000 else 0.05)
    dead = mc.dead_rows(c)
    dst, alive = torch.nonzero(dead).reshape(-1), torch.nonzero(~dead).reshape(-1)
    src = mc.hand_draws(alive[:: max(1, alive.numel() // 40)], dst.numel())
    assert dst.numel() >= 5 and (n < 5000 or int(torch.bincount(src).max()) == 200)
    probe = dc.model_of(c, device=DEV)
    params = [probe.param(k) for k in dc.NAMES]
    keys = list(probe.optimizer.state.keys())
    mcmc.relocate(probe, draws=src.to(DEV), backend="hip")
    assert all(a is probe.param(k) for a, k in zip(params, dc.NAMES)) and list(probe.optimizer.state.keys()) == keys
    ours, theirs, n_launch = moved_pair(c, "relocate", dst, src)
    assert n_launch == dict(mcmc_noise=0, mcmc_count=1, mcmc_plan=1, mcmc_rows=1), n_launch
    exp = mc.expected_state(c, dst, src, n, 0.005)
    mc.check_state(ours, exp, dst, src, f"hip relocate N={n} deg {deg}", exact=True)
    mc.check_state(theirs, exp, dst, src, f"torch relocate N={n} deg {deg}", exact=False)
    assert all(dc.same_bits(ours.param(k), probe.param(k)) for k in dc.NAMES)                  # a second run: the same bits
    dc.can_step(ours)
    dc.can_step(moved_pair(c, "relocate", dst, src, cls=optim.HipAdam)[0])


@pytest.mark.parametrize("n, deg, factor", [(1, 1, 2.0), (257, 1, 1.05), (1024, 1, 1.05), (5000, 1, 1.07), (5000, 0, 1.07)])
def test_grow(n, deg, factor):
    c = mc.case(n, deg=deg, seed=300 + n + deg)
    n_new = int(factor * n) - n
    src = mc.hand_draws(range(0, n, max(1, n // 40)), n_new)
    assert n_new >= 1 and (n < 5000 or int(torch.bincount(src).max()) == 200)
    dst = torch.arange(n, n + n_new)
    ours, theirs, n_launch = moved_pair(c, "grow", dst, src, cap_max=10 ** 6, factor=factor)
    assert n_launch == dict(mcmc_noise=0, mcmc_count=1, mcmc_plan=1, mcmc_rows=1), n_launch
    exp = mc.expected_state(c, dst, src, n + n_new, 0.005)
    mc.check_state(ours, exp, dst, src, f"hip grow N={n} deg {deg}", exact=True)
    mc.check_state(theirs, exp, dst, src, f"torch grow N={n} deg {deg}", exact=False)
    for name, old in (("xyz_gradient_accum", c["in_accum"]), ("denom", c["in_denom"]), ("max_radii2D", c["in_max_radii2D"])):
        t = getattr(ours, name)
        assert t.shape[0] == n + n_new and dc.same_bits(t[:n], torch.from_numpy(np.asarray(old, np.float32))) and not t[n:].any()
    again = moved_pair(c, "grow", dst, src, cls=optim.HipAdam, cap_max=10 ** 6, factor=factor)[0]
    assert all(dc.same_bits(ours.param(k), again.param(k)) for k in dc.NAMES)                  # a second run: the same bits
    dc.can_step(ours)
    dc.can_step(again)


def test_relocate_makes_one_host_read_and_default_draws_keep_the_stream():
    import warnings
    c = mc.case(3000, seed=11)
    a, b = dc.model_of(c, device=DEV), dc.model_of(c, device=DEV)
    dead = mc.dead_rows(c).to(DEV)
    alive = torch.nonzero(~dead).reshape(-1)
    torch.manual_seed(4)
    draws = alive[torch.multinomial(torch.sigmoid(a._opacity.detach()).reshape(-1)[alive], int(dead.sum()), replacement=True)]
    state = torch.cuda.get_rng_state(DEV)
    torch.manual_seed(4)
    mcmc.load()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            mcmc.relocate(a, backend="hip")
            total = len([w for w in caught if "synchroniz" in str(w.message).lower()])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert total == 1, [str(w.message) for w in caught]
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    mcmc.relocate(b, draws=draws, backend="hip")
    assert all(dc.same_bits(a.param(k), b.param(k)) for k in dc.NAMES)


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------

def test_training_to_a_budget():
    from common import syn
    from lightgaussian_amd.gaussian_renderer import render
    c = mc.case(200, deg=1, seed=21)
    c["in_scaling"] = c["in_scaling"] - 1.5
    c["in_xyz"] = c["in_xyz"] * 1.5
    model = dc.model_of(c, device=DEV, cls=optim.HipAdam)
    W = H = 64
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    sizes = []
    for it in range(1, 31):
        cam = syn.orbit_camera(it % 8, 8, W, H).to(DEV)
        view = syn.SyntheticGaussians(model._xyz, model._features_dc, model._features_rest, model._scaling, model._rotation, model._opacity, 1, 1)
        image = render(cam, view, syn.PipelineParams(), bg)["render"]
        loss = (image - target).abs().mean() + mcmc.regularizers(model)
        model.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        model.optimizer.step()
        done = mcmc.after_step(model, it, dc.LRS["xyz"], 300, start=0, stop=1000, every=10, factor=1.25)
        assert (done["grow"] is not None) == (it % 10 == 0) and (done["grow"] is None or done["grow"]["backend"] == "hip")
        sizes.append(model._xyz.shape[0])
    assert sizes[-1] == 300 and sizes[9] == 250 and sizes[0] == 200, sizes
    assert isinstance(model.optimizer, optim._HipStep)
    for name in dc.NAMES:
        p = model.param(name)
        assert p.shape[0] == 300 and bool(torch.isfinite(p).all()), name
        assert model.optimizer.state[p]["exp_avg"].shape[0] == 300
