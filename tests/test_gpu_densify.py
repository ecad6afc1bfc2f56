"""-m gpu: lg_densify_stats / lg_densify_plan / lg_densify_rows through lightgaussian_amd.densify.

backend="hip" against the reference's goldens (tests/golden/reference_densify.npz) and against backend="torch" on the device with
the same noise; row counts, row order, every copied row and every moment bit for bit, the computed child rows by the rule of
tests/densify_common.py with R64 from float64 CPU copies.  accumulate_stats against the reference's four statements."""
import warnings

import numpy as np
import pytest
import torch

import densify_common as dc
from lightgaussian_amd import _lib, densify, optim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def launches():
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    return {k: prof.get(k, (0.0, 0))[1] for k in ("densify_stats", "densify_plan", "densify_rows")}


# ---- 1. the goldens ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.CASES)
def test_hip_backend_reproduces_the_reference(name):
    c = dc.case(name)
    model = dc.model_of(c, device=DEV)
    densify.set_profile(True)
    _lib.profile_reset()
    try:
        rec = densify.densify_and_prune(model, noise=torch.from_numpy(c["noise"]).to(DEV), backend="hip", **c["kwargs"])
        n = launches()
    finally:
        densify.set_profile(False)
    assert rec == dict(zip(("N_out", "n_keep", "n_clone", "n_s", "n_child"), (int(v) for v in c["counts"][:5])), backend="hip")
    assert n["densify_plan"] == 1 and n["densify_rows"] == (1 if rec["N_out"] else 0), n
    dc.check_golden(model, c, name)
    dc.can_step(model)


# ---- 2. hip against torch on the device -------------------------------------------------------------------------------------------

def both_backends(c, noise=None):
    th = densify.thresholds(dc.model_of(c), **c["kwargs"])
    ours, theirs = dc.model_of(c, device=DEV), dc.model_of(c, device=DEV)
    keep_rows, clone_rows, split_rows, parents, rank = dc.contract_rows(theirs, th)
    n_s = split_rows.numel()
    if noise is None:
        noise = torch.randn(2 * n_s, 3, generator=torch.Generator().manual_seed(11)).to(DEV)
    want = densify.densify_and_prune(theirs, noise=noise, backend="torch", **c["kwargs"])
    got = densify.densify_and_prune(ours, noise=noise, backend="hip", **c["kwargs"])
    assert want["backend"] == "torch" and got["backend"] == "hip"
    counts = (want["N_out"], keep_rows.numel(), clone_rows.numel(), n_s, parents.numel())
    assert tuple(got[k] for k in ("N_out", "n_keep", "n_clone", "n_s", "n_child")) == counts == tuple(want[k] for k in ("N_out", "n_keep", "n_clone", "n_s", "n_child"))
    out = {}
    for n in dc.NAMES:
        p = theirs.param(n)
        st = theirs.optimizer.state[p]
        out[n], out["m_" + n], out["v_" + n] = p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
    r64 = dc.expected_r64(c, parents, rank, n_s, noise.cpu().numpy())
    return ours, out, counts, r64


# (1_049_601 = 1025 * 1024 + 1 rows are 1026 block words: the single-workgroup scan of lg_densify_plan takes its second, carry round)
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000, 1_049_601])
def test_hip_equals_torch_on_the_device(n):
    c = dc.random_case(n, deg=1, seed=100 + n)
    if n == 1:                                      # the one row is split: above the gradient threshold, larger than percent_dense * extent
        c["in_accum"][:], c["in_denom"][:] = 1.0, 1.0
        c["in_scaling"][:], c["in_opacity"][:] = np.log(0.2), 1.0
    ours, out, counts, r64 = both_backends(c)
    if n >= 1023:
        assert min(counts[1:]) > 0 and counts[3] > counts[4], counts      # every kind of row, and split parents whose children leave
    else:
        assert counts == (2, 0, 0, 1, 1)
    dc.check_against(ours, out, counts, r64[0], r64[1], f"N={n}", step=3)


def test_empty_results():
    # everything pruned: N_out = 0
    c = dc.random_case(700, seed=5)
    c["kwargs"]["min_opacity"] = 2.0
    ours, out, counts, r64 = both_backends(c)
    assert counts[0] == 0 and counts[3] > 0
    dc.check_against(ours, out, counts, r64[0], r64[1], "all pruned", step=3)
    # nothing split: n_s = 0 and the noise is empty
    c = dc.random_case(700, seed=6, scale=(0.004, 0.045))
    ours, out, counts, r64 = both_backends(c, noise=torch.zeros(0, 3, device=DEV))
    assert counts[3] == 0 and counts[2] > 0 and counts[0] > 0
    dc.check_against(ours, out, counts, r64[0], r64[1], "nothing split", step=3)
    # and with the default draw of an empty noise
    model = dc.model_of(c, device=DEV)
    assert densify.densify_and_prune(model, backend="hip", **c["kwargs"])["N_out"] == counts[0]


def test_seeded_default_noise_is_the_reference_stream():
    c = dc.random_case(1500, seed=8)
    th = densify.thresholds(dc.model_of(c), **c["kwargs"])
    probe = dc.model_of(c, device=DEV)
    n_s = dc.contract_rows(probe, th)[2].numel()
    assert n_s > 100
    stds = torch.rand(2 * n_s, 3, device=DEV) + 0.5
    torch.manual_seed(42)
    unit = torch.normal(mean=torch.zeros(2 * n_s, 3, device=DEV), std=torch.ones(2 * n_s, 3, device=DEV))
    torch.manual_seed(42)
    scaled = torch.normal(mean=torch.zeros(2 * n_s, 3, device=DEV), std=stds)          # the reference's draw
    state = torch.cuda.get_rng_state(DEV)
    assert torch.equal(scaled, unit * stds)
    a, b = dc.model_of(c, device=DEV), dc.model_of(c, device=DEV)
    torch.manual_seed(42)
    densify.densify_and_prune(a, backend="hip", **c["kwargs"])
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    densify.densify_and_prune(b, noise=unit, backend="hip", **c["kwargs"])
    for n in dc.NAMES:
        assert dc.same_bits(a.param(n), b.param(n)), n


def test_one_host_read_per_call():
    c = dc.case("mixed")
    model = dc.model_of(c, device=DEV)
    noise = torch.from_numpy(c["noise"]).to(DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.ones(1, device=DEV).item()                                          # control: this build reports a synchronisation
            control = len([w for w in caught if "synchroniz" in str(w.message).lower()])
            densify.densify_and_prune(model, noise=noise, backend="hip", **c["kwargs"])
            total = len([w for w in caught if "synchroniz" in str(w.message).lower()])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert control == 1, "torch.cuda.set_sync_debug_mode reports nothing on this build"
    assert total - control == 1, [str(w.message) for w in caught]


# ---- 3. view statistics -----------------------------------------------------------------------------------------------------------

class Stats:
    def __init__(self, n, gen):
        self.xyz_gradient_accum = (torch.rand(n, 1, generator=gen) * 1e-3).to(DEV)
        self.denom = torch.randint(0, 9, (n, 1), generator=gen).float().to(DEV)
        self.max_radii2D = (torch.randint(0, 30, (n,), generator=gen)).float().to(DEV)


def four_statements(model, grad, f, radii):
    """add_densification_stats (scene/gaussian_model.py:784-788) and the trainer's max_radii2D line (train_densify_prune.py:172-174)."""
    model.max_radii2D[f] = torch.max(model.max_radii2D[f], radii[f])
    model.xyz_gradient_accum[f] += torch.norm(grad[f, :2], dim=-1, keepdim=True)
    model.denom[f] += 1


@pytest.mark.parametrize("n, fill", [(1, None), (1025, None), (3000, True), (3000, False), (5000, None)])
def test_accumulate_stats(n, fill):
    gen = torch.Generator().manual_seed(n + (0 if fill is None else 1 + int(fill)))
    ours, theirs = Stats(n, torch.Generator().manual_seed(n)), Stats(n, torch.Generator().manual_seed(n))
    r64 = ours.xyz_gradient_accum.double().cpu().clone()
    views = 3
    densify.set_profile(True)
    _lib.profile_reset()
    try:
        for v in range(views):
            vp = torch.zeros(n, 3, device=DEV)
            vp.grad = (torch.randn(n, 3, generator=gen) * torch.exp(3.0 * torch.randn(n, 1, generator=gen)) * 1e-4).to(DEV)
            f = (torch.rand(n, generator=gen) < 0.5) if fill is None else torch.full((n,), fill)
            if n == 1:
                f[:] = v != 1
            f = f.to(DEV)
            radii = torch.randint(0, 60, (n,), generator=gen, dtype=torch.int32).to(DEV)
            version = ours.xyz_gradient_accum._version
            densify.accumulate_stats(ours, vp, f, radii=radii)
            assert ours.xyz_gradient_accum._version > version
            four_statements(theirs, vp.grad, f, radii)
            g = vp.grad.double().cpu()
            r64[f.cpu()] += torch.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)[f.cpu()][:, None]
        n_launch = launches()["densify_stats"]
    finally:
        densify.set_profile(False)
    assert n_launch == views
    assert dc.same_bits(ours.denom, theirs.denom) and dc.same_bits(ours.max_radii2D, theirs.max_radii2D)
    dc.rule(f"accum N={n}", ours.xyz_gradient_accum.cpu().numpy(), theirs.xyz_gradient_accum.cpu().numpy(), r64.numpy())
    if fill is False:
        first = Stats(n, torch.Generator().manual_seed(n))
        assert dc.same_bits(ours.xyz_gradient_accum, first.xyz_gradient_accum) and dc.same_bits(ours.max_radii2D, first.max_radii2D)
    # without radii, max_radii2D is not touched
    before = ours.max_radii2D.clone()
    vp = torch.zeros(n, 3, device=DEV)
    vp.grad = torch.ones(n, 3, device=DEV)
    densify.accumulate_stats(ours, vp, torch.ones(n, dtype=torch.bool, device=DEV))
    assert dc.same_bits(ours.max_radii2D, before)


def test_accumulate_stats_never_synchronises():
    n = 2000
    model = Stats(n, torch.Generator().manual_seed(1))
    vp = torch.zeros(n, 3, device=DEV)
    vp.grad = torch.randn(n, 3, device=DEV)
    f = torch.rand(n, device=DEV) < 0.5
    radii = torch.randint(0, 60, (n,), dtype=torch.int32, device=DEV)
    _lib.load()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                                          # control: the mode is live on this build
        densify.accumulate_stats(model, vp, f, radii=radii)
        densify.accumulate_stats(model, vp, f)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert float(model.denom.sum()) > 0


# ---- 4. the new model trains and renders ------------------------------------------------------------------------------------------

def test_new_model_steps_renders_and_densifies_again():
    from common import syn
    from lightgaussian_amd.gaussian_renderer import render
    c = dc.random_case(3000, deg=1, seed=21, scale=(0.004, 0.3))
    c["in_xyz"] = c["in_xyz"] * 1.5
    model = dc.model_of(c, device=DEV, cls=optim.HipAdamW)
    first = densify.densify_and_prune(model, backend="hip", **c["kwargs"])
    assert first["backend"] == "hip" and first["N_out"] > 3000 and first["n_child"] > 0 and first["n_clone"] > 0
    W = H = 64
    cam = syn.orbit_camera(0, 8, W, H).to(DEV)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)

    def view():
        return syn.SyntheticGaussians(model._xyz, model._features_dc, model._features_rest, model._scaling, model._rotation, model._opacity, 1, 1)

    pkg = render(cam, view(), syn.PipelineParams(), bg)
    image = pkg["render"]
    assert tuple(image.shape) == (3, H, W) and bool(torch.isfinite(image).all())
    image.mean().backward()
    assert all(model.param(n).grad is not None and model.param(n).grad.shape[0] == first["N_out"] for n in dc.NAMES)
    densify.accumulate_stats(model, pkg["viewspace_points"], pkg["visibility_filter"], radii=pkg["radii"])
    assert float(model.denom.sum()) == float(pkg["visibility_filter"].sum()) > 0
    before = model._xyz.detach().clone()
    model.optimizer.step()
    assert isinstance(model.optimizer, optim._HipStep) and not torch.equal(model._xyz.detach(), before)
    assert all(float(model.optimizer.state[model.param(n)]["step"]) == 4.0 for n in dc.NAMES)
    model.xyz_gradient_accum += 0.01
    second = densify.densify_and_prune(model, backend="hip", **c["kwargs"])
    assert second["backend"] == "hip" and second["N_out"] == model._xyz.shape[0] == model.optimizer.state[model._xyz]["exp_avg"].shape[0]
    assert bool(torch.isfinite(render(cam, view(), syn.PipelineParams(), bg)["render"]).all())
