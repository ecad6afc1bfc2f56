"""-m gpu: every row-changing feature in one sequence on one model -- prune.prune_points, densify.densify_and_prune, mcmc.grow,
mcmc.relocate, then a step of the re-keyed HipAdam -- next to a twin that takes backend="torch" on the device with the same mask,
noise and draws (lightgaussian_amd.model_rows under all of them).

After every stage, by the rules of tests/densify_common.py and tests/mcmc_common.py and no other: row counts, row order, every copied
row and every moment bit for bit; the children of split rows by densify_common.rule; the recomputed opacity and scaling rows by
mcmc_common.check_state, each model against the float64 twin of the state it had before the stage.  The tensors nothing ever
computes -- f_dc, f_rest, rotation and all moments -- are also the same bits in both models from the first stage to the last."""
import pytest
import torch

import densify_common as dc
import mcmc_common as mc
from lightgaussian_amd import _lib, densify, mcmc, model_rows, optim, prune

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 257                                       # one row past a 256-thread workgroup
COPIED = ("f_dc", "f_rest", "rotation")
PROFILED = ("densify_plan", "densify_rows", "mcmc_count", "mcmc_plan", "mcmc_rows")


class profiled:
    def __enter__(self):
        densify.set_profile(True)
        mcmc.set_profile(True)
        _lib.profile_reset()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        self.launches = {k: prof.get(k, (0.0, 0))[1] for k in PROFILED}
        densify.set_profile(False)
        mcmc.set_profile(False)


def state_case(model):
    """The model's present state in densify_common's layout (numpy copies), with its bookkeeping tensors."""
    c = {}
    for n in dc.NAMES:
        p = model.param(n)
        st = model.optimizer.state[p]
        c[f"in_{n}"], c[f"in_m_{n}"], c[f"in_v_{n}"] = (t.detach().cpu().numpy().copy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))
    c.update({name: getattr(model, name).cpu().numpy().copy() for name in model_rows.BOOK})
    return c


def assert_copied_tensors_agree(ours, theirs, label):
    for n in dc.NAMES:
        if n in COPIED:
            assert dc.same_bits(ours.param(n), theirs.param(n)), (label, n)
        for key in ("exp_avg", "exp_avg_sq"):
            assert dc.same_bits(ours.optimizer.state[ours.param(n)][key], theirs.optimizer.state[theirs.param(n)][key]), (label, n, key)


def top_sources(c, rows, n):
    """n source rows among `rows`, the most opaque first and twice: every source is drawn at most twice and sigma > 0.3 there, so the
    corrected opacities stay far above min_opacity in both backends."""
    sigma = torch.sigmoid(torch.from_numpy(c["in_opacity"])).reshape(-1)[rows]
    order = rows[torch.argsort(sigma, descending=True)]
    assert n <= order.numel() and float(sigma.max()) > 0.3 and float(torch.sort(sigma, descending=True).values[max(n - 2, 0)]) > 0.3
    return torch.cat([order[:1], order[:n - 1]])[:n]


@pytest.mark.parametrize("deg, scale, min_opacity", [(1, (0.004, 1.2), 0.001), (0, (0.004, 0.045), 0.005)], ids=["deg1-split-dead", "deg0-nosplit-nodead"])
def test_sequence_of_every_row_changing_feature(deg, scale, min_opacity):
    c = mc.case(N, deg=deg, seed=500 + deg, dead=0.15)
    c["in_scaling"] = dc.random_case(N, deg=deg, seed=500 + deg, scale=scale)["in_scaling"]
    c["kwargs"]["min_opacity"] = min_opacity                  # (0.001: rows with sigma in (0.001, 0.005] outlive densify, dead for relocate)
    ours, theirs = (dc.model_of(c, device=DEV, cls=optim.HipAdam) for _ in range(2))
    assert ours._features_rest.shape == (N, (deg + 1) ** 2 - 1, 3)
    gen = torch.Generator().manual_seed(77)

    # ---- 1. prune_points: both models, against boolean indexing of the state before ----
    mask = torch.rand(N, generator=gen) < 0.3
    keep = ~mask
    n = int(keep.sum())
    for model, label in ((ours, "ours"), (theirs, "twin")):
        before = state_case(model)
        old = [model.param(k) for k in dc.NAMES]
        named = prune.prune_points(model, mask.to(DEV))
        assert list(named) == list(dc.NAMES) and set(model.optimizer.state.keys()) == {g["params"][0] for g in model.optimizer.param_groups}
        for group, k, was in zip(model.optimizer.param_groups, dc.NAMES, old):
            p = group["params"][0]
            assert p is model.param(k) is named[k] and p is not was and p.requires_grad and p.is_leaf and p.shape[0] == n
            st = model.optimizer.state[p]
            assert dc.same_bits(p, torch.from_numpy(before[f"in_{k}"])[keep]), (label, k)
            assert dc.same_bits(st["exp_avg"], torch.from_numpy(before[f"in_m_{k}"])[keep]) and float(st["step"]) == 3.0
            assert dc.same_bits(st["exp_avg_sq"], torch.from_numpy(before[f"in_v_{k}"])[keep])
        for name in model_rows.BOOK:
            assert dc.same_bits(getattr(model, name), torch.from_numpy(before[name])[keep]), (label, name)
    assert_copied_tensors_agree(ours, theirs, "prune_points")

    # ---- 2. densify_and_prune: hip against torch with the same noise, by densify_common.check_against ----
    before = state_case(theirs)
    th = densify.thresholds(theirs, **c["kwargs"])
    keep_rows, clone_rows, split_rows, parents, rank = dc.contract_rows(theirs, th)
    n_s = split_rows.numel()
    noise = torch.randn(2 * n_s, 3, generator=gen).to(DEV)
    want = densify.densify_and_prune(theirs, noise=noise, backend="torch", **c["kwargs"])
    with profiled() as prof:
        got = densify.densify_and_prune(ours, noise=noise, backend="hip", **c["kwargs"])
    assert want["backend"] == "torch" and got["backend"] == "hip"
    counts = (want["N_out"], keep_rows.numel(), clone_rows.numel(), n_s, parents.numel())
    assert tuple(got[k] for k in ("N_out", "n_keep", "n_clone", "n_s", "n_child")) == counts == tuple(want[k] for k in ("N_out", "n_keep", "n_clone", "n_s", "n_child"))
    assert prof.launches == dict(densify_plan=1, densify_rows=1, mcmc_count=0, mcmc_plan=0, mcmc_rows=0), prof.launches
    if deg == 1:
        assert min(counts[1:]) > 0 and counts[3] > counts[4], counts     # every kind of row, and split parents whose children leave
    else:
        assert counts[3] == 0 and counts[2] > 0 and noise.shape == (0, 3), counts
    after = state_case(theirs)
    out = {}
    for k in dc.NAMES:
        out[k], out["m_" + k], out["v_" + k] = after[f"in_{k}"], after[f"in_m_{k}"], after[f"in_v_{k}"]
    r64 = dc.expected_r64(before, parents, rank, n_s, noise.cpu().numpy())
    dc.check_against(ours, out, counts, r64[0], r64[1], f"sequence deg {deg} densify", step=3)
    assert_copied_tensors_agree(ours, theirs, "densify_and_prune")
    assert dc.same_bits(ours._opacity, theirs._opacity)                  # (opacity is copied here; it is what the draws below are read from)

    # ---- 3. grow: each model against the twin of its own state, by mcmc_common.check_state ----
    n = counts[0]
    n_new = int(1.05 * n) - n
    assert n_new >= 2
    for model in (ours, theirs):                                        # bookkeeping with something in it, to be kept in front of the zero rows
        model.xyz_gradient_accum += torch.arange(1.0, n + 1.0, device=DEV)[:, None]
        model.denom += 2.0
        model.max_radii2D += torch.arange(n, 0.0, -1.0, device=DEV)
    src = top_sources(state_case(ours), torch.arange(n), n_new)
    dst = torch.arange(n, n + n_new)
    records = {}
    for model, backend in ((ours, "hip"), (theirs, "torch")):
        before = state_case(model)
        with profiled() as prof:
            records[backend] = mcmc.grow(model, cap_max=10 ** 6, draws=src.to(DEV), backend=backend)
        assert records[backend]["backend"] == backend and records[backend]["N_out"] == n + n_new
        if backend == "hip":
            assert prof.launches == dict(densify_plan=0, densify_rows=0, mcmc_count=1, mcmc_plan=1, mcmc_rows=1), prof.launches
        mc.check_state(model, mc.expected_state(before, dst, src, n + n_new, 0.005), dst, src, f"sequence deg {deg} {backend} grow", exact=backend == "hip")
        for name in model_rows.BOOK:
            t = getattr(model, name)
            assert t.shape[0] == n + n_new and dc.same_bits(t[:n], torch.from_numpy(before[name])) and not t[n:].any() and t[:n].all()
    assert {k: int(v) for k, v in records["hip"].items() if k != "backend"} == {k: int(v) for k, v in records["torch"].items() if k != "backend"}
    assert int(records["hip"]["n_sources"]) == torch.unique(src).numel() == n_new - 1
    assert_copied_tensors_agree(ours, theirs, "grow")

    # ---- 4. relocate: in place; with no dead row nothing is launched ----
    n = n + n_new
    case_now = state_case(ours)
    dead = mc.dead_rows(case_now)
    assert torch.equal(dead, mc.dead_rows(state_case(theirs)))
    dst, alive = torch.nonzero(dead).reshape(-1), torch.nonzero(~dead).reshape(-1)
    assert (dst.numel() >= 3) if deg == 1 else (dst.numel() == 0), dst.numel()
    src = top_sources(case_now, alive, dst.numel()) if dst.numel() else torch.zeros(0, dtype=torch.int64)
    records = {}
    for model, backend in ((ours, "hip"), (theirs, "torch")):
        before = state_case(model)
        params, keys = [model.param(k) for k in dc.NAMES], list(model.optimizer.state.keys())
        with profiled() as prof:
            records[backend] = mcmc.relocate(model, draws=src.to(DEV), backend=backend)
        assert records[backend]["backend"] == backend and records[backend]["n_dead"] == dst.numel()
        assert all(a is model.param(k) for a, k in zip(params, dc.NAMES)) and all(a is b for a, b in zip(model.optimizer.state.keys(), keys))
        if backend == "hip":
            busy = 1 if dst.numel() else 0
            assert prof.launches == dict(densify_plan=0, densify_rows=0, mcmc_count=busy, mcmc_plan=busy, mcmc_rows=busy), prof.launches
        mc.check_state(model, mc.expected_state(before, dst, src, n, 0.005), dst, src, f"sequence deg {deg} {backend} relocate", exact=backend == "hip")
    assert int(records["hip"]["n_sources"]) == int(records["torch"]["n_sources"]) == torch.unique(src).numel()
    assert_copied_tensors_agree(ours, theirs, "relocate")

    # ---- 5. the re-keyed optimizer steps: the same gradients, so rows that held the same bits before hold the same bits after ----
    equal_rows = {}
    for k, shape in dc.shapes(n, deg).items():
        grad = torch.randn(shape, generator=gen).to(DEV)
        a, b = ours.param(k), theirs.param(k)
        assert tuple(a.shape) == tuple(b.shape) == shape
        a.grad, b.grad = grad, grad.clone()
        equal_rows[k] = (dc.bits(a).flatten(1) == dc.bits(b).flatten(1)).all(dim=1)        # ([n, 0] rows: all of nothing, True)
    assert all(bool(equal_rows[k].all()) for k in COPIED) and int(equal_rows["xyz"].sum()) >= counts[1]
    was = {k: ours.param(k).detach().clone() for k in dc.NAMES}
    ours.optimizer.step()
    theirs.optimizer.step()
    assert isinstance(ours.optimizer, optim._HipStep)
    for k in dc.NAMES:
        a, b = ours.param(k), theirs.param(k)
        assert float(ours.optimizer.state[a]["step"]) == float(theirs.optimizer.state[b]["step"]) == 4.0
        assert a.numel() == 0 or not torch.equal(a.detach(), was[k]), k
        rows = equal_rows[k]
        assert dc.same_bits(a.detach().cpu()[rows], b.detach().cpu()[rows]), k
        assert bool(torch.isfinite(a).all())
    assert_copied_tensors_agree(ours, theirs, "step")
