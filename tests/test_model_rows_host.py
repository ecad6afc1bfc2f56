"""lightgaussian_amd.model_rows without a GPU: the optimizer walk (entries), the surgery (install) and the table builder (row_table)
under prune.prune_points, densify.densify_and_prune and mcmc.relocate / grow, on a CPU model of five rows built by
tests/densify_common.py / tests/mcmc_common.py with torch.optim.Adam.

prune.compact_tensors has no CPU path, so the two-parameters-in-one-group case exercises install directly with hand-compacted
tensors; prune_points itself runs in tests/test_gpu_model_rows.py and tests/test_gpu_compact.py."""
import warnings

import pytest
import torch

import densify_common as dc
import mcmc_common as mc
from lightgaussian_amd import _lib, densify, mcmc, model_rows, optim, prune

N = 5
DENSIFY_ARGS = dict(max_grad=0.0002, min_opacity=0.005, extent=5.0, max_screen_size=20)


def groups_of(model, extra=()):
    return [{"params": [model.param(n)] + list(extra if n == "xyz" else ()), "lr": dc.LRS[n], "name": n} for n in dc.NAMES]


def take_step(model):
    gen = torch.Generator().manual_seed(1)
    for group in model.optimizer.param_groups:
        for p in group["params"]:
            p.grad = torch.randn(p.shape, generator=gen)
    model.optimizer.step()


def fresh(steps=1, make=None, extra=()):
    """Five rows, no optimizer state but what `steps` real steps of the optimizer leave (torch.optim.Adam unless `make` builds another
    from the parameter groups); `extra` parameters join the xyz group."""
    c = mc.case(N, seed=3)
    model = dc.Model({n: c[f"in_{n}"] for n in dc.NAMES}, None, 0, c["percent_dense"], c["in_accum"], c["in_denom"], c["in_max_radii2D"], cls=torch.optim.Adam)
    if make is not None or extra:
        model.optimizer = (make or (lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15)))(groups_of(model, extra))
    for _ in range(steps):
        take_step(model)
    return model


def snapshot(model):
    """Everything the callers could touch: the objects and their bits."""
    params = [p for g in model.optimizer.param_groups for p in g["params"]]
    tensors = [p.detach().clone() for p in params] + [getattr(model, name).clone() for name in model_rows.BOOK]
    state = {p: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in model.optimizer.state[p].items()} for p in model.optimizer.state}
    return params, [model.param(n) for n in dc.NAMES], tensors, state


def assert_untouched(model, before):
    params, named, tensors, state = before
    now = snapshot(model)
    assert all(a is b for a, b in zip(now[0], params)) and len(now[0]) == len(params)
    assert all(a is b for a, b in zip(now[1], named))
    assert all(dc.same_bits(a, b) for a, b in zip(now[2], tensors))
    assert len(now[3]) == len(state) and all(a is b for a, b in zip(now[3], state))
    for p in state:
        assert now[3][p].keys() == state[p].keys()
        assert all(torch.equal(torch.as_tensor(now[3][p][k]), torch.as_tensor(state[p][k])) for k in state[p])


def row_changers():
    """(what, call) of every feature that goes through model_rows.entries."""
    return [("prune_points", lambda m: prune.prune_points(m, torch.tensor([True, False, False, True, False]))),
            ("densify_and_prune", lambda m: densify.densify_and_prune(m, backend="torch", **DENSIFY_ARGS)),
            ("grow", lambda m: mcmc.grow(m, cap_max=10 ** 6, factor=2.0, backend="torch")),
            ("relocate", lambda m: mcmc.relocate(m, backend="torch"))]


# ---- install ------------------------------------------------------------------------------------------------------------------------

def hand_compacted(entries, keep):
    return [tuple(t.detach()[keep].clone() for t in [p] + model_rows.moments(st)) + (None,) * (0 if st is not None else 2) for _, _, p, st in entries]


def test_install_moves_the_state_objects_to_the_new_keys():
    model = fresh(steps=1)
    opt = model.optimizer
    entries = model_rows.entries(model, "test")
    assert [(g["name"], j) for g, j, _, _ in entries] == [(n, 0) for n in dc.NAMES]
    assert all(st is opt.state[p] and float(st["step"]) == 1.0 for _, _, p, st in entries)
    keep = torch.tensor([0, 2, 4])
    new = hand_compacted(entries, keep)
    book = {name: getattr(model, name)[keep].clone() for name in model_rows.BOOK}
    named = model_rows.install(model, entries, new, book=book)
    assert list(named) == list(dc.NAMES) and len(opt.state) == len(dc.NAMES)
    for (group, j, old, st), (tensor, exp_avg, exp_avg_sq) in zip(entries, new):
        p = group["params"][j]
        assert p is model.param(group["name"]) and p is named[group["name"]] and p is not old
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.data_ptr() == tensor.data_ptr()
        assert old not in opt.state and opt.state[p] is st                       # the same dict object under the new key
        assert float(st["step"]) == 1.0 and st["exp_avg"] is exp_avg and st["exp_avg_sq"] is exp_avg_sq
        assert dc.same_bits(p, old[keep]) and tuple(st["exp_avg"].shape) == tuple(p.shape)
    assert all(getattr(model, name) is book[name] for name in model_rows.BOOK)
    dc.can_step(model)


def test_no_state_yet():
    model = fresh(steps=0)
    entries = model_rows.entries(model, "test")
    assert len(entries) == len(dc.NAMES) and all(st is None for _, _, _, st in entries)
    model.optimizer.state[model._xyz]                                            # (a defaultdict: looking leaves an empty state behind)
    assert model_rows.entries(model, "test")[0][3] is None
    del model.optimizer.state[model._xyz]
    keep = torch.tensor([1, 3])
    accum = model.xyz_gradient_accum
    named = model_rows.install(model, entries, hand_compacted(entries, keep))
    assert len(model.optimizer.state) == 0 and model.xyz_gradient_accum is accum  # no book: the bookkeeping attributes stay
    for group, n in zip(model.optimizer.param_groups, dc.NAMES):
        assert group["params"][0] is model.param(n) and named[n] is model.param(n) and model.param(n).shape[0] == 2
    take_step(model)
    assert all(float(model.optimizer.state[model.param(n)]["step"]) == 1.0 for n in dc.NAMES)


def test_every_caller_works_without_state():
    for what, call in row_changers()[1:]:                                        # (prune_points: compact_tensors needs the GPU)
        model = fresh(steps=0)
        call(model)
        assert len(model.optimizer.state) == 0, what
        assert all(g["params"][0] is model.param(g["name"]) for g in model.optimizer.param_groups), what


def test_two_parameters_in_one_group():
    extra = torch.nn.Parameter(torch.arange(2.0 * N).reshape(N, 2))
    model = fresh(steps=1, extra=[extra])
    opt = model.optimizer
    entries = model_rows.entries(model, "test")
    assert [(g["name"], j) for g, j, _, _ in entries[:3]] == [("xyz", 0), ("xyz", 1), ("f_dc", 0)] and entries[1][2] is extra
    assert len(entries) == len(dc.NAMES) + 1 and all(st is not None for _, _, _, st in entries)
    keep = torch.tensor([0, 2, 3])
    states = [st for _, _, _, st in entries]
    named = model_rows.install(model, entries, hand_compacted(entries, keep))
    first, second = opt.param_groups[0]["params"]
    assert first is model._xyz is named["xyz"] and second is not extra and len(named) == len(dc.NAMES)
    assert dc.same_bits(second, extra[keep]) and dc.same_bits(first, entries[0][2][keep])
    assert not any(second is v for v in vars(model).values())                    # only the first parameter of a group is bound to the model
    assert opt.state[first] is states[0] and opt.state[second] is states[1] and extra not in opt.state
    assert len(opt.state) == len(dc.NAMES) + 1 and states[1]["exp_avg"].shape == second.shape
    take_step(model)
    assert float(opt.state[second]["step"]) == 2.0


# ---- what entries refuses -----------------------------------------------------------------------------------------------------------

def test_state_without_moments_is_refused_by_every_caller():
    for what, call in row_changers():
        model = fresh(steps=1, make=lambda groups: torch.optim.SGD(groups, lr=1e-3, momentum=0.9))
        assert "momentum_buffer" in model.optimizer.state[model._xyz]
        before = snapshot(model)
        with pytest.raises(ValueError, match=rf"^{what}: the optimizer state of group 'xyz' .*exp_avg / exp_avg_sq"):
            call(model)
        assert_untouched(model, before)


def test_a_parameter_without_one_row_per_gaussian_is_refused_by_every_caller():
    for what, call in row_changers():
        model = fresh(steps=1)
        model.optimizer.add_param_group({"params": [torch.nn.Parameter(torch.zeros(N - 1, 3))], "lr": 1e-3, "name": "other"})
        before = snapshot(model)
        with pytest.raises(ValueError, match=rf"^{what}: every parameter of the optimizer must have one row per Gaussian$"):
            call(model)
        assert_untouched(model, before)


# ---- row_table ----------------------------------------------------------------------------------------------------------------------

def test_row_table_chunks_and_fields():
    assert _lib.DENSIFY_MAX_TENSORS == 32
    tensors = [(torch.zeros(N, k % 4 + 1), torch.zeros(N + 2, k % 4 + 1)) for k in range(33)]
    rows = [(None if k == 0 else a, b, k % 4 + 1, k % 5) for k, (a, b) in enumerate(tensors)]
    rows.insert(7, (torch.zeros(N, 0, 3), torch.zeros(N + 2, 0, 3), 0, 0))      # [N, 0, 3]: nothing to write, left out
    chunks = list(model_rows.row_table(rows))
    assert [count for count, _ in chunks] == [32, 1] and [len(table) for _, table in chunks] == [32, 1]
    got = [row for _, table in chunks for row in table]
    for k, (row, (a, b)) in enumerate(zip(got, tensors)):
        assert isinstance(row, _lib.lg_densify_tensor)
        assert row.src == (None if k == 0 else a.data_ptr()) and row.dst == b.data_ptr() and (row.row_words, row.role) == (k % 4 + 1, k % 5)
    assert list(model_rows.row_table([])) == [] and list(model_rows.row_table(rows[7:8])) == []


# ---- the small helpers --------------------------------------------------------------------------------------------------------------

def test_every_module_keeps_its_own_profile_switch():
    flags = {"densify": densify._flags, "mcmc": mcmc._flags, "optim": optim._profile_flag}
    modules = {"densify": densify, "mcmc": mcmc, "optim": optim}
    assert all(f() == 0 for f in flags.values())
    for name, module in modules.items():
        module.set_profile(True)
        try:
            assert {k: f() for k, f in flags.items()} == {k: (_lib.FLAG_PROFILE if k == name else 0) for k in flags}
        finally:
            module.set_profile(False)
    assert all(f() == 0 for f in flags.values())


def test_warn_once_is_per_model_module_entry_point_and_reason():
    a, b = fresh(steps=0), fresh(steps=0)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for model in (a, a, b):
            model_rows.warn_once(model, "densify", "densify_and_prune", "max_grad <= 0")
        model_rows.warn_once(a, "mcmc", "densify_and_prune", "max_grad <= 0")
        model_rows.warn_once(a, "densify", "accumulate_stats", "max_grad <= 0")
        model_rows.warn_once(a, "densify", "densify_and_prune", "N >= 2^30")
    texts = [str(w.message) for w in caught]
    assert len(texts) == 5 and texts[0] == "lightgaussian_amd.densify.densify_and_prune: max_grad <= 0 is outside the HIP path; taking the torch path"
    assert texts[2].startswith("lightgaussian_amd.mcmc.densify_and_prune: ")


def test_backend_names_and_scalar_rounding():
    for what in ("densify_and_prune", "relocate"):
        model_rows.check_backend("hip", what)
        model_rows.check_backend("torch", what)
        with pytest.raises(ValueError, match=rf"^{what}: unknown backend 'cuda' \(hip \| torch\)$"):
            model_rows.check_backend("cuda", what)
    assert model_rows.f32(0.1) == float(torch.tensor(0.1, dtype=torch.float32)) != 0.1
    assert not model_rows.plain_f32(torch.zeros(3)) and not model_rows.plain_f32(None) and not model_rows.plain_f32(torch.zeros(3), contiguous=True)
