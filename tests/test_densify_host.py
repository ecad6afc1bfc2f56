"""Densification without a GPU: lightgaussian_amd.densify's torch backend against the goldens the reference's own densify_and_prune
produced (tests/golden/make_golden_densify.py), the lg_math.h child formulas through the CPU harness, the four C entry points and
their argument checks, and the run.py hook.  The comparison rules are in tests/densify_common.py."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import torch

import common
import densify_common as dc
import dropin_common
from lightgaussian_amd import _lib, densify, run as lg_run

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")


# ---- backend="torch" against the reference's own output ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.CASES)
def test_torch_backend_reproduces_the_reference(name):
    c = dc.case(name)
    model = dc.model_of(c)
    old = [model.param(n) for n in dc.NAMES]
    rec = densify.densify_and_prune(model, noise=torch.from_numpy(c["noise"]), backend="torch", **c["kwargs"])
    assert rec == dict(zip(("N_out", "n_keep", "n_clone", "n_s", "n_child"), (int(v) for v in c["counts"][:5])), backend="torch")
    dc.check_golden(model, c, name)
    assert all(p not in model.optimizer.state for p in old)
    dc.can_step(model)


def test_exact_tie_row_is_selected():
    c = dc.case("tie")
    row = int(c["counts"][6])
    g = c["in_accum"][row, 0] / c["in_denom"][row, 0]
    assert np.float32(g) == np.float32(c["kwargs"]["max_grad"])
    model = dc.model_of(c)
    raw = model._xyz.detach()[row].clone()
    densify.densify_and_prune(model, noise=torch.from_numpy(c["noise"]), backend="torch", **c["kwargs"])
    n_keep, n_clone = int(c["counts"][1]), int(c["counts"][2])
    kept = model._xyz.detach()[:n_keep + n_clone]
    hits = int((kept == raw).all(dim=1).sum())
    th = densify.thresholds(dc.model_of(c), **c["kwargs"])
    m, sigma = float(np.exp(c["in_scaling"][row]).max()), 1.0 / (1.0 + np.exp(-float(c["in_opacity"][row, 0])))
    cloned = m <= th["thr_d"] and not (sigma < th["min_opacity"] or m > th["thr_w"])
    # selected: cloned (the original and its copy are both there) or split / pruned (the original has left) -- never one unselected copy
    assert hits == (2 if cloned else 0)


def test_default_noise_is_the_reference_draw():
    """With the generator seeded, the default draw equals torch.normal(zeros, std) / std's stream: same values, same state afterwards."""
    c = dc.case("mixed")
    n_s = int(c["counts"][3])
    torch.manual_seed(31)
    expect = torch.normal(mean=torch.zeros(2 * n_s, 3), std=torch.ones(2 * n_s, 3))
    state = torch.get_rng_state()
    a, b = dc.model_of(c), dc.model_of(c)
    torch.manual_seed(31)
    densify.densify_and_prune(a, backend="torch", **c["kwargs"])
    assert torch.equal(torch.get_rng_state(), state)
    densify.densify_and_prune(b, noise=expect, backend="torch", **c["kwargs"])
    for n in dc.NAMES:
        assert dc.same_bits(a.param(n), b.param(n)), n
    # the reference's own draw, torch.normal(mean=zeros, std=stds), is this stream scaled by its stds
    stds = torch.rand(2 * n_s, 3, generator=torch.Generator().manual_seed(2)) + 0.5
    torch.manual_seed(31)
    scaled = torch.normal(mean=torch.zeros(2 * n_s, 3), std=stds)
    assert torch.equal(scaled, expect * stds) and torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="noise"):
        densify.densify_and_prune(dc.model_of(c), noise=torch.zeros(3, 3), backend="torch", **c["kwargs"])
    with pytest.raises(ValueError, match="backend"):
        densify.densify_and_prune(dc.model_of(c), backend="cuda", **c["kwargs"])


def test_hip_backend_on_cpu_parameters_falls_back_with_one_warning():
    c = dc.case("no_screen")
    model = dc.model_of(c)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        rec = densify.densify_and_prune(model, noise=torch.from_numpy(c["noise"]), backend="hip", **c["kwargs"])
        model.xyz_gradient_accum += 1.0
        model.denom += 1.0
        densify.densify_and_prune(model, backend="hip", **c["kwargs"])
    ours = [w for w in caught if "densify_and_prune" in str(w.message)]
    assert rec["backend"] == "torch" and len(ours) == 1 and "float32 on the GPU" in str(ours[0].message)
    model = dc.model_of(c)
    with pytest.warns(UserWarning, match="max_grad <= 0"):
        densify.densify_and_prune(model, backend="hip", **dict(c["kwargs"], max_grad=0.0))


def test_thresholds_are_rounded_once():
    model = dc.model_of(dc.case("deg0"))
    model.percent_dense = 0.01
    th = densify.thresholds(model, 0.0002, 0.005, np.float32(4.8), None)
    f32 = lambda v: float(np.float32(v))      # noqa: E731  (not common.f32: a Python float rounded to float32)
    assert th == dict(thr_g=f32(0.0002), thr_d=f32(0.01 * float(np.float32(4.8))), thr_w=f32(0.1 * float(np.float32(4.8))), min_opacity=f32(0.005),
                      use_extent=False)
    assert densify.thresholds(model, 0.0002, 0.005, 4.8, 20)["use_extent"] is True
    assert densify.thresholds(model, 0.0002, 0.005, 4.8, 0)["use_extent"] is False


# ---- accumulate_stats, torch path -------------------------------------------------------------------------------------------------

def test_accumulate_stats_reproduces_add_densification_stats():
    z = dc.golden()
    grads, filters = torch.from_numpy(z["stats/grad"]), torch.from_numpy(z["stats/filter"])
    n = grads.shape[1]
    model = dc.model_of(dc.case("mixed"))
    model.xyz_gradient_accum, model.denom, model.max_radii2D = torch.zeros(n, 1), torch.zeros(n, 1), torch.zeros(n)
    radii_ref = torch.zeros(n)
    gen = torch.Generator().manual_seed(3)
    for g, f in zip(grads, filters):
        vp = torch.zeros(n, 3)
        vp.grad = g
        radii = torch.randint(0, 50, (n,), generator=gen, dtype=torch.int32)
        densify.accumulate_stats(model, vp, f, radii=radii)
        radii_ref[f] = torch.max(radii_ref[f], radii[f])
    assert dc.same_bits(model.xyz_gradient_accum, torch.from_numpy(z["stats/accum"]))
    assert dc.same_bits(model.denom, torch.from_numpy(z["stats/denom"]))
    assert dc.same_bits(model.max_radii2D, radii_ref)
    with pytest.raises(ValueError, match="no gradient"):
        densify.accumulate_stats(model, torch.zeros(n, 3), filters[0])


# ---- lg_math.h child formulas through the CPU harness -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "all_split", "deg3"])
def test_child_formulas_of_lg_math_follow_the_rule(name):
    c = dc.case(name)
    n_out, n_keep, n_clone, n_s, n_child = (int(v) for v in c["counts"][:5])
    first = n_keep + n_clone
    # parents of the kept children, from the golden output: rotation is copied bit for bit, so is every other raw row
    rot = np.ascontiguousarray(c["out_rotation"][first:])
    lookup = {c["in_rotation"][i].tobytes(): i for i in range(c["in_rotation"].shape[0])}
    parents = np.array([lookup[r.tobytes()] for r in rot], dtype=np.int64)
    assert parents.shape[0] == 2 * n_child and (parents[:n_child] == parents[n_child:]).all()
    # rank of a parent among ALL split-selected rows: recover the selection from the contract's own float32 decisions
    s = np.exp(c["in_scaling"].astype(np.float32)).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.nan_to_num((c["in_accum"] / c["in_denom"]).reshape(-1), nan=0.0, posinf=np.inf)
    th = densify.thresholds(dc.model_of(c), **c["kwargs"])
    selected = np.nonzero((g >= np.float32(th["thr_g"])) & (s > np.float32(th["thr_d"])))[0]
    assert selected.shape[0] == n_s
    rank = np.searchsorted(selected, parents[:n_child])
    noise = np.ascontiguousarray(np.concatenate([c["noise"][rank], c["noise"][n_s + rank]]), np.float32)
    xyz, sc = (np.ascontiguousarray(c[k][parents], np.float32) for k in ("in_xyz", "in_scaling"))
    out_xyz, out_sc = np.zeros_like(xyz), np.zeros_like(sc)
    p = common.ptr
    dc.harness().h_densify_children(2 * n_child, p(xyz), p(sc), p(rot), p(noise), p(out_xyz), p(out_sc))
    dc.rule(f"{name} harness xyz", out_xyz, c["out_xyz"][first:], c["r64_xyz"])
    dc.rule(f"{name} harness scaling", out_sc, c["out_scaling"][first:], c["r64_scaling"])


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------

ENTRY_POINTS = {"lg_densify_scratch_bytes": 1, "lg_densify_stats": 9, "lg_densify_plan": 15, "lg_densify_rows": 12}


def test_entry_points_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, f"{name} is not declared in include/lightgaussian.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.EXPORTS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == nargs
    body = re.search(r"typedef struct lg_densify_tensor \{(.*?)\} lg_densify_tensor;", src, flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*;", body) == [f[0] for f in _lib.lg_densify_tensor._fields_]
    assert C.sizeof(_lib.lg_densify_tensor) == 24
    for k, role in enumerate(("COPY", "MOMENT", "XYZ", "SCALING", "ZERO")):
        assert int(re.search(r"#define LG_DENSIFY_%s (\d+)" % role, src).group(1)) == getattr(_lib, "DENSIFY_" + role) == k
    assert int(re.search(r"#define LG_DENSIFY_MAX_TENSORS (\d+)", src).group(1)) == _lib.DENSIFY_MAX_TENSORS
    assert int(re.search(r"#define LG_ABI_VERSION (\d+)", src).group(1)) == 7 and _lib.ABI_VERSION == 7 and lib.lg_abi_version() == 7
    # flags [N] + two uint4 per 1024 rows, each part 256-byte aligned
    assert lib.lg_densify_scratch_bytes(0) > 0
    for n in (1, 1024, 1025, 3_000_000):
        assert lib.lg_densify_scratch_bytes(n) >= n + 2 * 16 * ((n + 1023) // 1024)


def _tensor(src=0x1000, dst=0x2000, words=3, role=0):
    t = _lib.lg_densify_tensor()
    t.src, t.dst, t.row_words, t.role = src, dst, words, role
    return t


def _rows(tensors, N=10, N_out=12, map_=0x4000, record=0x5000, rotation=0x6000, scaling=0x7000, noise=0x8000, noise_rows=4, n=None):
    arr = (_lib.lg_densify_tensor * max(len(tensors), 1))(*tensors)
    return _lib.load().lg_densify_rows(N, N_out, map_, record, len(tensors) if n is None else n, arr, rotation, scaling, noise, noise_rows, 0, None)


def _plan(N=10, scaling=0x1000, opacity=0x2000, accum=0x3000, denom=0x4000, thr_g=2e-4, thr_d=0.05, thr_w=0.5, min_opacity=0.005, map_=0x5000,
          record=0x6000, scratch=0x7000):
    return _lib.load().lg_densify_plan(N, scaling, opacity, accum, denom, thr_g, thr_d, thr_w, min_opacity, 1, map_, record, scratch, 0, None)


def _stats(N=10, grad=0x1000, filt=0x2000, radii=None, max_radii=None, accum=0x3000, denom=0x4000):
    return _lib.load().lg_densify_stats(N, grad, filt, radii, max_radii, accum, denom, 0, None)


@pytest.mark.parametrize("fn, what, kwargs", [
    (_stats, "N outside", dict(N=-1)),
    (_stats, "N outside", dict(N=1 << 30)),
    (_stats, "null", dict(grad=None)),
    (_stats, "null", dict(filt=None)),
    (_stats, "null", dict(accum=None)),
    (_stats, "null", dict(denom=None)),
    (_stats, "radii without max_radii2D", dict(radii=0x5000)),
    (_stats, "aligned", dict(accum=0x3002)),
    (_plan, "N outside", dict(N=-1)),
    (_plan, "N outside", dict(N=1 << 30)),
    (_plan, "thr_g", dict(thr_g=0.0)),
    (_plan, "thr_g", dict(thr_g=-1.0)),
    (_plan, "thr_g", dict(thr_g=float("nan"))),
    (_plan, "NaN threshold", dict(thr_d=float("nan"))),
    (_plan, "null record", dict(record=None)),
    (_plan, "null scaling", dict(scaling=None)),
    (_plan, "null scaling", dict(map_=None)),
    (_plan, "null scaling", dict(scratch=None)),
    (_plan, "misaligned", dict(map_=0x5004)),
    (_plan, "misaligned", dict(opacity=0x2001)),
    (_rows, "N outside", dict(tensors=[_tensor()], N=-1)),
    (_rows, "N_out outside", dict(tensors=[_tensor()], N_out=21)),
    (_rows, "N_out outside", dict(tensors=[_tensor()], N_out=-1)),
    (_rows, "num_tensors", dict(tensors=[_tensor()], n=33)),
    (_rows, "num_tensors", dict(tensors=[_tensor()], n=-1)),
    (_rows, "noise", dict(tensors=[_tensor()], noise=None)),
    (_rows, "noise", dict(tensors=[_tensor()], noise_rows=-2)),
    (_rows, "map / record", dict(tensors=[_tensor()], map_=None)),
    (_rows, "map / record", dict(tensors=[_tensor()], record=None)),
    (_rows, "unknown role", dict(tensors=[_tensor(role=5)])),
    (_rows, "row_words", dict(tensors=[_tensor(words=0)])),
    (_rows, "null src / dst", dict(tensors=[_tensor(), _tensor(src=None)])),              # the second entry is looked at too
    (_rows, "null src / dst", dict(tensors=[_tensor(dst=None, role=4)])),
    (_rows, "4-byte aligned", dict(tensors=[_tensor(dst=0x2002)])),
    (_rows, "row_words == 3", dict(tensors=[_tensor(words=4, role=2)])),
    (_rows, "row_words == 3", dict(tensors=[_tensor(words=1, role=3)])),
    (_rows, "needs rotation and scaling", dict(tensors=[_tensor(role=2)], rotation=None)),
])
def test_invalid_arguments_refused_before_any_device_call(fn, what, kwargs):
    """This process has no GPU: a call that reached the HIP runtime would come back as LG_ERR_DEVICE."""
    assert fn(**kwargs) == _lib.LG_ERR_INVALID_ARGUMENT
    msg = _lib.load().lg_last_error().decode()
    assert fn.__name__.replace("_", "lg_densify_", 1) in msg and what in msg, msg


def test_nothing_to_do_is_ok_without_a_device():
    assert _stats(N=0, grad=None, filt=None, accum=None, denom=None) == _lib.LG_OK
    assert _rows([_tensor()], N_out=0) == _lib.LG_OK
    assert _rows([], n=0) == _lib.LG_OK
    assert _rows([_tensor(src=None, role=4)], N=0, N_out=0, map_=None, record=None, noise=None, noise_rows=0) == _lib.LG_OK


# ---- the runner -------------------------------------------------------------------------------------------------------------------

def test_hip_densify_rebinds_both_methods_and_unpatch_restores():
    if not dropin_common.available():
        pytest.skip("the reference tree is not present")
    _, gm, _ = dropin_common.load()
    cls = gm.GaussianModel
    originals = {"add_densification_stats": cls.add_densification_stats, "densify_and_prune": cls.densify_and_prune}
    try:
        report = lg_run.hip_densify()
        assert cls.add_densification_stats is lg_run._add_densification_stats and cls.densify_and_prune is lg_run._densify_and_prune
        assert set(report) == {"scene.gaussian_model.GaussianModel.add_densification_stats", "scene.gaussian_model.GaussianModel.densify_and_prune"}
        assert lg_run.hip_densify() == report                                      # idempotent
        for name, old in originals.items():
            new = getattr(cls, name)
            want = [p.name for p in inspect.signature(old).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
            have = [p.name for p in inspect.signature(new).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
            assert have[:len(want)] == want, (name, want, have)
            for p_old, p_new in zip(inspect.signature(old).parameters.values(), inspect.signature(new).parameters.values()):
                if p_old.default is not inspect.Parameter.empty:
                    assert p_new.default == p_old.default, (name, p_old.name)
        # the defaults of patch_reference() do not include it
        lg_run.unpatch_reference()
        lg_run.patch_reference()
        assert cls.densify_and_prune is originals["densify_and_prune"] and cls.add_densification_stats is originals["add_densification_stats"]
        # the rebound methods on a reference GaussianModel with CPU tensors: the torch path, the reference's result
        lg_run.hip_densify()
        c = dc.case("deg0")
        model = cls(0)
        twin = dc.model_of(c)
        for n in dc.NAMES:
            setattr(model, dc.ATTRS[n], twin.param(n))
        model.optimizer, model.percent_dense = twin.optimizer, c["percent_dense"]
        model.xyz_gradient_accum, model.denom, model.max_radii2D = twin.xyz_gradient_accum, twin.denom, twin.max_radii2D
        torch.manual_seed(777 + dc.CASES.index("deg0"))                            # the generator's seed for this case's noise
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model.densify_and_prune(*[c["kwargs"][k] for k in ("max_grad", "min_opacity", "extent", "max_screen_size")])
        model.param = lambda n: getattr(model, dc.ATTRS[n])
        dc.check_golden(model, c, "rebound deg0")
    finally:
        lg_run.unpatch_reference()
    assert cls.add_densification_stats is originals["add_densification_stats"] and cls.densify_and_prune is originals["densify_and_prune"]


def test_runner_knows_the_flag(tmp_path):
    script = tmp_path / "trainer.py"
    script.write_text("raise AssertionError('the script must not run')\n")
    with pytest.raises(SystemExit) as e:
        lg_run.main(["--no-such-flag", str(script)])
    assert "--hip-densify" in str(e.value) and "--hip-densify" in lg_run.__doc__
    src = inspect.getsource(lg_run.main)
    assert src.index("hip_densify()") < src.index("patch_reference(")            # the data-parallel wrapper wraps the new method
