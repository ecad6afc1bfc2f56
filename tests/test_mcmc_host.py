"""lightgaussian_amd.mcmc without a GPU: the lg_math.h functions through a g++ harness against the float64 twin of
tests/mcmc_common.py, the torch backend of relocate / grow / add_noise on CPU tensors, the extension header against the module's
prototype table, and the argument checks of the library and of the Python layer."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import common
import densify_common as dc
import mcmc_common as mc
import test_abi
import tolerance
from lightgaussian_amd import _lib, mcmc

HDR_MCMC = os.path.join(common.ROOT, "include", "lightgaussian_mcmc.h")
OPACITIES = (0.005, 0.01, 0.1, 0.5, 0.9, 0.999, 1.0 - 2.0 ** -20)
COPIES = (2, 3, 10, 35, 51)


def fptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. the math of lg_math.h -------------------------------------------------------------------------------------------------------

def test_closed_form_sum_equals_the_double_loop():
    h = mc.harness()
    worst = 0.0
    for o in OPACITIES:
        for M in COPIES:
            x = mc.x_of(o, M)
            want, got = mc.double_loop_D(x, M), h.h_mcmc_binomial_sum(x, M)
            worst = max(worst, abs(got - want) / abs(want))
            assert abs(got - want) <= 1e-12 * abs(want), (o, M, got, want)
    print(f"closed form against the double loop: worst relative difference {worst:.3e}")


def test_relocation_function_against_the_twin():
    h = mc.harness()
    gen = np.random.default_rng(3)
    raws, cnts = [], []
    for o in OPACITIES:
        for cnt in (1, 2, 9, 34, 50, 51, 200):
            raws.append(math.log(o / (1.0 - o)))
            cnts.append(cnt)
    opacity = np.asarray(raws, np.float32)
    cnt = np.asarray(cnts, np.int32)
    scaling = gen.uniform(-6.0, 0.5, size=(opacity.size, 3)).astype(np.float32)
    got_op, got_sc = np.empty_like(opacity), np.empty_like(scaling)
    h.h_mcmc_relocate(opacity.size, fptr(opacity), fptr(scaling), fptr(cnt), 0.005, fptr(got_op), fptr(got_sc))
    r64_op, r64_sc = mc.relocation_r64(opacity, scaling, cnt, 0.005)
    for what, got, r64 in (("opacity'", got_op, r64_op), ("scaling'", got_sc, r64_sc)):
        ratio = np.abs(got.astype(np.float64) - r64) / (mc.EXACT * np.abs(r64))
        print(f"{what}: worst |got - r64| / (2^-23 |r64|) = {ratio.max():.3f}")
        assert np.isfinite(got).all() and ratio.max() <= 1.0, (what, int(ratio.argmax()))
    # counts above 51 are clamped: 50 draws and 200 draws of one row give the same bits
    assert np.array_equal(got_op[cnt == 200], got_op[cnt == 50]) and np.array_equal(got_op[cnt == 51], got_op[cnt == 50])
    assert not np.array_equal(got_op[cnt == 34], got_op[cnt == 50])


@pytest.mark.parametrize("n", [1, 777])
def test_noise_function_against_the_twin_and_the_torch_backend(n):
    h = mc.harness()
    c = mc.noise_case(n, seed=40 + n)
    arrays = [np.ascontiguousarray(c[k], np.float32) for k in ("in_xyz", "in_scaling", "in_rotation", "in_opacity", "noise")]
    xyz_lr, noise_lr = 1e-5, 5e5                # c = 5: steps of the size of the scene
    cc = float(np.float32(noise_lr * xyz_lr))
    got, gate = np.empty_like(arrays[0]), np.empty(n, np.float32)
    h.h_mcmc_noise(n, *(fptr(a) for a in arrays), cc, 100.0, 0.995, fptr(got), fptr(gate))
    model = dc.model_of(c)
    mcmc.add_noise(model, xyz_lr, noise_lr=noise_lr, noise=torch.from_numpy(c["noise"]), backend="torch")
    r32 = model._xyz.detach().numpy()
    r64 = mc.noise_r64(*arrays, cc, 100.0, 0.995)
    tolerance.assert_rule3(got, r64, r32, f"noise N={n} xyz", ref="torch backend")
    step64 = r64 - arrays[0].astype(np.float64)
    tolerance.assert_rule3(got.astype(np.float64) - arrays[0], step64, r32.astype(np.float64) - arrays[0], f"noise N={n} step", ref="torch backend",
                           nonzero=n > 1)
    still = gate == 0.0
    if n > 1:
        assert still.any() and (~still).any() and np.abs(step64).max() > 0.5          # the gate reaches exact 0; steps of the scene's size
    assert np.array_equal(got[still].view(np.int32), arrays[0][still].view(np.int32))


def test_gate_overflow_gives_zero_not_nan():
    h = mc.harness()
    one = lambda v: np.asarray(v, np.float32)          # noqa: E731
    xyz, scaling, rotation, noise = one([[1, 2, 3]]), one([[0, 0, 0]]), one([[1, 0, 0, 0]]), one([[1, 1, 1]])
    got, gate = np.empty_like(xyz), np.empty(1, np.float32)
    for raw in (2.5, 40.0, 200.0):                      # sigma -> 1: exp(-k (1 - sigma - x0)) overflows float32
        h.h_mcmc_noise(1, fptr(xyz), fptr(scaling), fptr(rotation), fptr(one([raw])), fptr(noise), 1.0, 100.0, 0.995, fptr(got), fptr(gate))
        assert gate[0] == 0.0 and np.array_equal(got, xyz)


# ---- 2. the torch backend: relocation and growth ------------------------------------------------------------------------------------

def relocate_inputs(c):
    dead = mc.dead_rows(c)
    dst = torch.nonzero(dead).reshape(-1)
    alive = torch.nonzero(~dead).reshape(-1)
    return dst, mc.hand_draws(alive[:: max(1, alive.numel() // 40)], dst.numel())


def test_torch_relocate_against_the_twin():
    c = mc.case(8000, seed=1)
    dst, src = relocate_inputs(c)
    assert dst.numel() > 250 and int(torch.bincount(src).max()) == 200
    model = dc.model_of(c)
    before = [model.param(n) for n in dc.NAMES]
    keys = list(model.optimizer.state.keys())
    rec = mcmc.relocate(model, draws=src, backend="torch")
    assert rec["backend"] == "torch" and rec["n_dead"] == dst.numel() and int(rec["n_sources"]) == torch.unique(src).numel()
    assert all(a is model.param(n) for a, n in zip(before, dc.NAMES)) and list(model.optimizer.state.keys()) == keys
    mc.check_state(model, mc.expected_state(c, dst, src, 8000, 0.005), dst, src, "torch relocate", exact=False)
    dc.can_step(model)


@pytest.mark.parametrize("deg", [0, 1])
def test_torch_grow_against_the_twin(deg):
    n = 7000
    c = mc.case(n, deg=deg, seed=2)
    n_new = int(1.05 * n) - n
    src = mc.hand_draws(range(3, n, 97), n_new)
    model = dc.model_of(c)
    before = [model.param(k) for k in dc.NAMES]
    rec = mcmc.grow(model, cap_max=10 ** 6, draws=src, backend="torch")
    assert rec["backend"] == "torch" and rec["N_out"] == n + n_new and rec["n_new"] == n_new
    assert not any(a is model.param(k) for a, k in zip(before, dc.NAMES))
    dst = torch.arange(n, n + n_new)
    mc.check_state(model, mc.expected_state(c, dst, src, n + n_new, 0.005), dst, src, f"torch grow deg {deg}", exact=False)
    for name, old in (("xyz_gradient_accum", c["in_accum"]), ("denom", c["in_denom"]), ("max_radii2D", c["in_max_radii2D"])):
        t = getattr(model, name)
        assert t.shape[0] == n + n_new and dc.same_bits(t[:n], torch.from_numpy(np.asarray(old, np.float32))) and not t[n:].any()
    dc.can_step(model)
    # the cap binds
    rec = mcmc.grow(model, cap_max=n + n_new + 10, backend="torch")
    assert rec["n_new"] == 10 and model._xyz.shape[0] == n + n_new + 10


def test_seeded_default_draws_consume_the_stream_as_documented():
    c = mc.case(3000, seed=5)
    a, b = dc.model_of(c), dc.model_of(c)
    dead = mc.dead_rows(c)
    alive = torch.nonzero(~dead).reshape(-1)
    sigma = torch.sigmoid(torch.from_numpy(c["in_opacity"])).reshape(-1)
    torch.manual_seed(9)
    draws = alive[torch.multinomial(sigma[alive], int(dead.sum()), replacement=True)]
    state = torch.get_rng_state()
    torch.manual_seed(9)
    mcmc.relocate(a, backend="torch")
    assert torch.equal(torch.get_rng_state(), state)
    mcmc.relocate(b, draws=draws, backend="torch")
    assert all(dc.same_bits(a.param(n), b.param(n)) for n in dc.NAMES)
    # grow: multinomial over all rows; add_noise: randn_like
    torch.manual_seed(10)
    draws = torch.multinomial(torch.sigmoid(a._opacity.detach()).reshape(-1), 150, replacement=True)
    noise = torch.randn(3150, 3)
    torch.manual_seed(10)
    mcmc.grow(a, cap_max=10 ** 6, backend="torch")
    mcmc.add_noise(a, 1e-6, backend="torch")
    mcmc.grow(b, cap_max=10 ** 6, draws=draws, backend="torch")
    mcmc.add_noise(b, 1e-6, noise=noise, backend="torch")
    assert all(dc.same_bits(a.param(n), b.param(n)) for n in dc.NAMES)


def test_large_category_counts_draw_by_inverse_cdf(monkeypatch):
    monkeypatch.setattr(mcmc, "MULTINOMIAL_MAX", 100)
    w = torch.zeros(1000)
    w[[7, 500, 999]] = torch.tensor([1.0, 2.0, 1.0])
    torch.manual_seed(0)
    d = mcmc._draw(w, 4000)
    assert d.dtype == torch.int64 and set(d.tolist()) == {7, 500, 999}
    assert 1800 < int((d == 500).sum()) < 2200


def test_empty_cases_change_nothing():
    c = mc.case(500, seed=6, dead=0.0)
    for backend in ("torch", "hip"):                    # (no dead row: neither backend has anything to launch, GPU or not)
        model = dc.model_of(c)
        rec = mcmc.relocate(model, backend=backend)
        assert rec["n_dead"] == 0 and int(rec["n_sources"]) == 0
        assert all(dc.same_bits(model.param(n), torch.from_numpy(c[f"in_{n}"])) for n in dc.NAMES)
        rec = mcmc.grow(model, cap_max=500, backend=backend)
        assert rec["n_new"] == 0 and rec["N_out"] == 500 and model._xyz.shape[0] == 500
        assert mcmc.grow(model, cap_max=100, backend=backend)["n_new"] == 0
    c["in_opacity"][:] = -9.0                           # all rows dead: nobody to copy
    model = dc.model_of(c)
    rec = mcmc.relocate(model, backend="torch")
    assert rec["n_dead"] == 500 and all(dc.same_bits(model.param(n), torch.from_numpy(c[f"in_{n}"])) for n in dc.NAMES)


def test_bad_draws_and_arguments_raise():
    c = mc.case(400, seed=7)
    model = dc.model_of(c)
    dead = mc.dead_rows(c)
    n_dead = int(dead.sum())
    alive, gone = torch.nonzero(~dead).reshape(-1), torch.nonzero(dead).reshape(-1)
    good = alive[:1].repeat(n_dead)
    for bad in (good[:-1], good.to(torch.int32), good.clone().index_fill_(0, torch.tensor([0]), 400),
                good.clone().index_fill_(0, torch.tensor([0]), -1), good.clone().index_fill_(0, torch.tensor([0]), int(gone[0])), good.tolist()):
        with pytest.raises(ValueError):
            mcmc.relocate(model, draws=bad, backend="torch")
    for bad in (torch.zeros(19, dtype=torch.int64), torch.zeros(20, dtype=torch.float32), torch.full((20,), 400, dtype=torch.int64)):
        with pytest.raises(ValueError):
            mcmc.grow(model, cap_max=10 ** 6, draws=bad, backend="torch")
    with pytest.raises(ValueError):
        mcmc.add_noise(model, 1e-6, noise=torch.zeros(399, 3), backend="torch")
    with pytest.raises(ValueError):
        mcmc.relocate(model, backend="cuda")
    assert all(dc.same_bits(model.param(n), torch.from_numpy(c[f"in_{n}"])) for n in dc.NAMES)


def test_regularizers_and_the_schedule():
    c = mc.case(300, seed=8)
    model = dc.model_of(c)
    loss = mcmc.regularizers(model, opacity_reg=0.01, scale_reg=0.02)
    want = 0.01 * torch.sigmoid(model._opacity).abs().mean() + 0.02 * torch.exp(model._scaling).abs().mean()
    assert torch.allclose(loss, want) and loss.requires_grad
    loss.backward()
    assert model._opacity.grad is not None and model._scaling.grad is not None and model._xyz.grad is None
    # off the schedule only the noise runs; on it the model grows to the cap
    xyz = model._xyz.detach().clone()
    done = mcmc.after_step(model, 150, 1e-6, 310, start=100, stop=1000, every=100, backend="torch")
    assert done == {"relocate": None, "grow": None} and model._xyz.shape[0] == 300 and not torch.equal(model._xyz.detach(), xyz)
    done = mcmc.after_step(model, 200, 1e-6, 310, start=100, stop=1000, every=100, backend="torch")
    assert done["relocate"]["n_dead"] > 0 and done["grow"]["N_out"] == 310 == model._xyz.shape[0]
    assert mcmc.after_step(model, 1000, 1e-6, 400, start=100, stop=1000, every=100, backend="torch")["grow"] is None
    model.optimizer._lg_dp_wrapped = True
    with pytest.raises(RuntimeError, match="data-parallel"):
        mcmc.after_step(model, 200, 1e-6, 310, backend="torch")


def test_hip_backend_falls_back_with_one_warning_per_reason():
    c = mc.case(200, seed=9)
    model = dc.model_of(c)                              # CPU parameters
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert mcmc.relocate(model, backend="hip")["backend"] == "torch"
        mcmc.add_noise(model, 1e-6, backend="hip")
        assert mcmc.grow(model, cap_max=10 ** 6, backend="hip")["backend"] == "torch"
        mcmc.add_noise(model, 1e-6, backend="hip")
        assert mcmc.relocate(model, backend="hip")["backend"] in ("torch", "hip")
    seen = [w for w in caught if "outside the HIP path" in str(w.message)]
    assert len(seen) == 3, [str(w.message) for w in caught]          # relocate, add_noise, grow: each once


# ---- 3. the extension header and the library's argument checks ----------------------------------------------------------------------

def mcmc_header(monkeypatch):
    """test_abi's parse pointed at the extension header alone."""
    monkeypatch.setattr(test_abi, "HDR", HDR_MCMC)
    monkeypatch.setattr(test_abi, "HDR_DEBUG", os.devnull)


def test_extension_header_matches_the_prototype_table(monkeypatch):
    frozen = test_abi._header_prototypes()
    assert len(frozen) == 67 and len(_lib.PROTOTYPES) == 67 and not [n for n in frozen if n.startswith("lg_mcmc")]
    assert len(test_abi._header_constants()) == 36 and len(test_abi._header_structs()) == 8
    mcmc_header(monkeypatch)
    declared = test_abi._header_prototypes()
    assert sorted(declared) == sorted(test_abi._declared_functions(HDR_MCMC)) == sorted(mcmc.PROTOTYPES)
    assert all(n.startswith("lg_mcmc_") for n in declared) and len(declared) == 4
    assert test_abi._prototype_mismatches(declared, mcmc.PROTOTYPES) == []
    assert declared["lg_mcmc_rows"] == ("int32", ["int32", "int64", "int32"] + ["pointer"] * 3 + ["int32", "pointer", "uint32", "pointer"])
    assert not set(declared) & set(_lib.PROTOTYPES) and test_abi._header_structs() == {}
    values = test_abi._header_constants()
    assert values and all(n.startswith("LG_MCMC_") for n in values)
    for name, value in values.items():
        assert getattr(mcmc, name[len("LG_"):]) == value, name
    assert {n for n in vars(mcmc) if n.startswith("MCMC_")} == {n[len("LG_"):] for n in values}
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in declared)
    assert (mcmc.MCMC_COPY, mcmc.MCMC_MOMENT) == (_lib.DENSIFY_COPY, _lib.DENSIFY_MOMENT) and _lib.ABI_VERSION == 7


def refused(rc, *words):
    msg = _lib.load().lg_last_error().decode()
    assert rc == _lib.LG_ERR_INVALID_ARGUMENT and all(w in msg for w in words), (rc, msg)


def test_library_refuses_bad_arguments_before_any_device_call():
    lib = mcmc.load()
    A = C.c_void_p(4096)                                # a well-aligned address that is never looked through: every call below is refused
    odd = C.c_void_p(4098)
    assert lib.lg_mcmc_scratch_bytes(1000) >= 1000 * 20 and lib.lg_mcmc_scratch_bytes(0) > 0
    names = ("xyz", "scaling", "rotation", "opacity", "noise")
    for k, name in enumerate(names):
        ptrs = [A] * 5
        ptrs[k] = None
        refused(lib.lg_mcmc_noise(10, *ptrs, 1.0, 100.0, 0.995, 0, None), "lg_mcmc_noise", "null", name)
    refused(lib.lg_mcmc_noise(-1, A, A, A, A, A, 1.0, 100.0, 0.995, 0, None), "lg_mcmc_noise", "N outside")
    refused(lib.lg_mcmc_noise(1 << 30, A, A, A, A, A, 1.0, 100.0, 0.995, 0, None), "lg_mcmc_noise", "N outside")
    refused(lib.lg_mcmc_noise(10, A, A, A, A, A, float("nan"), 100.0, 0.995, 0, None), "lg_mcmc_noise", "NaN")
    refused(lib.lg_mcmc_noise(10, A, odd, A, A, A, 1.0, 100.0, 0.995, 0, None), "lg_mcmc_noise", "aligned")
    for k, name in enumerate(("src", "opacity", "scaling", "scratch")):
        ptrs = [A] * 4
        ptrs[k] = None
        refused(lib.lg_mcmc_plan(10, 5, ptrs[0], ptrs[1], ptrs[2], 0.005, ptrs[3], 0, None), "lg_mcmc_plan", "null", name)
    refused(lib.lg_mcmc_plan(1 << 30, 5, A, A, A, 0.005, A, 0, None), "lg_mcmc_plan", "N outside")
    refused(lib.lg_mcmc_plan(10, -1, A, A, A, 0.005, A, 0, None), "lg_mcmc_plan", "n < 0")
    refused(lib.lg_mcmc_plan(0, 5, A, A, A, 0.005, A, 0, None), "lg_mcmc_plan", "empty model")
    refused(lib.lg_mcmc_plan(10, 5, A, A, A, 1.0, A, 0, None), "lg_mcmc_plan", "min_opacity")
    refused(lib.lg_mcmc_plan(10, 5, A, A, A, float("nan"), A, 0, None), "lg_mcmc_plan", "min_opacity")
    refused(lib.lg_mcmc_plan(10, 5, A, A, A, 0.005, C.c_void_p(4104), 0, None), "lg_mcmc_plan", "misaligned", "scratch")
    table = (_lib.lg_densify_tensor * 2)()

    def fill(src=4096, dst=4096, words=3, role=mcmc.MCMC_COPY):
        for row in table:
            row.src, row.dst, row.row_words, row.role = 4096, 4096, 3, mcmc.MCMC_COPY
        table[1].src, table[1].dst, table[1].row_words, table[1].role = src, dst, words, role
        return table

    rows = lambda n=10, n_out=10, k=5, dst=A, src=A, scratch=A, nt=2, t=None: lib.lg_mcmc_rows(n, n_out, k, dst, src, scratch, nt, t or fill(), 0, None)   # noqa: E731
    refused(rows(n=1 << 30, n_out=1 << 30), "lg_mcmc_rows", "N outside")
    refused(rows(n_out=9), "lg_mcmc_rows", "N_out")
    refused(rows(n_out=1 << 31), "lg_mcmc_rows", "N_out")
    refused(rows(k=-1), "lg_mcmc_rows", "n < 0")
    refused(rows(nt=33), "lg_mcmc_rows", "num_tensors")
    refused(lib.lg_mcmc_rows(10, 10, 5, A, A, A, 2, None, 0, None), "lg_mcmc_rows", "null tensors")
    refused(rows(dst=None), "lg_mcmc_rows", "null dst")
    refused(rows(src=None), "lg_mcmc_rows", "null src")
    refused(rows(scratch=None), "lg_mcmc_rows", "null scratch")
    refused(rows(src=odd), "lg_mcmc_rows", "misaligned")
    refused(rows(t=fill(role=4)), "lg_mcmc_rows", "tensors", "role")
    refused(rows(t=fill(words=0)), "lg_mcmc_rows", "tensors", "row_words")
    refused(rows(t=fill(src=0, dst=0)), "lg_mcmc_rows", "tensors", "null src / dst")
    refused(rows(t=fill(src=4098, dst=4098)), "lg_mcmc_rows", "tensors", "aligned")
    refused(rows(t=fill(role=mcmc.MCMC_OPACITY)), "lg_mcmc_rows", "tensors", "opacity role")
    refused(rows(t=fill(role=mcmc.MCMC_SCALING, words=1)), "lg_mcmc_rows", "tensors", "scaling role")
    refused(rows(t=fill(dst=8192)), "lg_mcmc_rows", "tensors", "src == dst")              # in place with separate tensors
    refused(rows(n_out=12), "lg_mcmc_rows", "tensors", "src == dst")                      # growth onto the source tensors
    # nothing to do is not an error, and launches nothing
    assert lib.lg_mcmc_noise(0, None, None, None, None, None, 1.0, 100.0, 0.995, 0, None) == _lib.LG_OK
    assert lib.lg_mcmc_plan(0, 0, None, None, None, 0.005, None, 0, None) == _lib.LG_OK
    assert lib.lg_mcmc_rows(10, 10, 0, None, None, None, 2, fill(), 0, None) == _lib.LG_OK
    assert lib.lg_mcmc_rows(10, 12, 5, A, A, A, 0, None, 0, None) == _lib.LG_OK
