"""CPU: the fused VecTree training step (lightgaussian_amd.vq.ema_update) below the kernel -- the committed golden file is
consistent with the formulas the step implements, the runner routes the reference's EuclideanCodebook.forward to it (and only
the configurations it covers), under whatever name vectree/vq.py was imported, and the two C symbols are declared and bound.
(The kernel itself: tests/test_gpu_vq_train.py.)"""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import common
import dropin_common
import vq_train_common as vc
from lightgaussian_amd import _lib
from lightgaussian_amd import run as lg_run
from lightgaussian_amd import vq as lg_vq

REF_VECTREE = os.path.join(dropin_common.REF, "vectree")


# ---- the golden file pins the formulas of ema_update on the reference ----------------------------------------------------------

@pytest.mark.parametrize("name", vc.CASES)
def test_golden_file_is_consistent_with_the_float64_restatement(name):
    case = vc.load_case(np.load(vc.GOLD), name)
    assert len(case["steps"]) >= 2
    for t, s in enumerate(case["steps"]):
        x = case["x"][s["keep"]]
        assert 1.0 - s["keep"].mean() <= 0.02, (name, t)                          # the near-tie cap of the maker
        assert x.shape == (len(s["ind"]), case["d"]) and (s["w"] is None) == (not case["weighted"])
        ind64, best, gap = vc.nearest_f64(x, s["embed_pre"])
        assert np.array_equal(ind64, s["ind"]), (name, t)                         # the reference's indices ARE the float64 argmin
        assert gap.min() >= 1e-4 * 0.9 * best.mean()
        e64, c64, new_size, _ = vc.ema_step_f64(x, s["w"], s["embed_pre"], s["cs_pre"], s["ind"])
        assert np.abs(e64 - s["embed_f64"]).max() <= 1e-12 * np.abs(e64).max(), (name, t)
        assert np.abs(c64 - s["cs_f64"]).max() <= 1e-12 * np.abs(c64).max(), (name, t)
        assert abs(new_size.sum() - len(x)) <= 1e-9 * len(x)
        # the reference's own float32 result sits at its stored deviation from those values -- and that deviation is float32 noise
        dev_e, dev_c = vc.row_error(s["embed_ref"], e64), vc.row_error(s["cs_ref"], c64)
        assert dev_e <= s["dev_embed"] * (1 + 1e-6) + 1e-12 and dev_c <= s["dev_cs"] * (1 + 1e-6) + 1e-12, (name, t, dev_e, dev_c)
        assert s["dev_embed"] < 2e-6 and s["dev_cs"] < 2e-6, (name, t, s["dev_embed"], s["dev_cs"])
        # the commitment loss the reference returned is the mean squared distance to the pre-update codes
        q = s["embed_pre"][s["ind"]].astype(np.float64)
        assert abs(((q - x) ** 2).mean() - s["loss"]) <= 1e-5 * max(s["loss"], 1e-6), (name, t)
    if len(case["steps"]) > 1:
        # some code received no row in a later step and decayed: embed * decay, cluster_size * decay
        s = case["steps"][-1]
        empty = np.setdiff1d(np.arange(case["K"]), s["ind"])
        assert len(empty) > 0
        assert np.allclose(s["embed_f64"][empty], vc.DECAY * s["embed_pre"][empty].astype(np.float64), rtol=1e-12, atol=0)


def test_golden_file_fits_the_size_limit_of_a_committed_file():
    assert os.path.getsize(vc.GOLD) < 1024 * 1024


# ---- header / binding ------------------------------------------------------------------------------------------------------

def test_the_two_symbols_are_declared_and_bound():
    hdr = open(os.path.join(common.ROOT, "include", "lightgaussian.h")).read()
    assert re.search(r"^size_t\s+lg_vq_ema_scratch_bytes\s*\(int32_t n, int32_t K, int32_t d\);", hdr, flags=re.M)
    assert re.search(r"^int\s+lg_vq_ema_step\s*\(", hdr, flags=re.M)
    assert re.search(r"#define\s+LG_ABI_VERSION\s+7\b", hdr) and _lib.ABI_VERSION == 7
    assert "lg_vq_ema_scratch_bytes" in _lib.EXPORTS and "lg_vq_ema_step" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.lg_abi_version() == 7
    assert lib.lg_vq_ema_step.argtypes is not None and len(lib.lg_vq_ema_step.argtypes) == 13
    # the size query is host arithmetic: zero exactly where the search's own query is, linear in n and K * d otherwise
    for n, K, d in ((1000, 256, 27), (80000, 8192, 27), (80000, 8192, 48), (1, 1, 1), (500000, 65536, 63)):
        b = lib.lg_vq_ema_scratch_bytes(n, K, d)
        assert 0 < b < 128 * n + 16 * K * (d + 2) + (1 << 20) + lib.lg_vq_scratch_bytes(K, d), (n, K, d, b)
    for n, K, d in ((1000, 256, 64), (1000, 0, 27), (1000, 256, 0), (-1, 256, 27), (1 << 30, 256, 27)):
        assert lib.lg_vq_ema_scratch_bytes(n, K, d) == 0, (n, K, d)
        if n >= 0 and n < (1 << 30):
            assert lib.lg_vq_scratch_bytes(K, d) == 0
    # argument checks come before any launch (no GPU here)
    assert lib.lg_vq_ema_step(10, 64, 8, None, None, None, None, 0.8, 1e-5, None, None, 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_vq_ema_step(0, 27, 8, None, None, None, None, 0.8, 1e-5, None, None, 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_vq_ema_step(10, 27, 8, None, None, None, None, 0.8, 1e-5, None, None, 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert b"missing buffer" in lib.lg_last_error()


def test_ema_update_argument_errors_need_no_gpu():
    x, e, c = torch.zeros(10, 5), torch.zeros(4, 5), torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lg_vq.ema_update(x, e, c)
    with pytest.raises(ValueError):
        lg_vq.ema_update(x, torch.zeros(4, 6), c)
    with pytest.raises(ValueError):
        lg_vq.ema_update(x, e, torch.zeros(5))
    with pytest.raises(ValueError):
        lg_vq.ema_update(x, e, c, weight=torch.ones(9))
    with pytest.raises(ValueError):
        lg_vq.ema_update(torch.zeros(0, 5), e, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lg_vq.train_codebook(torch.zeros(10, 5), torch.ones(10), e, c, iterations=1)


# ---- runner wiring on the reference's real module ---------------------------------------------------------------------------

class _FakeHip(torch.Tensor):
    """A CPU tensor that answers is_cuda = True: what the runner's gate looks at.  (The recorder below stands in for the kernel.)"""
    is_cuda = property(lambda self: True)


def _hip(t):
    return t.detach().clone().as_subclass(_FakeHip)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, flatten, embed, cluster_size, weight=None, decay=0.8, eps=1e-5, return_quantized=False):
        self.calls.append(dict(flatten=flatten, embed=embed, cluster_size=cluster_size, weight=weight, decay=decay, eps=eps,
                               return_quantized=return_quantized))
        h, n, d = flatten.shape
        ind = torch.arange(h * n, dtype=torch.int64).reshape(h, n) % embed.shape[1]
        return ind, torch.stack([torch.Tensor(embed[i])[ind[i]] for i in range(h)])


@pytest.fixture()
def clean_imports():
    """sys.path / sys.modules as they were, once the test ends: later tests see what they saw before."""
    if not os.path.exists(os.path.join(REF_VECTREE, "vq.py")):
        pytest.skip("the reference tree is not present")
    pytest.importorskip("einops")
    path, mods = list(sys.path), dict(sys.modules)
    yield
    lg_run.unpatch_reference()
    sys.path[:] = path
    for name, mod in list(sys.modules.items()):
        if name not in mods and (name == "vq" or str(getattr(mod, "__file__", "") or "").startswith(dropin_common.REF)):
            del sys.modules[name]
    for name in ("vq", "vectree", "vectree.vq"):
        if name in mods:
            sys.modules[name] = mods[name]


def _reference_vq_as_package():
    if dropin_common.REF not in sys.path:
        sys.path.insert(0, dropin_common.REF)
    return importlib.import_module("vectree.vq")


def _stub_search(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(lg_vq, "ema_update", rec)
    monkeypatch.setattr(lg_vq, "nearest_code", lambda a, b: torch.cdist(torch.Tensor(a), torch.Tensor(b)).argmin(-1))
    return rec


def test_patched_forward_hands_the_modules_own_buffers_to_ema_update(clean_imports, monkeypatch):
    vq = _reference_vq_as_package()
    original = vq.EuclideanCodebook.forward
    rec = _stub_search(monkeypatch)
    report = lg_run.patch_reference()
    assert vq.EuclideanCodebook.forward is not original
    assert any(k.startswith("vectree.vq.EuclideanCodebook.forward") and "skipped" not in v for k, v in report.items()), sorted(report)
    assert lg_run.patch_reference() == report                                      # idempotent
    torch.manual_seed(0)
    model = vq.VectorQuantize(dim=6, codebook_size=8, decay=0.8, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0).train()
    cb = model._codebook
    cb._buffers["embed"], cb._buffers["cluster_size"] = _hip(cb.embed), _hip(cb.cluster_size)
    embed_before = torch.Tensor(cb.embed).clone()
    x, w = _hip(torch.randn(1, 50, 6)), _hip(torch.rand(1, 50, 1) + 0.1)
    quantize, embed_ind, loss = model(x, weight=w)                                 # vectree/vectree.py:200
    assert len(rec.calls) == 1
    call = rec.calls[0]
    assert call["embed"] is cb._buffers["embed"] and call["cluster_size"] is cb._buffers["cluster_size"]     # in place, on the module's state
    assert tuple(call["flatten"].shape) == (1, 50, 6) and call["weight"] is w and call["return_quantized"] is True
    assert call["decay"] == cb.decay == 0.8 and call["eps"] == cb.eps
    assert tuple(quantize.shape) == (1, 50, 6) and tuple(embed_ind.shape) == (1, 50) and embed_ind.dtype == torch.int64
    assert torch.equal(torch.Tensor(embed_ind), rec(x, cb.embed, cb.cluster_size)[0])
    assert loss.shape == (1,) and float(loss) > 0                                  # VectorQuantize.forward went on to its commitment loss
    assert torch.equal(torch.Tensor(cb.embed), embed_before)                        # (the recorder updates nothing)
    # the codebook called directly, [1, n, d] and [1, b, n, d]: the shapes of the original forward
    rec.calls.clear()
    q3, i3 = cb(x, w)
    q4, i4 = cb(x.reshape(1, 5, 10, 6))
    assert len(rec.calls) == 2 and rec.calls[1]["weight"] is None and tuple(rec.calls[1]["flatten"].shape) == (1, 50, 6)
    twin = vq.EuclideanCodebook(dim=6, codebook_size=8, threshold_ema_dead_code=0).train()
    o3, oi3 = original(twin, torch.Tensor(x), torch.Tensor(w))
    o4, oi4 = original(twin, torch.Tensor(x).reshape(1, 5, 10, 6))
    assert (tuple(q3.shape), tuple(i3.shape)) == (tuple(o3.shape), tuple(oi3.shape)) == ((1, 50, 6), (1, 50))
    assert (tuple(q4.shape), tuple(i4.shape)) == (tuple(o4.shape), tuple(oi4.shape)) == ((1, 5, 10, 6), (1, 5, 10))
    lg_run.unpatch_reference()
    assert vq.EuclideanCodebook.forward is original and vq.torch is torch


def test_every_other_configuration_runs_the_original_forward(clean_imports, monkeypatch):
    vq = _reference_vq_as_package()
    rec = _stub_search(monkeypatch)
    cosine_forward = vq.CosineSimCodebook.forward

    def pair(**kw):
        torch.manual_seed(1)
        a = vq.EuclideanCodebook(dim=6, codebook_size=8, **kw)
        b = vq.EuclideanCodebook(dim=6, codebook_size=8, **kw)
        b.load_state_dict(a.state_dict())
        return a, b

    torch.manual_seed(2)
    x, w = torch.randn(1, 40, 6), torch.rand(1, 40, 1) + 0.1
    # unpatched results first
    plain_train, patched_train = pair(threshold_ema_dead_code=0)
    plain_eval, patched_eval = pair(threshold_ema_dead_code=0)
    plain_eval.eval(); patched_eval.eval()
    want_train, want_eval = plain_train(x, w), plain_eval(x)
    lg_run.patch_reference()
    # CPU tensors in training mode: the reference's own step, bit for bit, state included
    got = patched_train(x, w)
    assert torch.equal(got[0], want_train[0]) and torch.equal(got[1], want_train[1])
    assert torch.equal(patched_train.embed, plain_train.embed) and torch.equal(patched_train.cluster_size, plain_train.cluster_size)
    # eval mode, also on "HIP" tensors: the search proxy, not the training step
    got = patched_eval(x)
    assert torch.equal(got[0], want_eval[0]) and torch.equal(got[1], want_eval[1])
    patched_eval._buffers["embed"], patched_eval._buffers["cluster_size"] = _hip(patched_eval.embed), _hip(patched_eval.cluster_size)
    got = patched_eval(_hip(x))
    assert torch.equal(torch.Tensor(got[1]), want_eval[1])
    assert not rec.calls

    def hip_module(m):
        m._buffers["embed"], m._buffers["cluster_size"] = _hip(m.embed), _hip(m.cluster_size)
        return m.train()

    # code expiry != 0, a temperature, a DDP reduce function, a learnable codebook, a half-precision input: the original forward
    expiry = hip_module(vq.EuclideanCodebook(dim=6, codebook_size=8, threshold_ema_dead_code=2))
    expiry(_hip(x), _hip(w))
    ddp = hip_module(vq.EuclideanCodebook(dim=6, codebook_size=8, threshold_ema_dead_code=0))
    ddp.all_reduce_fn = lambda t: None
    ddp(_hip(x), _hip(w))
    half = hip_module(vq.EuclideanCodebook(dim=6, codebook_size=8, threshold_ema_dead_code=0))
    half(_hip(x.double()), _hip(w))
    assert not rec.calls
    # ... and the same module with nothing unusual about it does go to the fused step
    ok = hip_module(vq.EuclideanCodebook(dim=6, codebook_size=8, threshold_ema_dead_code=0))
    ok(_hip(x), _hip(w))
    assert len(rec.calls) == 1
    # the cosine codebook is another class: untouched
    assert vq.CosineSimCodebook.forward is cosine_forward
    vq.CosineSimCodebook(dim=6, codebook_size=8, threshold_ema_dead_code=0).train()(x)
    assert len(rec.calls) == 1


def test_the_module_imported_as_top_level_vq_is_patched_too(clean_imports, monkeypatch):
    """vectree/vectree.py does `from vq import VectorQuantize` with its own directory first on sys.path: the module the script
    uses is top-level `vq`.  The runner patches before the script runs (nothing imported yet) and must find it then -- and also
    when it has been imported already."""
    rec = _stub_search(monkeypatch)
    for name in ("vq", "vectree", "vectree.vq"):
        sys.modules.pop(name, None)
    sys.path.insert(0, REF_VECTREE)                                  # what `python vectree/vectree.py` (and the runner) set up
    report = lg_run.patch_reference()
    vq = importlib.import_module("vq")                               # the script's own import, afterwards
    assert os.path.samefile(vq.__file__, os.path.join(REF_VECTREE, "vq.py")) and vq.__name__ == "vq"
    assert type(vq.torch).__name__ == "_TorchProxy" and vq.gumbel_sample.__module__ == "lightgaussian_amd.run"
    assert vq.EuclideanCodebook.forward.__module__ == "lightgaussian_amd.run"
    assert "vq.gumbel_sample" in report and any(k.startswith("vq.EuclideanCodebook.forward") for k in report), sorted(report)
    assert "vectree" not in sys.modules                              # vectree.py itself was not executed as a module on the way
    model = vq.VectorQuantize(dim=6, codebook_size=8, decay=0.8, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0).train()
    cb = model._codebook
    cb._buffers["embed"], cb._buffers["cluster_size"] = _hip(cb.embed), _hip(cb.cluster_size)
    model(_hip(torch.randn(1, 30, 6)), weight=_hip(torch.ones(1, 30, 1)))
    assert len(rec.calls) == 1
    lg_run.unpatch_reference()
    assert vq.torch is torch and vq.EuclideanCodebook.forward.__module__ != "lightgaussian_amd.run"
    # already imported under that name when the patch comes
    lg_run.patch_reference()
    assert type(vq.torch).__name__ == "_TorchProxy" and vq.EuclideanCodebook.forward.__module__ == "lightgaussian_amd.run"
    lg_run.unpatch_reference()
    assert vq.torch is torch
