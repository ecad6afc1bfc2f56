"""The poisoned, guarded torch.empty of tests/poison_common.py, on the CPU: what it hands out, what it lets through, that it restores
the three names, that its guard check sees one byte -- and the host-side prune functions under the three patterns."""
import numpy as np
import pytest
import torch

import common  # noqa: F401
import poison_common as pz
from poison_common import ONE, SENTINEL, ZERO, poisoned

WORDS = (ZERO, SENTINEL, ONE)


def _words(t, raw, nbytes):
    """The tensor's bytes, straight from the raw block."""
    return raw[pz.GUARD:pz.GUARD + nbytes]


def _pattern_bytes(word, n):
    return np.resize(np.array([word], np.uint32).view(np.uint8), n)


@pytest.mark.parametrize("word", WORDS)
def test_size_forms_give_a_contiguous_aligned_tensor_that_holds_the_pattern(word):
    with poisoned(word, "cpu") as p:
        made = [torch.empty((3, 5)), torch.empty(3, 5), torch.empty(7), torch.empty(torch.Size([3, 5])), torch.empty(size=(3, 5)),
                torch.empty([3, 5], dtype=torch.float32, device="cpu")]
        for t, shape in zip(made, [(3, 5), (3, 5), (7,), (3, 5), (3, 5), (3, 5)]):
            assert t.shape == shape and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 64 == 0    # (the CPU allocator aligns to 64)
            assert np.array_equal(t.view(torch.int32).numpy().view(np.uint32), np.full(shape, word, np.uint32))
        assert len(p.allocations) == len(made)
        for (raw, nbytes), t in zip(p.allocations, made):
            assert nbytes == t.numel() * 4 and raw.numel() == 2 * pz.GUARD + nbytes and raw.data_ptr() + pz.GUARD == t.data_ptr()
        p.check_guards()


@pytest.mark.parametrize("dtype,shape", [(torch.uint8, (7,)), (torch.uint8, (3, 5)), (torch.int32, (3,)), (torch.float32, (2, 3)),
                                         (torch.int64, (5,)), (torch.float16, (3,)), (torch.bool, (9,))])
def test_dtypes_and_byte_counts_that_are_no_multiple_of_four(dtype, shape):
    with poisoned(SENTINEL, "cpu") as p:
        t = torch.empty(shape, dtype=dtype)
        (raw, nbytes), = p.allocations
        assert t.dtype == dtype and t.shape == shape and nbytes == t.numel() * t.element_size()
        assert raw.numel() == pz.GUARD + (nbytes + 3) // 4 * 4 + pz.GUARD
        assert np.array_equal(_words(t, raw, nbytes).numpy(), _pattern_bytes(SENTINEL, nbytes))
        assert np.array_equal(t.view(torch.uint8).numpy().reshape(-1), _pattern_bytes(SENTINEL, nbytes))
    t.fill_(1)                  # the tensor outlives the block and is ordinary memory
    p.check_guards()


def test_a_zero_size_tensor_still_gets_both_guards():
    with poisoned(ONE, "cpu") as p:
        t = torch.empty((0, 3), dtype=torch.int64)
        u = torch.empty(0)
        assert t.shape == (0, 3) and t.dtype == torch.int64 and u.shape == (0,)
        for raw, nbytes in p.allocations:
            assert nbytes == 0 and raw.numel() == 2 * pz.GUARD
            assert np.array_equal(raw.numpy(), _pattern_bytes(ONE, 2 * pz.GUARD))


def test_empty_like_and_new_empty_are_poisoned_too_and_requires_grad_is_applied():
    src = torch.zeros(4, 3, dtype=torch.float32)
    with poisoned(ONE, "cpu") as p:
        a = torch.empty_like(src)
        b = src.new_empty((2, 5))
        c = src.new_empty(0)
        d = src.new_empty(6, dtype=torch.int32)
        e = torch.empty_like(src, dtype=torch.int32)
        f = torch.empty(3, requires_grad=True)
        assert len(p.allocations) == 6
    assert a.shape == (4, 3) and a.dtype == torch.float32 and bool((a == 1.0).all())
    assert b.shape == (2, 5) and bool((b == 1.0).all()) and c.shape == (0,)
    assert d.dtype == torch.int32 and bool((d == ONE).all()) and e.shape == (4, 3) and bool((e == ONE).all())
    assert f.requires_grad and f.is_leaf and not a.requires_grad


def test_what_is_not_a_plain_allocation_on_the_device_goes_to_the_real_function():
    src = torch.zeros(2, 3, 4, 5)
    strided = torch.zeros(6, 4).t()
    out = torch.zeros(3)
    with poisoned(SENTINEL, "cpu") as on_cpu:
        assert torch.empty(3, out=out) is out                                                   # out=
        torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)                            # a non-contiguous memory format
        assert torch.empty_like(src, memory_format=torch.channels_last).is_contiguous(memory_format=torch.channels_last)
        assert torch.empty_like(strided).stride() == strided.stride()                           # preserve_format of a strided source
        assert torch.empty((3, 3), layout=torch.sparse_coo).layout is torch.sparse_coo          # a non-strided layout
        assert torch.empty(3, device="meta").device.type == "meta"                              # another device
        assert src.new_empty(3, device="meta").device.type == "meta"
        assert len(on_cpu.allocations) == 0
    with poisoned(SENTINEL, "cuda") as on_gpu:                                                  # cpu IS the other device here
        t = torch.empty(5)
        torch.empty_like(src)
        src.new_empty(4)
        assert t.shape == (5,) and len(on_gpu.allocations) == 0
    if torch.cuda.is_available():
        with poisoned(SENTINEL, "cpu") as p:
            assert torch.empty(3, pin_memory=True).is_pinned() and len(p.allocations) == 0     # pinned memory


def test_the_three_names_are_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(KeyError):
        with poisoned(ONE, "cpu"):
            assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with poisoned(ONE, "cpu"):
        pass
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before


def test_check_guards_passes_on_untouched_guards_and_names_the_allocation_that_was_overrun():
    with poisoned(SENTINEL, "cpu") as p:
        a, b, c = torch.empty(5), torch.empty(7, dtype=torch.uint8), torch.empty((2, 2))
        a.zero_(); b.zero_(); c.zero_()          # writing the tensors themselves, every byte, is fine
        p.check_guards()
        raw, nbytes = p.allocations[1]
        assert nbytes == 7
        raw[pz.GUARD + 8] ^= 1                   # the first byte of the back guard (7 bytes round up to 8)
        with pytest.raises(AssertionError, match=r"allocation #1 of 3 \(7 bytes\): back guard"):
            p.check_guards()
        raw[pz.GUARD + 8] ^= 1
        p.check_guards()
        raw[pz.GUARD - 1] ^= 0x80                # the last byte of the front guard
        with pytest.raises(AssertionError, match=r"allocation #1 of 3 \(7 bytes\): front guard overwritten, first at word 1023"):
            p.check_guards()
        raw[pz.GUARD - 1] ^= 0x80
        raw2, _ = p.allocations[2]
        raw2[0] = 9
        raw2[-1] = 9
        with pytest.raises(AssertionError, match=r"allocation #2 of 3 \(16 bytes\): front guard overwritten, first at word 0"):
            p.check_guards()
        raw2[0:4] = torch.from_numpy(_pattern_bytes(SENTINEL, 4).copy())
        with pytest.raises(AssertionError, match=r"allocation #2 of 3 \(16 bytes\): back guard overwritten, first at word 1023"):
            p.check_guards()
        raw2[-4:] = torch.from_numpy(_pattern_bytes(SENTINEL, 4).copy())


def test_the_block_checks_the_guards_on_exit():
    with pytest.raises(AssertionError, match="back guard"):
        with poisoned(ZERO, "cpu") as p:
            torch.empty(4)
            p.allocations[0][0][-1] = 1


def test_assert_identical_compares_bits_and_names_the_leaf():
    nan = torch.tensor([float("nan"), 1.0])
    runs = [("unpatched", {"a": nan.clone(), "n": [np.arange(3), None, 4]}), ("ZERO", {"a": nan.clone(), "n": [np.arange(3), None, 4]})]
    pz.assert_identical(runs, "nan equals nan bit for bit")
    scalars = lambda v: {"loss": torch.tensor(v), "step": torch.tensor(3, dtype=torch.int64), "none": torch.zeros(0, 3)}  # noqa: E731
    pz.assert_identical([("unpatched", scalars(0.25)), ("ONE", scalars(0.25))], "0-dim and empty tensors")
    with pytest.raises(AssertionError, match="loss differs"):
        pz.assert_identical([("unpatched", scalars(0.25)), ("ONE", scalars(0.5))], "0-dim tensors")
    runs.append(("ONE", {"a": torch.tensor([float("nan"), -0.0]), "n": [np.arange(3), None, 4]}))
    runs[0][1]["a"][1] = 0.0
    runs[1][1]["a"][1] = 0.0
    with pytest.raises(AssertionError, match="a differs between unpatched and ONE: 1 of 2 elements, first at flat index 1"):
        pz.assert_identical(runs, "minus zero is not zero")


# ---- host-side product code under the three patterns ------------------------------------------------------------------------------------
def test_host_prune_functions_do_not_depend_on_what_empty_memory_held():
    """prune.prune_mask and calculate_v_imp_score on CPU tensors (their torch path): unpatched against the three patterns, bit for bit.
    (loss_utils has no CPU path: l1_dssim_loss refuses CPU tensors, which test_refusals_host / test_lazy_loss pin.)"""
    from common import syn
    from lightgaussian_amd import prune
    g = syn.make_gaussians(257, seed=3)
    imp = torch.rand(257, generator=torch.Generator().manual_seed(1))
    imp[::7] = 0.0
    imp[5::11] = imp[4]                      # ties

    def run():
        v = prune.calculate_v_imp_score(g, imp, 0.1)
        return {"v": v, "mask": prune.prune_mask(0.66, v), "mask_imp": prune.prune_mask(0.3, imp)}

    runs = [("unpatched", run())]
    for name, word in pz.PATTERNS:
        with poisoned(word, "cpu"):
            runs.append((name, run()))
    pz.assert_identical(runs, "host prune")
    assert 0 < int(runs[0][1]["mask"].sum()) < 257
