"""-m gpu: K4 on its own (lg_debug_sort_keys: stand-alone histogram + hand-written onesweep passes) against torch's stable
sort of the same bit field; the K2/K3 kernels are covered through the rasterizer's bit-exact parity tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from lightgaussian_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sort(keys, begin, end):
    lib = _lib.load()
    n = keys.shape[0]
    out = torch.empty_like(keys)
    temp = torch.empty(max(lib.lg_debug_sort_temp_bytes(n), 1), dtype=torch.uint8, device=keys.device)
    _lib.check(lib.lg_debug_sort_keys(n, keys.data_ptr(), out.data_ptr(), begin, end, temp.data_ptr(),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def _field(keys, begin, end):
    return (keys >> begin) & ((1 << (end - begin)) - 1)


@pytest.mark.parametrize("n,begin,end,seed", [(1, 0, 8, 0), (63, 3, 11, 1), (8192, 0, 32, 2), (8193, 22, 54, 3), (100_000, 22, 61, 4),
                                              (1_000_003, 29, 61, 5), (4_141_089, 29, 61, 6), (300_000, 0, 5, 7), (70_000, 10, 23, 8)])
def test_stable_sort_of_a_bit_field(n, begin, end, seed):
    g = torch.Generator().manual_seed(seed)
    keys = torch.randint(0, 2 ** 62, (n,), generator=g, dtype=torch.int64).to(DEV)
    out = _sort(keys, begin, end)
    f_in = _field(keys, begin, end)
    order = torch.sort(f_in, stable=True).indices
    assert torch.equal(out, keys[order]), "not the stable order of the sorted field"
    assert torch.equal(keys, keys.clone())                          # input preserved (checked below against a copy)


def test_skewed_digits_and_input_preserved():
    g = torch.Generator().manual_seed(11)
    n = 500_000
    # tile-like top field with few distinct values, depth-like middle field, id in the low bits: the rasterizer's key shape
    tile = torch.randint(0, 37, (n,), generator=g, dtype=torch.int64)
    depth = (torch.rand(n, generator=g) ** 3 * (2 ** 19 - 1)).long()
    keys = ((tile << 41) | (depth << 22) | torch.arange(n)).to(DEV)
    copy = keys.clone()
    out = _sort(keys, 22, 47)
    assert torch.equal(keys, copy)
    assert torch.equal(out, torch.sort(keys).values)               # ids unique and ascending => the stable order is the full order
    # all keys equal in the sorted field: the sort must be the identity
    same = (torch.full((n,), 5, dtype=torch.int64) << 30 | torch.arange(n)).to(DEV)
    assert torch.equal(_sort(same, 30, 40), same)


def test_back_to_back_sorts_on_one_stream_and_bad_arguments():
    g = torch.Generator().manual_seed(12)
    keys = torch.randint(0, 2 ** 40, (200_000,), generator=g, dtype=torch.int64).to(DEV)
    a = _sort(keys, 0, 40)
    b = _sort(a, 0, 40)
    assert torch.equal(a, torch.sort(keys).values) and torch.equal(a, b)
    lib = _lib.load()
    assert lib.lg_debug_sort_keys(10, keys.data_ptr(), a.data_ptr(), 5, 5, keys.data_ptr(), None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_debug_sort_keys(0, None, None, 0, 8, None, None) == _lib.LG_OK


def test_a_look_back_that_gives_up_is_reported_not_passed_on():
    """r2 verdict / ADVICE: when a look-back exhausts its poll budget the pass used to continue with a wrong exclusive prefix -- a
    silently mis-sorted key array.  lg_debug_sort_orphan runs one digit pass whose only tile has a predecessor that never
    publishes (ticket preset to 1): the kernel must come back (no hang) with the error word set, surfaced as LG_ERR_DEVICE.
    (In a view the same bit lands in the abort word counters[0]: lg_tile_ranges and the blend kernels leave the view empty and
    LG_FLAG_DEBUG / lg_view_status() report it.)"""
    lib = _lib.load()
    n = 5000
    keys = torch.randint(0, 2 ** 40, (n,), generator=torch.Generator().manual_seed(3), dtype=torch.int64).to(DEV)
    pad = torch.zeros(8192 + n, dtype=torch.int64, device=DEV)       # the pass addresses its tile as tile 1: room below the keys
    pad[8192:] = keys
    out = torch.zeros_like(pad)
    temp = torch.empty(lib.lg_debug_sort_temp_bytes(2 * 8192), dtype=torch.uint8, device=DEV)
    rc = lib.lg_debug_sort_orphan(n, pad[8192:].data_ptr(), out[8192:].data_ptr(), temp.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.LG_ERR_DEVICE and b"look-back gave up" in lib.lg_last_error()
    torch.cuda.synchronize()
    # and the healthy path still reports success on the same buffers
    good = _sort(keys, 0, 40)
    assert torch.equal(good, torch.sort(keys).values)


def test_view_status_reads_the_abort_word_of_a_healthy_view():
    import math
    from lightgaussian_amd import synthetic as syn
    from lightgaussian_amd.gaussian_renderer import render
    dev = torch.device(DEV)
    pc = syn.make_gaussians(20000, seed=3, log_scale_mean=math.log(0.02)).to(dev).requires_grad_(True)
    cam = syn.orbit_camera(0, 8, 320, 200).to(dev)
    img = render(cam, pc, syn.PipelineParams(), torch.zeros(3, device=dev))["render"]
    geom = img.grad_fn.saved_tensors[-3]
    words = (C.c_uint32 * 4)()
    lib = _lib.load()
    _lib.check(lib.lg_view_status(geom.data_ptr(), 20000, C.byref(words), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert words[0] == 0 and words[3] > 0 and words[3] == _lib.last_stats()["num_rendered"]


# ---- second stage of the view's sort: every tile's list ordered by depth inside LDS (lg_tile_sort / _long) ----
def _tile_lists(image, W, H):
    """(ranges [tiles, 2], entries [R] uint64) of the view that produced `image`, from the binning buffer its forward saved."""
    from lightgaussian_amd import rasterizer
    fn = image.grad_fn
    *_, radii, geom, binning, img = fn.saved_tensors
    call = rasterizer._Call(fn.raster_settings, fn.saved_tensors[0], None, None, None, None, None, None, exact=False, opts=fn.opts)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    R = int(fn.num_rendered)
    ranges = torch.empty(T * 2, dtype=torch.int32, device=image.device)
    entries = torch.empty(max(R, 1), dtype=torch.int64, device=image.device)
    _lib.check(_lib.load().lg_debug_tile_lists(C.byref(call.view), binning.data_ptr(), R, ranges.data_ptr(), entries.data_ptr(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    ranges = ranges.cpu().numpy().reshape(T, 2).astype(np.int64)
    return ranges, entries.cpu().numpy().view(np.uint64)[: int(ranges[:, 1].max())]


def test_two_stage_sort_gives_the_lists_of_the_one_stage_sort_in_every_length_class():
    """Default: radix passes on the tile bits + one LDS counting sort per tile (a wave for lists up to 1024 entries, a workgroup up
    to 4096, the chunked 1024-thread kernel beyond).  option sort_all_bits: every bit through the global radix passes (round 2).
    Both must leave the same lists, entry for entry, and every list strictly ascending in (depth, id)."""
    import os
    from lightgaussian_amd import synthetic as syn
    from lightgaussian_amd.gaussian_renderer import render
    dev = torch.device(DEV)
    W, H = 640, 368
    g = syn.make_gaussians(300_000, seed=12)
    syn.make_heavy_tailed(g, frac=0.1)
    pc = g.to(dev).requires_grad_(True)
    cam = syn.orbit_camera(1, 10, W, H).to(dev)
    lists = {}
    from lightgaussian_amd import rasterizer
    for mode in ("two_stage", "one_stage"):
        with rasterizer.options(sort_all_bits=mode == "one_stage"):
            pkg = render(cam, pc, syn.PipelineParams(), torch.zeros(3, device=dev))
            lists[mode] = _tile_lists(pkg["render"], W, H) + (pkg["render"].detach().cpu().numpy(),)
    (ra, ea, ia), (rb, eb, ib) = lists["two_stage"], lists["one_stage"]
    n = ra[:, 1] - ra[:, 0]
    assert ((n > 1) & (n <= 1024)).any() and ((n > 1024) & (n <= 4096)).any() and (n > 4096).any(), (int(n.max()), np.percentile(n, [50, 90, 99]))
    assert np.array_equal(ra, rb)
    # (the two renders may lay their keys out differently -- the exact forward sizes the depth field from the view's own depth
    #  maximum, the bounded one from the caller's bound -- so the lists are compared by Gaussian id, the low bits_for(N) key bits)
    idm = np.uint64((1 << (g.num - 1).bit_length()) - 1)
    assert ea.shape == eb.shape and np.array_equal(ea & idm, eb & idm), f"{int(((ea & idm) != (eb & idm)).sum())} of {ea.size} entries differ"
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
    # the key is tile | depth | id with nothing dropped at this size, so the u64 order IS (tile, depth, id): the whole array ascends
    assert (ea[1:] > ea[:-1]).all() and (eb[1:] > eb[:-1]).all()
