"""The block-sparse TSDF volume, host side (no GPU): lg_math.h's block arithmetic through the g++ harness against the float64 twin of the
touch rule and against the dense harness of tests/mesh_common.py, the torch backend against the harness, closed surfaces across block
borders, the header against the binding and the compiler, the refusals of include/lightgaussian_blocks.h (they precede every device
call), and the Python surface of lightgaussian_amd.blocks."""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import blocks_common as bc
import mesh_common as mc
import test_abi
import tolerance
from common import ROOT, syn
from lightgaussian_amd import _lib, blocks, mesh

BLOCKS = (49, 151)                  # blocks the six views touch, per input set
BAND_BLOCKS = (30, 106)             # blocks that hold band points (weight > 0, tsdf < 1)
BAND_POINTS = 3745                  # ... and the band points of the first set


def _torch_views(views, color=True, alpha=False, **kw):
    return [dict(depth=torch.from_numpy(v["depth"]), camera=v["cam"], color=torch.from_numpy(v["color"]) if color else None,
                 alpha=torch.from_numpy(v["alpha"]) if alpha else None, **kw) for v in views]


def _cpu_volume(origin, voxel, trunc, color=True):
    return blocks.BlockTSDFVolume(voxel, origin=origin, trunc=trunc, color=color, device="cpu")


# ---- allocation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", (0, 1))
def test_touch_rule_against_float64_sandwich(which):
    origin, voxel, trunc, views = bc.input_set(which)
    keys, skipped, pix = bc.harness_touch(origin, voxel, trunc, views, pixels=True)
    tw = bc.twin_touch(origin, voxel, trunc, views)
    share = float(tw["near"].mean())
    print(f"set {which}: {len(keys)} blocks, {100 * share:.4f} % of the pixels within {bc.NEAR} voxel of a block face, largest range {pix[pix[:, 0] == 1][:, 4:].max()}")
    assert share <= mc.MAX_LEFT_OUT and skipped == 0 and not tw["skipped"].any()
    assert len(keys) == BLOCKS[which] and np.all(np.diff(keys) > 0)
    inner = bc.twin_keys(tw, ~tw["near"])
    grown = bc.twin_touch(origin, voxel, trunc, views, grow=bc.NEAR)
    outer = bc.twin_keys(grown, np.ones_like(grown["near"]))
    assert np.isin(inner, keys).all(), "the float32 set misses a block of the twin's pixels away from block faces"
    assert np.isin(keys, outer).all(), "the float32 set holds a block outside the twin's enlarged boxes"
    if which == 0:
        c = bc.coords_of(keys)
        assert c.min() == -1 and c.max() == 2 and pix[pix[:, 0] == 1][:, 4:].max() == 3
    # with an alpha map and a depth_max fewer pixels take part: a subset, and the twin agrees
    k2, s2 = bc.harness_touch(origin, voxel, trunc, views, use_alpha=True, depth_max=3.6)
    tw2 = bc.twin_touch(origin, voxel, trunc, views, use_alpha=True, depth_max=3.6)
    assert s2 == 0 and np.isin(k2, keys).all() and tw2["take"].sum() < tw["take"].sum() and np.isin(bc.twin_keys(tw2, ~tw2["near"]), k2).all()


@pytest.mark.parametrize("which", (0, 1))
def test_every_band_point_lies_in_a_touched_block(which):
    origin, voxel, trunc, views = bc.input_set(which)
    keys, skipped = bc.harness_touch(origin, voxel, trunc, views)
    base, dims = bc.dense_box(keys, margin_blocks=1)
    (f, w, _c), decided, _near = mc.twin_integrate(dims, bc.lattice_origin(origin, voxel, base), voxel, trunc, mc.fresh_volume(dims, color=False), views)
    band = np.flatnonzero((w.reshape(-1) > 0) & (f.reshape(-1) < 1))
    where = bc.sparse_rank_of(keys, band, dims, base)
    held = np.unique(where[where >= 0] // 512)
    print(f"set {which}: {len(band)} band points in {len(held)} of {len(keys)} blocks; {int((where < 0).sum())} outside")
    assert skipped == 0 and len(band) > 1000 and (where >= 0).all(), "a point the integration moves into the band lies in no touched block"
    assert len(held) == BAND_BLOCKS[which] and (which == 1 or len(band) == BAND_POINTS)


def test_skipped_pixels_and_refusals():
    cam = syn.orbit_camera(0, 6, 1, 1, radius=4.0)
    import math
    view = dict(cam=cam, W=1, H=1, tanfov=(math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)), vm=np.ascontiguousarray(cam.world_view_transform.numpy(), np.float32).reshape(16),
                depth=np.full((1, 1), 50.0, np.float32))
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    keys, skipped, pix = bc.harness_touch(origin, voxel, trunc, [view], pixels=True)
    assert len(keys) == 0 and skipped == 1 and pix[0, 0] == 2, "a 1 x 1 map at distance 50 spans more than 4 blocks"
    # lattice indices beyond +-2^23: the same pixel at a voxel size of 1e-6
    keys, skipped, pix = bc.harness_touch(origin, 1e-6, 4e-6, [dict(view, depth=np.full((1, 1), 20.0, np.float32))], pixels=True)
    assert len(keys) == 0 and skipped == 1 and pix[0, 0] == 2
    # a depth of 0, an infinite one and a NaN take no part and are not counted
    for d in (0.0, np.inf, np.nan, -1.0):
        keys, skipped, pix = bc.harness_touch(origin, voxel, trunc, [dict(view, depth=np.full((1, 1), d, np.float32))], pixels=True)
        assert len(keys) == 0 and skipped == 0 and pix[0, 0] == 0
    vol = _cpu_volume(origin, voxel, trunc, color=False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = vol.allocate([dict(depth=torch.full((1, 1), 50.0), camera=cam)])
        again = vol.allocate([dict(depth=torch.full((1, 1), 50.0), camera=cam)])
    assert out == dict(blocks=0, new_blocks=0, skipped_pixels=1) and again["skipped_pixels"] == 1 and vol.n_blocks == 0
    assert len([w for w in seen if "skipped" in str(w.message)]) == 1, "one warning per volume"
    with pytest.raises(ValueError, match="trunc"):
        blocks.BlockTSDFVolume(voxel, origin=origin, trunc=4.01 * voxel, device="cpu")


def test_allocation_order_and_regrid():
    origin, voxel, trunc, views = bc.input_set(0)
    tv = _torch_views(views)
    a, b = _cpu_volume(origin, voxel, trunc), _cpu_volume(origin, voxel, trunc)
    first = a.allocate(tv[:3])
    assert first["blocks"] == first["new_blocks"] == a.n_blocks > 0 and float(a.tsdf.min()) == 1 and float(a.weight.max()) == 0 and float(a.color.abs().max()) == 0
    a.allocate(tv[3:])
    b.allocate(tv[3:]); b.allocate(tv[:3])
    want, _s = bc.harness_touch(origin, voxel, trunc, views)
    assert np.array_equal(a.keys.numpy(), want) and np.array_equal(b.keys.numpy(), want)
    for x, y in ((a.tsdf, b.tsdf), (a.weight, b.weight), (a.color, b.color)):
        assert x.shape == y.shape and np.array_equal(bc.bits(x), bc.bits(y))
    # seeded values survive a regrid bit for bit; new blocks are fresh
    c = _cpu_volume(origin, voxel, trunc)
    c.allocate(tv[:2])
    g = torch.Generator().manual_seed(3)
    c.tsdf.copy_(torch.rand(c.tsdf.shape, generator=g) * 2 - 1); c.weight.copy_(torch.randint(0, 6, c.weight.shape, generator=g).float()); c.color.copy_(torch.rand(c.color.shape, generator=g))
    old_keys, old = c.keys.clone(), [t.clone() for t in (c.tsdf, c.weight, c.color)]
    out = c.allocate(tv[2:])
    assert out["new_blocks"] > 0 and out["blocks"] == len(want)
    at = torch.searchsorted(c.keys, old_keys)
    assert torch.equal(c.keys[at], old_keys)
    new = torch.ones(c.n_blocks, dtype=torch.bool); new[at] = False
    for t, o, fresh in zip((c.tsdf, c.weight, c.color), old, (1.0, 0.0, 0.0)):
        assert np.array_equal(bc.bits(t[at]), bc.bits(o)) and bool((t[new] == fresh).all())
    # allocate_blocks: the same union, any order, duplicates allowed
    d, e = _cpu_volume(origin, voxel, trunc), _cpu_volume(origin, voxel, trunc)
    coords = torch.from_numpy(bc.coords_of(want))
    d.allocate_blocks(coords.flip(0)); d.allocate_blocks(coords[:5])
    e.allocate_blocks(coords[10:]); e.allocate_blocks(coords[:30].to(torch.int32))
    assert np.array_equal(d.keys.numpy(), want) and np.array_equal(e.keys.numpy(), want) and torch.equal(d.coords(), coords.to(torch.int32))
    assert d.allocate_blocks(torch.zeros((0, 3), dtype=torch.int64))["new_blocks"] == 0


# ---- integration --------------------------------------------------------------------------------------------------------------------
def _shifted_first_set():
    """The first input set under the origin of lattice point (-16, -16, -16): every index is >= 8, and a dense grid with the same origin
    has the global index as its index."""
    origin, voxel, trunc, views = bc.input_set(0)
    origin = bc.lattice_origin(origin, voxel, (-16, -16, -16))
    keys, skipped = bc.harness_touch(origin, voxel, trunc, views)
    c = bc.coords_of(keys)
    assert skipped == 0 and c.min() >= 1 and len(keys) >= 30
    dims = tuple(int(v) for v in (c.max(axis=0) + 1) * 8)
    return origin, voxel, trunc, views, keys, dims


@pytest.mark.parametrize("color,kw", ((True, dict()), (True, dict(use_alpha=True, depth_max=3.6)), (False, dict(use_alpha=True))))
def test_integrate_equals_the_dense_harness_bit_for_bit(color, kw):
    origin, voxel, trunc, views, keys, dims = _shifted_first_set()
    got = bc.harness_integrate(keys, origin, voxel, trunc, bc.fresh_pools(len(keys), color), views, **kw)
    want = mc.harness_integrate(dims, origin, voxel, trunc, mc.fresh_volume(dims, color), views, **kw)
    at = bc.block_index(keys, (0, 0, 0), dims)
    assert np.array_equal(bc.bits(got[0]), bc.bits(want[0].reshape(-1)[at])) and np.array_equal(bc.bits(got[1]), bc.bits(want[1].reshape(-1)[at]))
    assert (got[1] > 0).sum() > 1000
    if color:
        assert np.array_equal(bc.bits(got[2]), bc.bits(want[2].reshape(-1, 3)[at]))
    # nothing the dense volume moved into the band lies outside the blocks
    inside = np.zeros(want[0].size, bool); inside[at.reshape(-1)] = True
    assert not ((want[1].reshape(-1) > 0) & (want[0].reshape(-1) < 1) & ~inside).any()


def test_integrate_against_float64_under_negative_blocks():
    origin, voxel, trunc, views = bc.input_set(0)
    keys, _s = bc.harness_touch(origin, voxel, trunc, views)
    assert bc.coords_of(keys).min() < 0
    base, dims = bc.dense_box(keys)
    start = mc.fresh_volume(dims)
    got = bc.harness_integrate(keys, origin, voxel, trunc, bc.fresh_pools(len(keys)), views, use_alpha=True, depth_max=3.6)
    o = bc.lattice_origin(origin, voxel, base)
    r64, d64, near = mc.twin_integrate(dims, o, voxel, trunc, start, views, use_alpha=True, depth_max=3.6)
    r32, _d, _n = mc.twin_integrate(dims, o, voxel, trunc, start, views, use_alpha=True, depth_max=3.6, dtype=np.float32)
    at = bc.block_index(keys, base, dims).reshape(-1)
    keep = ~near.any(axis=0)[at]
    share = 1 - keep.mean()
    print(f"{100 * share:.3f} % of the points have a pair within {mc.MARGIN} of a decision; {100 * d64[:, at].mean():.1f} % of the pairs update")
    assert share <= mc.MAX_LEFT_OUT and d64[:, at].mean() > 0.03
    assert np.array_equal(got[1].reshape(-1)[keep], r64[1].reshape(-1)[at][keep]), "weights differ"
    tolerance.assert_rule3(got[0].reshape(-1)[keep], r64[0].reshape(-1)[at][keep], r32[0].reshape(-1)[at][keep], "tsdf")
    tolerance.assert_rule3(got[2].reshape(-1, 3)[keep], r64[2].reshape(-1, 3)[at][keep], r32[2].reshape(-1, 3)[at][keep], "colour")


def test_one_call_with_11_views_is_11_calls_in_the_harness():
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    views = mc.sphere_views(11, sizes=mc.IMAGES)
    keys, _s = bc.harness_touch(origin, voxel, trunc, views)
    rs = np.random.RandomState(5)
    n = len(keys)
    start = (rs.uniform(-1, 1, (n, 8, 8, 8)).astype(np.float32), rs.randint(0, 6, (n, 8, 8, 8)).astype(np.float32), rs.uniform(0, 1, (n, 8, 8, 8, 3)).astype(np.float32))
    once = bc.harness_integrate(keys, origin, voxel, trunc, start, views, use_alpha=True)
    state = start
    for v in views:
        state = bc.harness_integrate(keys, origin, voxel, trunc, state, [v], use_alpha=True)
    assert all(np.array_equal(bc.bits(a), bc.bits(b)) for a, b in zip(once, state)) and not np.array_equal(bc.bits(once[0]), bc.bits(start[0]))


# ---- extraction ---------------------------------------------------------------------------------------------------------------------
def test_extract_equals_the_dense_harness_as_a_set_and_in_the_contract_order():
    keys, f, w, c, dense = bc.scattered_field()
    assert 12 <= len(keys) <= 24, "about a third of the 27 blocks is missing"
    origin, voxel, _t = mc.volume_spec((32, 32, 32))
    got = bc.harness_extract(keys, f, w, c, origin, voxel)
    want = mc.harness_extract(dense[0], dense[1], dense[2], origin, voxel)
    assert (got["used"][:, 1:15] > 0).all(), "the field must meet all 6 x 14 non-trivial table entries"
    assert np.array_equal(got["used"], want["used"]) and len(got["faces"]) > 500
    perm = bc.match_meshes(got, want)
    # vertices by (block rank, point in block, slot): the dense vertices' owners, mapped into the blocks, ascend along the sparse ids
    p, k = bc.dense_vertex_owners(dense[0], dense[1])
    order = bc.sparse_rank_of(keys, p, (32, 32, 32)) * 7 + k
    assert (order >= 0).all() and np.all(np.diff(order[perm]) > 0), "vertex ids do not count (block rank, point, slot)"
    # faces by (block rank, cell, tetrahedron, triangle): the dense faces, stably sorted by their cell's place in the blocks, ARE the sparse faces
    cell = bc.sparse_rank_of(keys, want["cell_of_face"], (32, 32, 32))
    by_cell = np.argsort(cell, kind="stable")
    assert (cell >= 0).all() and np.array_equal(cell[by_cell], got["cell_of_face"])
    assert np.array_equal(perm[got["faces"].astype(np.int64)], want["faces"][by_cell].astype(np.int64))
    # another iso and min_weight
    g2, w2 = bc.harness_extract(keys, f, w, c, origin, voxel, 0.25, 2.0), mc.harness_extract(dense[0], dense[1], dense[2], origin, voxel, 0.25, 2.0)
    bc.match_meshes(g2, w2)


def test_one_block_and_no_block():
    f, w, c = mc.random_field((8, 8, 8), seed=2, observed=0.93)
    origin, voxel, _t = mc.volume_spec((8, 8, 8))
    keys = bc.keys_of([[-3, 0, 5]])
    got = bc.harness_extract(keys, f[None], w[None], c[None], origin, voxel)
    o = bc.lattice_origin(origin, voxel, (-24, 0, 40))
    want = mc.harness_extract(f, w, c, o, voxel)
    assert np.array_equal(got["nbr"], [[0, -1, -1, -1, -1, -1, -1, -1]])
    assert np.array_equal(got["faces"], want["faces"]) and len(got["faces"]) > 50 and got["vertices"].shape == want["vertices"].shape
    assert np.abs(got["vertices"] - want["vertices"]).max() <= 1e-5, "an isolated block is the dense 8 x 8 x 8 grid at its place"
    assert np.array_equal(bc.bits(got["colors"]), bc.bits(want["colors"]))
    none = bc.harness_extract(np.zeros(0, np.int64), np.zeros((0, 8, 8, 8), np.float32), np.zeros((0, 8, 8, 8), np.float32), None, origin, voxel)
    assert none["vertices"].shape == (0, 3) and none["faces"].shape == (0, 3)
    vol = _cpu_volume(origin, voxel, 4 * voxel)
    v, fc, col = vol.extract_mesh()
    assert v.shape == (0, 3) and fc.shape == (0, 3) and fc.dtype == torch.int32 and col.shape == (0, 3)


def _surfaces():
    dims = (12, 12, 12)
    _o, voxel, _t = mc.volume_spec(dims)
    yield "sphere", voxel, (lambda p: np.linalg.norm(p, axis=-1) - 1.0), 4 / 3 * np.pi, 2
    dims = (24, 12, 24)
    _o, voxel, _t = mc.volume_spec(dims)
    yield "torus", voxel, (lambda p: np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 2] ** 2) - 0.9) ** 2 + p[..., 1] ** 2) - 0.35), 2 * np.pi ** 2 * 0.9 * 0.35 ** 2, 0


@pytest.mark.parametrize("which", ("harness", "torch"))
def test_closed_surfaces_across_block_borders(which):
    for name, voxel, dist, volume, euler in _surfaces():
        origin = (0.0123456, -0.0071234, 0.0049871)
        trunc = 4 * voxel
        # the blocks that hold a point within trunc of the surface, found on a generous box of blocks
        n = int(np.ceil(1.6 / (8 * voxel))) + 1
        vol = _cpu_volume(origin, voxel, trunc, color=False)
        vol.allocate_blocks(torch.tensor([(x, y, z) for z in range(-n, n) for y in range(-n, n) for x in range(-n, n)]))
        d = dist(vol.points().double().numpy())
        near = np.abs(d).reshape(vol.n_blocks, -1).min(axis=1) < vol.trunc
        small = _cpu_volume(origin, voxel, trunc, color=False)
        small.allocate_blocks(vol.coords()[torch.from_numpy(near)])
        assert 8 <= small.n_blocks < vol.n_blocks and int(small.coords().min()) < 0
        d = dist(small.points().double().numpy())
        small.tsdf.copy_(torch.from_numpy(np.clip(d / small.trunc, -1, 1).astype(np.float32)))
        small.weight.fill_(1.0)
        if which == "harness":
            m = bc.harness_extract(small.keys.numpy(), small.tsdf.numpy(), small.weight.numpy(), None, small.origin, small.voxel_size)
            v, faces = m["vertices"], m["faces"]
        else:
            v, faces, _c = (None if t is None else t.numpy() for t in small.extract_mesh(drop_unreferenced=False))
        p = mc.mesh_properties(v, faces)
        print(f"{which} {name}: {small.n_blocks} blocks, {len(v)} vertices, {len(faces)} faces, V - E + F = {p['euler']}, volume {p['volume']:.4f} (analytic {volume:.4f})")
        assert p["closed"], f"{name}: an edge is not used once in each direction"
        assert p["euler"] == euler and p["volume"] > 0 and abs(p["volume"] / volume - 1) <= 0.08
        assert len(np.unique(faces)) == len(v), "a closed surface has no unreferenced vertex"


# ---- the torch backend ------------------------------------------------------------------------------------------------------------------
def test_torch_backend_equals_the_harness():
    origin, voxel, trunc, views = bc.input_set(0)
    want_keys, _s = bc.harness_touch(origin, voxel, trunc, views, use_alpha=True, depth_max=3.6)
    want = bc.harness_integrate(want_keys, origin, voxel, trunc, bc.fresh_pools(len(want_keys)), views, use_alpha=True, depth_max=3.6)
    vol = _cpu_volume(origin, voxel, trunc)
    assert vol.trunc == trunc and vol.voxel_size == voxel and vol.origin == tuple(origin)
    vol.integrate_many(_torch_views(views, alpha=True, alpha_min=0.5, depth_max=3.6))
    assert np.array_equal(vol.keys.numpy(), want_keys)
    for got, ref, name in ((vol.tsdf, want[0], "tsdf"), (vol.weight, want[1], "weight"), (vol.color, want[2], "colour")):
        bad = np.flatnonzero(bc.bits(got).reshape(-1) != bc.bits(ref).reshape(-1))
        assert bad.size == 0, f"{name} differs in {bad.size} words"
    h = bc.harness_extract(want_keys, *want, origin, voxel)
    v, f, c = vol.extract_mesh(drop_unreferenced=False)
    assert len(h["faces"]) > 500 and f.dtype == torch.int32 and np.array_equal(f.numpy(), h["faces"]), "faces or their order differ"
    assert np.array_equal(bc.bits(v), bc.bits(h["vertices"])) and np.array_equal(bc.bits(c), bc.bits(h["colors"]))
    # the scattered field: same mesh, same order
    keys, ft, wt, ct, _dense = bc.scattered_field()
    o, vx, _t = mc.volume_spec((32, 32, 32))
    sv = _cpu_volume(o, vx, 4 * vx)
    sv.allocate_blocks(torch.from_numpy(bc.coords_of(keys)))
    sv.tsdf.copy_(torch.from_numpy(ft)); sv.weight.copy_(torch.from_numpy(wt)); sv.color.copy_(torch.from_numpy(ct))
    h = bc.harness_extract(keys, ft, wt, ct, sv.origin, sv.voxel_size)
    v, f, c = sv.extract_mesh(drop_unreferenced=False)
    assert np.array_equal(f.numpy(), h["faces"]) and np.array_equal(bc.bits(v), bc.bits(h["vertices"])) and np.array_equal(bc.bits(c), bc.bits(h["colors"]))
    # points(): the dense expression with the global index
    pts = sv.points().numpy()
    g = bc.coords_of(keys)[:, :, None] * 8 + np.arange(8)
    assert np.array_equal(pts[:, 0, 0, :, 0], np.float32(o[0]) + np.float32(vx) * g[:, 0].astype(np.float32))
    assert np.array_equal(pts[:, :, 0, 0, 2], np.float32(o[2]) + np.float32(vx) * g[:, 2].astype(np.float32))


def test_end_to_end_on_the_cpu_path_and_to_dense():
    origin, voxel, trunc, views = bc.input_set(0)
    vol = _cpu_volume(origin, voxel, trunc)
    vol.integrate_many(_torch_views(views))
    assert vol.n_blocks == BLOCKS[0] and vol.nbytes() == vol.n_blocks * (8 + 512 * 4 * 5)
    v, f, c = vol.extract_mesh()
    err = np.abs(np.linalg.norm(v.numpy(), axis=1) - 1) / voxel
    print(f"{vol.n_blocks} blocks, {len(v)} vertices, {len(f)} faces: | |v| - 1 | mean {err.mean():.3f}, max {err.max():.3f} voxels")
    assert len(f) > 1000 and err.mean() < 0.5 and c.shape == v.shape and float(c.min()) >= 0 and float(c.max()) <= 1
    assert mc.mesh_properties(v.numpy(), f.numpy())["volume"] > 0
    # to_dense: the blocks' values at their places, fresh values elsewhere, and back
    for margin in (0, 3):
        dense = vol.to_dense(margin=margin)
        base, dims = bc.dense_box(vol.keys.numpy())
        assert dense.dims == tuple(d + 2 * margin for d in dims) and dense.trunc == vol.trunc and dense.voxel_size == vol.voxel_size
        at = torch.from_numpy(bc.block_index(vol.keys.numpy(), base - margin, dense.dims))
        for d, s in ((dense.tsdf, vol.tsdf), (dense.weight, vol.weight)):
            assert np.array_equal(bc.bits(d.reshape(-1)[at]), bc.bits(s))
        assert np.array_equal(bc.bits(dense.color.reshape(-1, 3)[at]), bc.bits(vol.color))
        outside = torch.ones(dense.tsdf.numel(), dtype=torch.bool); outside[at.reshape(-1)] = False
        assert bool((dense.tsdf.reshape(-1)[outside] == 1).all()) and bool((dense.weight.reshape(-1)[outside] == 0).all())
        dv, df, _dc = dense.extract_mesh()
        # the dense copy meshes to the same surface (in the dense order, and its coordinates may differ in the last bit)
        assert df.shape == f.shape and dv.shape == v.shape and np.abs(np.sort(dv.numpy().sum(axis=1)) - np.sort(v.numpy().sum(axis=1))).max() <= 1e-5
        assert abs(mc.mesh_properties(dv.numpy(), df.numpy())["volume"] - mc.mesh_properties(v.numpy(), f.numpy())["volume"]) <= 1e-5
    vol.reset()
    assert vol.n_blocks == BLOCKS[0] and float(vol.tsdf.min()) == 1 and float(vol.weight.max()) == 0 and float(vol.color.abs().max()) == 0
    vol.clear()
    assert vol.n_blocks == 0 and vol.tsdf.shape == (0, 8, 8, 8) and vol.color.shape == (0, 8, 8, 8, 3)
    # integrate with allocate=False leaves the block list alone
    vol.allocate(_torch_views(views[:1]))
    n = vol.n_blocks
    vol.integrate_many(_torch_views(views), allocate=False)
    assert vol.n_blocks == n and float(vol.weight.max()) > 0


# ---- the header, the binding and the compiler -----------------------------------------------------------------------------------------
def test_header_matches_binding():
    declared = test_abi.check_extension_header("lightgaussian_blocks.h", blocks.PROTOTYPES)
    assert len(declared) == 9 and declared["lg_blocks_mesh_scratch_bytes"] == ("size_t", ["int32"])
    assert declared["lg_blocks_touch"] == ("int32", ["pointer", "int32", "pointer", "int64", "pointer", "pointer", "pointer", "uint32", "pointer"])
    assert declared["lg_blocks_mesh_emit"] == ("int32", ["pointer", "float", "float", "pointer", "int64", "int64", "pointer", "pointer", "pointer", "uint32", "pointer"])
    text = open(os.path.join(ROOT, "include", "lightgaussian_blocks.h")).read()
    assert "LG_ABI_VERSION" not in text and '#include "lightgaussian_mesh.h"' in text
    assert len(mesh.PROTOTYPES) == 4 and not any(name in mesh.PROTOTYPES for name in blocks.PROTOTYPES)
    make = open(os.path.join(ROOT, "lightgaussian_amd", "csrc", "Makefile")).read()
    assert "lg_blocks.h" in make and "lightgaussian_blocks.h" in make
    math_h = open(os.path.join(ROOT, "lightgaussian_amd", "csrc", "lg_math.h")).read()
    assert blocks.BLOCK == int(re.search(r"#define LG_BLK (\d+)", math_h).group(1)) and blocks.MAX_SPAN == int(re.search(r"#define LG_BLK_MAX_SPAN (\d+)", math_h).group(1))


def test_struct_layout_against_the_compiler(tmp_path):
    text = test_abi._header_text((os.path.join(ROOT, "include", "lightgaussian_blocks.h"),))
    found = re.findall(r"typedef\s+struct\s+(lg_\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S)
    assert [name for name, _b in found] == ["lg_block_volume"]
    fields = [re.fullmatch(r".*?(\w+)\s*(?:\[\s*\d+\s*\])?", part.strip(), flags=re.S).group(1) for decl in found[0][1].split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [f[0] for f in blocks.lg_block_volume._fields_] == ["origin", "voxel_size", "trunc", "n_blocks", "keys", "tsdf", "weight", "color"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lightgaussian_blocks.h"', "int main(void) {", '    printf("sizeof %zu\\n", sizeof(lg_block_volume));']
    lines += [f'    printf("{f} %zu\\n", offsetof(lg_block_volume, {f}));' for f in fields] + ["    return 0;", "}"]
    src, exe = tmp_path / "blocks_layout.cpp", tmp_path / "blocks_layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    for what, value in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()):
        mine = C.sizeof(blocks.lg_block_volume) if what == "sizeof" else getattr(blocks.lg_block_volume, what).offset
        assert mine == int(value), f"lg_block_volume {what}: ctypes {mine}, the compiler {value}"
    assert C.sizeof(blocks.lg_block_volume) == 56 and not hasattr(_lib, "lg_block_volume") and not hasattr(mesh, "lg_block_volume")


# ---- refusals: before any device call, so they run without a device ---------------------------------------------------------------------
FAKE = 0x10000          # an address nobody dereferences: every call below is refused, or returns, before the first device call


def _volume(**kw):
    f = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, trunc=0.4, n_blocks=3, keys=FAKE, tsdf=FAKE + 4096, weight=FAKE + 8192, color=FAKE + 16384)
    f.update(kw)
    return blocks.lg_block_volume((C.c_float * 3)(*f["origin"]), f["voxel_size"], f["trunc"], f["n_blocks"], f["keys"], f["tsdf"], f["weight"], f["color"])


def _view(**kw):
    f = dict(W=33, H=17, tanfovx=0.5, tanfovy=0.3, viewmatrix=FAKE, depth=FAKE, color=FAKE, alpha=None, alpha_min=0.5, depth_max=0.0, z_min=0.05)
    f.update(kw)
    return mesh.lg_tsdf_view(*(f[n] for n, _t in mesh.lg_tsdf_view._fields_))


def test_refusals_of_the_library():
    lib = blocks.load()
    nan, inf = float("nan"), float("inf")
    sc = C.c_void_p(FAKE)

    def refused(rc, fn, *words):
        assert rc == _lib.LG_ERR_INVALID_ARGUMENT, (fn, words, rc)
        msg = lib.lg_last_error().decode()
        assert msg.startswith(fn + ":") and all(w in msg for w in words), msg

    one = (mesh.lg_tsdf_view * 1)(_view())
    volumes = [(dict(n_blocks=-1), "n_blocks"), (dict(n_blocks=1 << 20), "2^29"), (dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=nan), "voxel_size"),
               (dict(voxel_size=inf), "voxel_size"), (dict(trunc=0.0), "trunc"), (dict(trunc=-1.0), "trunc"), (dict(trunc=nan), "trunc"), (dict(trunc=0.41), "trunc"),
               (dict(origin=(0.0, nan, 0.0)), "origin"), (dict(origin=(inf, 0.0, 0.0)), "origin"), (dict(keys=None), "null keys"), (dict(keys=FAKE + 4), "keys must be 8-byte aligned"),
               (dict(tsdf=None), "null tsdf"), (dict(weight=None), "null weight"), (dict(tsdf=FAKE + 4), "tsdf must be 16-byte aligned"),
               (dict(weight=FAKE + 8), "weight must be 16-byte aligned"), (dict(color=FAKE + 4), "color must be 16-byte aligned")]
    for kw, word in volumes:
        v = _volume(**kw)
        refused(lib.lg_blocks_touch(C.byref(v), 1, one, 64, sc, sc, sc, 0, None), "lg_blocks_touch", word)
        refused(lib.lg_blocks_integrate(C.byref(v), 1, one, 0, None), "lg_blocks_integrate", word)
        refused(lib.lg_blocks_regrid(C.byref(v), C.byref(_volume()), 0, None), "lg_blocks_regrid", "from", word)
        refused(lib.lg_blocks_regrid(C.byref(_volume()), C.byref(v), 0, None), "lg_blocks_regrid", "to", word)
        refused(lib.lg_blocks_mesh_count(C.byref(v), 0.0, 1.0, sc, sc, 0, None), "lg_blocks_mesh_count", word)
        refused(lib.lg_blocks_mesh_emit(C.byref(v), 0.0, 1.0, sc, 3, 1, sc, None, sc, 0, None), "lg_blocks_mesh_emit", word)
    vol = _volume()
    for fn, call in (("lg_blocks_touch", lambda n, a: lib.lg_blocks_touch(C.byref(vol), n, a, 64, sc, sc, sc, 0, None)),
                     ("lg_blocks_integrate", lambda n, a: lib.lg_blocks_integrate(C.byref(vol), n, a, 0, None))):
        refused(call(-1, one), fn, "n_views < 0")
        refused(call(1, None), fn, "null views")
        views = [(dict(W=0), "W outside"), (dict(W=32769), "W outside"), (dict(H=0), "H outside"), (dict(H=32769), "H outside"), (dict(tanfovx=nan), "tanfovx is NaN"),
                 (dict(tanfovy=nan), "tanfovy is NaN"), (dict(z_min=nan), "NaN"), (dict(depth_max=nan), "NaN"), (dict(alpha_min=nan), "NaN"),
                 (dict(viewmatrix=None), "null viewmatrix"), (dict(depth=None), "null depth"), (dict(depth=FAKE + 2), "4-byte aligned"), (dict(alpha=FAKE + 1), "4-byte aligned")]
        for kw, word in views:
            refused(call(3, (mesh.lg_tsdf_view * 3)(_view(), _view(), _view(**kw))), fn, "views[2]", word)
    refused(lib.lg_blocks_integrate(C.byref(vol), 1, (mesh.lg_tsdf_view * 1)(_view(color=None)), 0, None), "lg_blocks_integrate", "views[0]", "null color")
    # a colour pointer the call does not read is not looked at, misaligned or not (lg_tsdf_integrate refuses it: tests/test_mesh_host.py).
    # lg_blocks_touch uses the same checker and never reads colour, but it launches even without blocks, so the verdict is seen here alone.
    odd = (mesh.lg_tsdf_view * 1)(_view(color=FAKE + 2))
    assert lib.lg_blocks_integrate(C.byref(_volume(color=None, n_blocks=0)), 1, odd, 0, None) == _lib.LG_OK
    refused(lib.lg_blocks_touch(None, 1, one, 64, sc, sc, sc, 0, None), "lg_blocks_touch", "null volume")
    refused(lib.lg_blocks_touch(C.byref(vol), 1, one, -1, sc, sc, sc, 0, None), "lg_blocks_touch", "capacity")
    refused(lib.lg_blocks_touch(C.byref(vol), 1, one, 64, None, sc, sc, 0, None), "lg_blocks_touch", "null candidates")
    refused(lib.lg_blocks_touch(C.byref(vol), 1, one, 64, C.c_void_p(FAKE + 4), sc, sc, 0, None), "lg_blocks_touch", "candidates must be 8-byte aligned")
    refused(lib.lg_blocks_touch(C.byref(vol), 1, one, 64, sc, None, sc, 0, None), "lg_blocks_touch", "null stats")
    refused(lib.lg_blocks_touch(C.byref(vol), 1, one, 64, sc, sc, None, 0, None), "lg_blocks_touch", "null scratch")
    refused(lib.lg_blocks_touch(C.byref(vol), 1, one, 64, sc, sc, C.c_void_p(FAKE + 16), 0, None), "lg_blocks_touch", "scratch must be 256-byte aligned")
    big = (mesh.lg_tsdf_view * 1)(_view(W=8192, H=8192))
    refused(lib.lg_blocks_touch(C.byref(vol), 1, big, 64, sc, sc, sc, 0, None), "lg_blocks_touch", "2^26 pixels")
    refused(lib.lg_blocks_merge(-1, sc, 1, sc, sc, sc, sc, 0, None), "lg_blocks_merge", "n_old")
    refused(lib.lg_blocks_merge(1 << 20, sc, 1, sc, sc, sc, sc, 0, None), "lg_blocks_merge", "n_old")
    refused(lib.lg_blocks_merge(1, sc, -1, sc, sc, sc, sc, 0, None), "lg_blocks_merge", "n_add")
    refused(lib.lg_blocks_merge(1, sc, 1 << 30, sc, sc, sc, sc, 0, None), "lg_blocks_merge", "2^30")
    refused(lib.lg_blocks_merge(1, None, 1, sc, sc, sc, sc, 0, None), "lg_blocks_merge", "null old_keys")
    refused(lib.lg_blocks_merge(1, sc, 1, None, sc, sc, sc, 0, None), "lg_blocks_merge", "null add_keys")
    refused(lib.lg_blocks_merge(1, sc, 1, sc, None, sc, sc, 0, None), "lg_blocks_merge", "null merged")
    refused(lib.lg_blocks_merge(1, sc, 1, sc, sc, None, sc, 0, None), "lg_blocks_merge", "null count")
    refused(lib.lg_blocks_merge(1, sc, 1, C.c_void_p(FAKE + 4), sc, sc, sc, 0, None), "lg_blocks_merge", "8-byte aligned")
    refused(lib.lg_blocks_merge(1, sc, 1, sc, sc, sc, None, 0, None), "lg_blocks_merge", "null scratch")
    refused(lib.lg_blocks_regrid(None, C.byref(vol), 0, None), "lg_blocks_regrid", "from", "null volume")
    refused(lib.lg_blocks_regrid(C.byref(vol), C.byref(_volume(color=None)), 0, None), "lg_blocks_regrid", "colour")
    for iso, mw, word in ((nan, 1.0, "iso"), (inf, 1.0, "iso"), (0.0, 0.0, "min_weight"), (0.0, -1.0, "min_weight"), (0.0, nan, "min_weight"), (0.0, inf, "min_weight")):
        refused(lib.lg_blocks_mesh_count(C.byref(vol), iso, mw, sc, sc, 0, None), "lg_blocks_mesh_count", word)
        refused(lib.lg_blocks_mesh_emit(C.byref(vol), iso, mw, sc, 3, 1, sc, None, sc, 0, None), "lg_blocks_mesh_emit", word)
    refused(lib.lg_blocks_mesh_count(C.byref(vol), 0.0, 1.0, None, sc, 0, None), "lg_blocks_mesh_count", "null scratch")
    refused(lib.lg_blocks_mesh_count(C.byref(vol), 0.0, 1.0, C.c_void_p(FAKE + 16), sc, 0, None), "lg_blocks_mesh_count", "scratch must be 256-byte aligned")
    refused(lib.lg_blocks_mesh_count(C.byref(vol), 0.0, 1.0, sc, None, 0, None), "lg_blocks_mesh_count", "null counts")
    refused(lib.lg_blocks_mesh_count(C.byref(vol), 0.0, 1.0, sc, C.c_void_p(FAKE + 4), 0, None), "lg_blocks_mesh_count", "counts must be 8-byte aligned")
    refused(lib.lg_blocks_mesh_emit(C.byref(vol), 0.0, 1.0, sc, -1, 1, sc, None, sc, 0, None), "lg_blocks_mesh_emit", "n_vertices outside")
    refused(lib.lg_blocks_mesh_emit(C.byref(vol), 0.0, 1.0, sc, 3, 1 << 31, sc, None, sc, 0, None), "lg_blocks_mesh_emit", "n_faces outside")
    refused(lib.lg_blocks_mesh_emit(C.byref(vol), 0.0, 1.0, sc, 3, 1, None, None, sc, 0, None), "lg_blocks_mesh_emit", "null vertices")
    refused(lib.lg_blocks_mesh_emit(C.byref(vol), 0.0, 1.0, sc, 3, 1, sc, None, None, 0, None), "lg_blocks_mesh_emit", "null faces")
    refused(lib.lg_blocks_mesh_emit(C.byref(vol), 0.0, 1.0, sc, 3, 1, sc, C.c_void_p(FAKE + 2), sc, 0, None), "lg_blocks_mesh_emit", "colors must be 4-byte aligned")
    refused(lib.lg_blocks_mesh_emit(C.byref(_volume(color=None)), 0.0, 1.0, sc, 3, 1, sc, sc, sc, 0, None), "lg_blocks_mesh_emit", "keeps no colour")
    # what returns LG_OK without a device call: no views or no blocks to integrate, nothing to regrid into; the widest band is accepted
    assert lib.lg_blocks_integrate(C.byref(vol), 0, None, 0, None) == _lib.LG_OK
    assert lib.lg_blocks_integrate(C.byref(_volume(n_blocks=0, keys=None, tsdf=None, weight=None, color=None)), 1, one, 0, None) == _lib.LG_OK
    assert lib.lg_blocks_regrid(C.byref(vol), C.byref(_volume(n_blocks=0, keys=None, tsdf=None, weight=None, color=None)), 0, None) == _lib.LG_OK
    assert lib.lg_blocks_integrate(C.byref(_volume(voxel_size=0.125, trunc=0.5)), 0, None, 0, None) == _lib.LG_OK
    assert lib.lg_blocks_mesh_scratch_bytes(-1) == 0 and lib.lg_blocks_mesh_scratch_bytes(1 << 20) == 0 and lib.lg_blocks_merge_scratch_bytes(-1) == 0
    assert lib.lg_blocks_mesh_scratch_bytes(3) >= 3 * (512 * 10 + 32 + 8) + 16 and lib.lg_blocks_mesh_scratch_bytes(3) % 256 == 0 and lib.lg_blocks_mesh_scratch_bytes(0) > 0
    assert lib.lg_blocks_touch_scratch_bytes(1, one) >= 8 * 5 * 3 and lib.lg_blocks_touch_scratch_bytes(1, (mesh.lg_tsdf_view * 1)(_view(W=0))) == 0
    assert lib.lg_blocks_merge_scratch_bytes(1000) >= 2 * 8000 and lib.lg_blocks_merge_scratch_bytes(1 << 30) == 0


def test_refusals_of_the_python_surface():
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    cam = syn.orbit_camera(0, 6, 6, 5, radius=4.0)
    depth, color, alpha = torch.rand(5, 6) + 3.0, torch.rand(3, 5, 6), torch.rand(5, 6)
    vol = _cpu_volume(origin, voxel, trunc)
    plain = _cpu_volume(origin, voxel, trunc, color=False)
    plain.integrate(depth, cam)                          # no colour kept: none asked
    plain.integrate(depth, cam, color=color)             # ... and one given is ignored
    assert plain.n_blocks > 0 and plain.color is None
    B = blocks.BlockTSDFVolume
    bad = [lambda: B(0.0, device="cpu"), lambda: B(float("nan"), device="cpu"), lambda: B(voxel, trunc=0.0, device="cpu"), lambda: B(voxel, trunc=5 * voxel, device="cpu"),
           lambda: B(voxel, trunc=float("nan"), device="cpu"), lambda: B(voxel, origin=(0.0, 0.0), device="cpu"), lambda: B(voxel, origin=(0.0, float("inf"), 0.0), device="cpu"),
           lambda: B(voxel, device="cpu", backend="triton"),
           lambda: vol.integrate(depth, cam), lambda: vol.integrate(depth.double(), cam, color=color), lambda: vol.integrate(depth[None], cam, color=color),
           lambda: vol.integrate(depth, cam, color=color[:2]), lambda: vol.integrate(depth, cam, color=color, alpha=alpha[:4]),
           lambda: vol.integrate(depth.numpy(), cam, color=color), lambda: vol.integrate(depth, cam, color=color, z_min=float("nan")),
           lambda: vol.integrate(depth.to("meta"), cam, color=color), lambda: vol.integrate_many([dict(depth=depth, camera=cam, color=color, colour=1)]),
           lambda: vol.allocate([dict(depth=depth[None], camera=cam)]), lambda: vol.allocate_blocks(torch.zeros((2, 2), dtype=torch.int64)),
           lambda: vol.allocate_blocks(torch.zeros((2, 3))), lambda: vol.allocate_blocks(torch.tensor([[0, 0, 1 << 20]])), lambda: vol.allocate_blocks(torch.tensor([[-(1 << 20) - 1, 0, 0]])),
           lambda: vol.extract_mesh(min_weight=0.0), lambda: vol.extract_mesh(iso=float("inf")), lambda: vol.to_dense(), lambda: vol.to_dense(margin=-1)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")
    vol.integrate_many([])                               # no view: nothing happens
    assert vol.n_blocks == 0
    vol.allocate_blocks(torch.tensor([[-(1 << 20), 0, (1 << 20) - 1]]))
    assert vol.n_blocks == 1 and vol.coords().tolist() == [[-(1 << 20), 0, (1 << 20) - 1]] and int(vol.keys[0]) >= 0
    # fuse_views takes the class as it takes a TSDFVolume: it asks for .color and .integrate_many only
    assert mesh.fuse_views([], None, None, vol) == 0
