"""The block-sparse TSDF volume on the GPU: lg_blocks_touch / _merge / _regrid / _integrate / _mesh_count / _mesh_emit
bit for bit against the g++ build of the same lg_math.h text (keys, statistics, pools, vertices, colours and faces, order included), one
call with 11 views against 11 calls, the whole-block cull, blocks without neighbours, poisoned memory, streams, the counts lg_blocks_mesh_emit
holds its arguments against, the profile names, and mesh.fuse_views with a BlockTSDFVolume against render_geometry + the torch backend."""
import ctypes as C
import inspect
import math
import types

import numpy as np
import pytest
import torch

import blocks_common as bc
import mesh_common as mc
import poison_common as pz
import tolerance
from common import syn
from lightgaussian_amd import _lib, blocks, mesh
from lightgaussian_amd.gaussian_renderer import render_geometry

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:BlockTSDFVolume:RuntimeWarning")]      # (the 1 x 1 view's pixel is skipped)
DEV = "cuda:0"
# (colour, alpha, depth_max)
MODES = ((True, False, 0.0), (True, True, 3.6), (False, False, 0.0), (False, True, 3.6))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_views(views, color=True, alpha=False, depth_max=0.0):
    return [dict(depth=dev(v["depth"]), camera=v["cam"].to(DEV), color=dev(v["color"]) if color else None, alpha=dev(v["alpha"]) if alpha else None,
                 alpha_min=0.5, depth_max=depth_max) for v in views]


def gpu_volume(origin, voxel, trunc, keys=None, state=None, color=True, backend="hip"):
    vol = blocks.BlockTSDFVolume(voxel, origin=origin, trunc=trunc, color=color, device=DEV, backend=backend)
    if keys is not None and len(keys):
        vol.allocate_blocks(dev(bc.coords_of(keys)))
        assert np.array_equal(vol.keys.cpu().numpy(), keys)
    if state is not None:
        vol.tsdf.copy_(dev(state[0])); vol.weight.copy_(dev(state[1]))
        if state[2] is not None:
            vol.color.copy_(dev(state[2]))
    return vol


def state_of(vol):
    return tuple(None if t is None else t.cpu().numpy() for t in (vol.tsdf, vol.weight, vol.color))


def assert_same_state(got, want, what):
    for name, g, w in zip(("tsdf", "weight", "colour"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.shape == w.shape, (what, name, g.shape, w.shape)
            bad = np.flatnonzero(bc.bits(g).reshape(-1) != bc.bits(w).reshape(-1))
            assert bad.size == 0, f"{what}: {name} differs in {bad.size} words, first at {bad[0]}: {g.reshape(-1)[bad[0]]} vs {w.reshape(-1)[bad[0]]}"


def assert_same_mesh(got, want, name):
    v, f, c = (None if t is None else t.cpu().numpy() for t in got)
    assert v.shape == want["vertices"].shape and f.shape == want["faces"].shape and f.dtype == np.int32, f"{name}: counts differ"
    assert np.array_equal(f, want["faces"]), f"{name}: faces differ"
    assert np.array_equal(bc.bits(v), bc.bits(want["vertices"])), f"{name}: vertex bits differ"
    assert (c is None) == (want["colors"] is None) and (c is None or np.array_equal(bc.bits(c), bc.bits(want["colors"]))), f"{name}: colour bits differ"


def seeded_pools(n, color=True, seed=0):
    rs = np.random.RandomState(11 + seed)
    return (rs.uniform(-1, 1, (n, 8, 8, 8)).astype(np.float32), rs.randint(0, 6, (n, 8, 8, 8)).astype(np.float32),
            rs.uniform(0, 1, (n, 8, 8, 8, 3)).astype(np.float32) if color else None)


# ---- allocation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", (0, 1))
def test_allocate_gives_the_keys_and_statistics_of_the_harness(which):
    origin, voxel, trunc, views = bc.input_set(which)
    want, skipped = bc.harness_touch(origin, voxel, trunc, views)
    vol = gpu_volume(origin, voxel, trunc)
    out = vol.allocate(gpu_views(views))
    assert out == dict(blocks=len(want), new_blocks=len(want), skipped_pixels=skipped) and len(want) == (49, 151)[which]
    assert vol.keys.dtype == torch.int64 and np.array_equal(vol.keys.cpu().numpy(), want)
    assert_same_state(state_of(vol), bc.fresh_pools(len(want)), "fresh pools")
    assert vol.allocate(gpu_views(views))["new_blocks"] == 0
    # in two parts, either way round: the same keys; and with an alpha map and a depth_max
    a, b = gpu_volume(origin, voxel, trunc), gpu_volume(origin, voxel, trunc)
    gv = gpu_views(views, alpha=True, depth_max=3.6)
    a.allocate(gv[:3]); a.allocate(gv[3:]); b.allocate(gv[3:]); b.allocate(gv[:3])
    want2, _s = bc.harness_touch(origin, voxel, trunc, views, use_alpha=True, depth_max=3.6)
    assert np.array_equal(a.keys.cpu().numpy(), want2) and np.array_equal(b.keys.cpu().numpy(), want2)
    # a candidate buffer that is too small is sized by the answer and the call repeated: the same set
    c = gpu_volume(origin, voxel, trunc)
    c._capacity = lambda pixels: 8
    assert c.allocate(gpu_views(views))["blocks"] == len(want) and np.array_equal(c.keys.cpu().numpy(), want)


def test_allocate_small_images_no_blocks_and_skipped_pixels():
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    views = mc.sphere_views(9, sizes=mc.IMAGES)                   # 1 x 1, 33 x 17 and 70 x 45, more than one launch of 8 views
    want, skipped = bc.harness_touch(origin, voxel, trunc, views)
    vol = gpu_volume(origin, voxel, trunc, color=False)
    assert vol.allocate(gpu_views(views, color=False)) == dict(blocks=len(want), new_blocks=len(want), skipped_pixels=skipped)
    assert np.array_equal(vol.keys.cpu().numpy(), want) and len(want) > 0
    # maps that hold nothing: no block; a 1 x 1 map at distance 50: skipped, counted, one warning
    empty = gpu_volume(origin, voxel, trunc)
    cam = views[0]["cam"].to(DEV)
    assert empty.allocate([dict(depth=torch.zeros((17, 33), device=DEV), camera=cam)]) == dict(blocks=0, new_blocks=0, skipped_pixels=0)
    with pytest.warns(RuntimeWarning, match="skipped"):
        assert empty.allocate([dict(depth=torch.full((1, 1), 50.0, device=DEV), camera=cam)]) == dict(blocks=0, new_blocks=0, skipped_pixels=1)
    assert empty.n_blocks == 0 and empty.extract_mesh()[0].shape == (0, 3) and empty.extract_mesh()[1].shape == (0, 3)
    empty.integrate_many(gpu_views(views[:1]), allocate=False)       # no block: nothing to do
    one = gpu_volume(origin, voxel, trunc)
    assert one.allocate_blocks(torch.tensor([[2, -1, 0], [2, -1, 0]]))["blocks"] == 1 and one.coords().tolist() == [[2, -1, 0]]
    assert_same_state(state_of(one), bc.fresh_pools(1), "one fresh block")


def test_regrid_keeps_old_blocks_bit_for_bit():
    origin, voxel, trunc, views = bc.input_set(0)
    gv = gpu_views(views)
    for color in (True, False):
        vol = gpu_volume(origin, voxel, trunc, color=color)
        vol.allocate(gv[:2])
        old_keys, old = vol.keys.clone(), seeded_pools(vol.n_blocks, color)
        vol.tsdf.copy_(dev(old[0])); vol.weight.copy_(dev(old[1]))
        if color:
            vol.color.copy_(dev(old[2]))
        assert vol.allocate(gv[2:])["new_blocks"] > 0
        at = torch.searchsorted(vol.keys, old_keys).cpu().numpy()
        got = state_of(vol)
        new = np.ones(vol.n_blocks, bool); new[at] = False
        for g, o, fresh in zip(got, old, (1.0, 0.0, 0.0)):
            if g is not None:
                assert np.array_equal(bc.bits(g[at]), bc.bits(o)) and (g[new] == fresh).all()


# ---- integration --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", (False, True))
def test_integrate_bit_identical_to_the_harness(shifted):
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    if shifted:
        origin = bc.lattice_origin(origin, voxel, (-16, -16, -16))
    all_views = mc.sphere_views(11, sizes=mc.IMAGES)
    for n in (1, 8, 9, 11):
        views = all_views[:n] if n > 1 else all_views[1:2]           # (view 0 is the 1 x 1 image: its one pixel is skipped)
        for k, (color, alpha, depth_max) in enumerate(MODES):
            if n not in (9, 11) and k > 1:
                continue
            keys, _s = bc.harness_touch(origin, voxel, trunc, views, use_alpha=alpha, depth_max=depth_max)
            want = bc.harness_integrate(keys, origin, voxel, trunc, bc.fresh_pools(len(keys), color), views, use_alpha=alpha, depth_max=depth_max)
            vol = gpu_volume(origin, voxel, trunc, color=color)
            vol.integrate_many(gpu_views(views, color, alpha, depth_max))
            assert np.array_equal(vol.keys.cpu().numpy(), keys), f"n {n} mode {k}: keys differ"
            assert_same_state(state_of(vol), want, f"shifted {shifted} n {n} mode {k}")
            assert (want[1] > 0).any()
    # into seeded pools, without allocation: a point no view touched keeps the bits it had
    keys, _s = bc.harness_touch(origin, voxel, trunc, all_views)
    start = seeded_pools(len(keys))
    want = bc.harness_integrate(keys, origin, voxel, trunc, start, all_views, use_alpha=True)
    vol = gpu_volume(origin, voxel, trunc, keys, start)
    vol.integrate_many(gpu_views(all_views, True, True), allocate=False)
    assert_same_state(state_of(vol), want, "seeded pools")
    assert (bc.bits(want[1]) == bc.bits(start[1])).any() and (bc.bits(want[1]) != bc.bits(start[1])).any()


def test_one_call_with_11_views_is_11_calls_with_one():
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    views = mc.sphere_views(11, sizes=mc.IMAGES)
    keys, _s = bc.harness_touch(origin, voxel, trunc, views)
    start = seeded_pools(len(keys))
    once, each = gpu_volume(origin, voxel, trunc, keys, start), gpu_volume(origin, voxel, trunc, keys, start)
    gv = gpu_views(views, True, True, 3.6)
    once.integrate_many(gv)
    for v in gv:
        each.integrate(**v)
    assert torch.equal(once.keys, each.keys)
    assert_same_state(state_of(once), state_of(each), "11 views")
    assert not np.array_equal(bc.bits(state_of(once)[0]), bc.bits(start[0]))


def test_a_view_that_faces_away_changes_nothing():
    origin, voxel, trunc, views = bc.input_set(0)
    keys, _s = bc.harness_touch(origin, voxel, trunc, views)
    start = seeded_pools(len(keys))
    vol = gpu_volume(origin, voxel, trunc, keys, start)
    away = []
    for v in gpu_views(views):
        cam = v["camera"]
        vm = cam.world_view_transform.clone()
        vm[:, 0] *= -1; vm[:, 2] *= -1                      # half a turn about the view's y axis: everything in front is now behind
        away.append(dict(v, camera=types.SimpleNamespace(world_view_transform=vm, FoVx=cam.FoVx, FoVy=cam.FoVy)))
    vol.integrate_many(away, allocate=False)
    assert_same_state(state_of(vol), start, "views that face away")
    # and mixed into a batch, the views that do see the blocks give the harness's bits
    mixed = [away[0]] + gpu_views(views)[:3] + [away[1]]
    vol.integrate_many(mixed, allocate=False)
    assert_same_state(state_of(vol), bc.harness_integrate(keys, origin, voxel, trunc, start, views[:3]), "a batch with views that face away")


# ---- extraction ---------------------------------------------------------------------------------------------------------------------
def test_extract_equals_the_harness():
    keys, f, w, c, _dense = bc.scattered_field()
    origin, voxel, _t = mc.volume_spec((32, 32, 32))
    vol = gpu_volume(origin, voxel, 4 * voxel, keys, (f, w, c))
    want = bc.harness_extract(keys, f, w, c, vol.origin, vol.voxel_size)
    assert (want["used"][:, 1:15] > 0).all() and len(want["faces"]) > 500
    assert_same_mesh(vol.extract_mesh(drop_unreferenced=False), want, "scattered field")
    for iso, mw in ((0.25, 1.0), (-0.1, 2.0)):
        assert_same_mesh(vol.extract_mesh(iso=iso, min_weight=mw, drop_unreferenced=False), bc.harness_extract(keys, f, w, c, vol.origin, vol.voxel_size, iso, mw), f"iso {iso}")
    plain = gpu_volume(origin, voxel, 4 * voxel, keys, (f, w, None), color=False)
    assert_same_mesh(plain.extract_mesh(drop_unreferenced=False), bc.harness_extract(keys, f, w, None, vol.origin, vol.voxel_size), "without colour")
    # drop_unreferenced: the torch ops after the kernels
    v, fc, col = vol.extract_mesh()
    ref = np.unique(want["faces"])
    assert len(v) == len(ref) < len(want["vertices"]) and np.array_equal(bc.bits(v), bc.bits(want["vertices"][ref])) and np.array_equal(ref[fc.cpu().numpy()], want["faces"])
    # the fused sphere, both input sets (negative block coordinates in the first)
    for which in (0, 1):
        o, vx, tr, views = bc.input_set(which)
        fused = gpu_volume(o, vx, tr)
        fused.integrate_many(gpu_views(views))
        st = state_of(fused)
        want = bc.harness_extract(fused.keys.cpu().numpy(), *st, fused.origin, fused.voxel_size)
        assert len(want["faces"]) > 1000
        assert_same_mesh(fused.extract_mesh(drop_unreferenced=False), want, f"fused sphere, set {which}")


def test_blocks_without_neighbours():
    origin, voxel, _t = mc.volume_spec((8, 8, 8))
    for coords in ([[-3, 0, 5]], [[0, 0, 0], [1, 1, 1]], [[0, 0, 0], [-1, -1, -1], [1, 0, 0]]):
        keys = np.sort(bc.keys_of(coords))
        n = len(keys)
        f, w, c = mc.random_field((8, 8, 8 * n), seed=n, observed=0.93)
        state = (f.reshape(n, 8, 8, 8), w.reshape(n, 8, 8, 8), c.reshape(n, 8, 8, 8, 3))
        vol = gpu_volume(origin, voxel, 4 * voxel, keys, state)
        want = bc.harness_extract(keys, *state, vol.origin, vol.voxel_size)
        assert len(want["faces"]) > 50 * n
        assert_same_mesh(vol.extract_mesh(drop_unreferenced=False), want, f"blocks {coords}")


def test_emit_holds_its_arguments_against_the_counts():
    keys, f, w, c, _dense = bc.scattered_field(seed=1)
    origin, voxel, _t = mc.volume_spec((32, 32, 32))
    vol = gpu_volume(origin, voxel, 4 * voxel, keys, (f, w, c))
    want = bc.harness_extract(keys, f, w, c, vol.origin, vol.voxel_size)
    lib, s = blocks.load(), vol._struct()
    scratch = _lib.scratch(lib.lg_blocks_mesh_scratch_bytes(vol.n_blocks), DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    st = _lib.stream(DEV)
    assert lib.lg_blocks_mesh_count(C.byref(s), 0.0, 1.0, _lib.ptr(scratch), _lib.ptr(counts), 0, st) == _lib.LG_OK
    nv, nf = counts.tolist()
    assert (nv, nf) == (len(want["vertices"]), len(want["faces"]))
    guard = torch.full((nv + 8, 3), -1, dtype=torch.int32, device=DEV)
    v, fc = guard.view(torch.float32), torch.full((nf + 8, 3), -1, dtype=torch.int32, device=DEV)
    for a, b, word in ((nv - 1, nf, "n_vertices differs"), (nv, nf + 1, "n_faces differs"), (nv + 1, nf - 1, "n_vertices differs")):
        assert lib.lg_blocks_mesh_emit(C.byref(s), 0.0, 1.0, _lib.ptr(scratch), a, b, _lib.ptr(v), None, _lib.ptr(fc), 0, st) == _lib.LG_ERR_INVALID_ARGUMENT
        assert word in lib.lg_last_error().decode()
    torch.cuda.synchronize()
    assert bool((guard == -1).all()) and bool((fc == -1).all()), "a refused call wrote something"
    assert lib.lg_blocks_mesh_emit(C.byref(s), 0.0, 1.0, _lib.ptr(scratch), nv, nf, _lib.ptr(v), None, _lib.ptr(fc), 0, st) == _lib.LG_OK
    torch.cuda.synchronize()
    assert bool((guard[nv:] == -1).all()) and bool((fc[nf:] == -1).all()) and np.array_equal(fc[:nf].cpu().numpy(), want["faces"])
    assert np.array_equal(bc.bits(v[:nv]), bc.bits(want["vertices"]))


# ---- memory and streams ----------------------------------------------------------------------------------------------------------------
def _whole_pipeline(color=True):
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    views = mc.sphere_views(9, sizes=mc.IMAGES)

    def run():
        vol = gpu_volume(origin, voxel, trunc, color=color)
        gv = gpu_views(views, color, True, 3.6)
        stats = vol.allocate(gv[:4])                              # allocate, then grow: touch, merge and regrid
        vol.integrate_many(gv[:4], allocate=False)
        vol.integrate_many(gv[4:])
        v, f, c = vol.extract_mesh(drop_unreferenced=False)
        return dict(first=stats["blocks"], keys=vol.keys, tsdf=vol.tsdf, weight=vol.weight, color=vol.color, vertices=v, faces=f, colors=c)
    return run


@pytest.mark.parametrize("color", (True, False))
def test_outputs_do_not_depend_on_what_memory_held(color):
    runs = pz.run_all(_whole_pipeline(color))
    pz.assert_identical(runs, f"allocate + regrid + integrate + extract, colour {color}")
    assert runs[0][1]["faces"].shape[0] > 0 and runs[0][1]["keys"].shape[0] > runs[0][1]["first"] > 0


def test_two_streams_and_two_runs_give_the_same_bits():
    run = _whole_pipeline()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(DEV)
        with torch.cuda.stream(s):
            outs.append(run())
        s.synchronize()
    pz.assert_identical([("first stream", outs[0]), ("second stream", outs[1])], "two streams")
    pz.assert_identical([("first run", run()), ("second run", run()), ("a stream", outs[0])], "two runs")


def test_profile_names():
    run = _whole_pipeline()
    _lib.profile_reset()
    blocks.set_profile(True)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        blocks.set_profile(False)
    seen = _lib.profile_read()
    _lib.profile_reset()
    assert seen.get("blocks_touch", (0, 0))[1] == 4, seen                     # two allocations: lg_blocks_touch and lg_blocks_merge each
    assert seen.get("blocks_regrid", (0, 0))[1] == 2, seen
    assert seen.get("blocks_integrate", (0, 0))[1] == 2, seen                 # 4 views and 5 views: one launch each
    for name in ("blocks_mesh_count", "blocks_mesh_scan", "blocks_mesh_emit"):
        assert seen.get(name, (0, 0))[1] == 1, (name, seen)


# ---- on top of the renderer -----------------------------------------------------------------------------------------------------------
def test_fuse_views_with_a_block_volume():
    W, H, N = 70, 45, 3000
    model = syn.make_gaussians(N, seed=11, extent=(1.2, 0.9, 1.2), log_scale_mean=math.log(0.08), opacity_mean=1.0).to(DEV)
    cams = [syn.orbit_camera(k, 9, W, H, radius=4.0, height_y=-1.5 if k % 2 == 0 else 0.8).to(DEV) for k in range(9)]
    pipe = syn.PipelineParams()
    origin, voxel, trunc = mc.volume_spec(bc.FIRST_DIMS)
    views = []
    with torch.no_grad():
        for cam in cams:
            pkg = render_geometry(cam, model, pipe, distortion=True, geometry_grad=False)
            views.append(dict(cam=cam, W=W, H=H, tanfov=mesh.tanfov(cam), vm=cam.world_view_transform.cpu().numpy().astype(np.float32).reshape(16),
                              depth=pkg["median_depth"].cpu().numpy(), color=pkg["render"].cpu().numpy(), alpha=pkg["alpha"].cpu().numpy()))
    gv = gpu_views(views, True, True, 0.0)
    keys, skipped = bc.harness_touch(origin, voxel, trunc, views, use_alpha=True)
    assert skipped == 0 and len(keys) > 8
    # a volume that starts empty: fuse_views integrates 8 views, then 1, and the key list may grow in between; the harness in the same two steps
    grow = blocks.BlockTSDFVolume(voxel, origin=origin, trunc=trunc, device=DEV)
    assert mesh.fuse_views(cams, model, pipe, grow) == 9 and "blocks" not in inspect.getsource(mesh)
    assert np.array_equal(grow.keys.cpu().numpy(), keys)
    k8, _s = bc.harness_touch(origin, voxel, trunc, views[:8], use_alpha=True)
    step = bc.harness_integrate(k8, origin, voxel, trunc, bc.fresh_pools(len(k8)), views[:8], use_alpha=True)
    at = np.searchsorted(keys, k8)
    grown = list(bc.fresh_pools(len(keys)))
    for g, s in zip(grown, step):
        g[at] = s
    assert_same_state(state_of(grow), bc.harness_integrate(keys, origin, voxel, trunc, tuple(grown), views[8:], use_alpha=True), "fuse_views into an empty volume")
    # with every block allocated first, all nine views reach every block: the harness's bits, and the torch backend on identical maps by the
    # tolerance rule against the float64 twin on the blocks' dense box
    vol = blocks.BlockTSDFVolume(voxel, origin=origin, trunc=trunc, device=DEV)
    tor = blocks.BlockTSDFVolume(voxel, origin=origin, trunc=trunc, device=DEV, backend="torch")
    vol.allocate(gv); tor.allocate(gv)
    assert torch.equal(tor.keys, vol.keys) and np.array_equal(vol.keys.cpu().numpy(), keys)
    assert mesh.fuse_views(cams, model, pipe, vol) == 9
    tor.integrate_many(gv, allocate=False)
    got, ref = state_of(vol), state_of(tor)
    assert_same_state(got, bc.harness_integrate(keys, origin, voxel, trunc, bc.fresh_pools(len(keys)), views, use_alpha=True), "fuse_views")
    base, dims = bc.dense_box(keys)
    r64, d64, near = mc.twin_integrate(dims, bc.lattice_origin(origin, voxel, base), voxel, trunc, mc.fresh_volume(dims), views, use_alpha=True)
    at = bc.block_index(keys, base, dims).reshape(-1)
    keep = ~near.any(axis=0)[at]
    print(f"{100 * (1 - keep.mean()):.3f} % of the points have a pair within a margin, {100 * d64[:, at].mean():.1f} % of the pairs update")
    assert 1 - keep.mean() <= mc.MAX_LEFT_OUT and d64.any()
    assert np.array_equal(got[1].reshape(-1)[keep], r64[1].reshape(-1)[at][keep]) and np.array_equal(ref[1].reshape(-1)[keep], r64[1].reshape(-1)[at][keep])
    tolerance.assert_rule3(got[0].reshape(-1)[keep], r64[0].reshape(-1)[at][keep], ref[0].reshape(-1)[keep], "tsdf")
    tolerance.assert_rule3(got[2].reshape(-1, 3)[keep], r64[2].reshape(-1, 3)[at][keep], ref[2].reshape(-1, 3)[keep], "colour")
    v, f, c = vol.extract_mesh()
    assert f.shape[0] > 0 and int(f.max()) < v.shape[0] and c.shape == v.shape
    assert mc.mesh_properties(v.cpu().numpy(), f.cpu().numpy())["volume"] > 0
    tv, tf, _tc = tor.extract_mesh()
    assert tf.shape == f.shape and tv.shape == v.shape
