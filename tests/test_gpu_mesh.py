"""TSDF fusion and marching tetrahedra on the GPU: lg_tsdf_integrate bit for bit against the g++ build of the
same lg_math.h text, one call with n views against n calls, untouched points, lg_mesh_count / lg_mesh_emit exactly against the harness,
poisoned memory, streams, fuse_views against render_geometry + the torch backend, and the checks of the Python surface."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mesh_common as mc
import poison_common as pz
import tolerance
from common import syn
from lightgaussian_amd import _lib, mesh
from lightgaussian_amd.gaussian_renderer import render_geometry

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = (0, 1, mc.B, mc.B + 1, 2 * mc.B + 1)
# (colour, alpha, depth_max)
MODES = ((True, False, 0.0), (True, True, 3.6), (False, False, 0.0), (False, True, 3.6))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def off16(t):
    """The same values in device memory that is 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def gpu_volume(dims, spec, state, misaligned=False, backend="hip"):
    origin, voxel, trunc = spec
    vol = mesh.TSDFVolume(origin, dims, voxel, trunc=trunc, color=state[2] is not None, device=DEV, backend=backend)
    vol.tsdf.copy_(dev(state[0])); vol.weight.copy_(dev(state[1]))
    if state[2] is not None:
        vol.color.copy_(dev(state[2]))
    if misaligned:
        vol.tsdf, vol.weight = off16(vol.tsdf), off16(vol.weight)
        if vol.color is not None:
            vol.color = off16(vol.color)
    return vol


def gpu_views(views, color, alpha, depth_max):
    return [dict(depth=dev(v["depth"]), camera=v["cam"].to(DEV), color=dev(v["color"]) if color else None, alpha=dev(v["alpha"]) if alpha else None,
                 alpha_min=0.5, depth_max=depth_max) for v in views]


def state_of(vol):
    return tuple(None if t is None else t.cpu().numpy() for t in (vol.tsdf, vol.weight, vol.color))


def assert_same_state(got, want, what):
    for name, g, w in zip(("tsdf", "weight", "colour"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            bad = np.flatnonzero(mc.bits(g).reshape(-1) != mc.bits(w).reshape(-1))
            assert bad.size == 0, f"{what}: {name} differs in {bad.size} words, first at {bad[0]}: {g.reshape(-1)[bad[0]]} vs {w.reshape(-1)[bad[0]]}"


# ---- integration --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", mc.GRIDS)
def test_integrate_bit_identical_to_the_harness(dims):
    spec = mc.volume_spec(dims)
    all_views = mc.sphere_views(COUNTS[-1], sizes=mc.IMAGES)
    touched_any = False
    for n in COUNTS:
        views = all_views[:n]
        for k, (color, alpha, depth_max) in enumerate(MODES):
            if n not in (mc.B + 1, COUNTS[-1]) and k > 1:
                continue
            start = mc.seeded_volume(dims, color=color, seed=n)
            want, decided = mc.harness_integrate(dims, *spec, start, views, use_alpha=alpha, depth_max=depth_max, decided=True)
            for misaligned in (False, True):
                vol = gpu_volume(dims, spec, start, misaligned)
                vol.integrate_many(gpu_views(views, color, alpha, depth_max))
                got = state_of(vol)
                assert_same_state(got, want, f"{dims} n {n} mode {k} misaligned {misaligned}")
            # a point no view touched keeps the bits it had (the seeded pattern, not the initial values)
            untouched = ~decided.astype(bool).any(axis=0) if n else np.ones(int(np.prod(dims)), bool)
            assert np.array_equal(mc.bits(got[0]).reshape(-1)[untouched], mc.bits(start[0]).reshape(-1)[untouched])
            assert np.array_equal(mc.bits(got[1]).reshape(-1)[untouched], mc.bits(start[1]).reshape(-1)[untouched])
            touched_any |= bool(n and (~untouched).any())
    assert touched_any, f"{dims}: no view updated a point"


@pytest.mark.parametrize("dims", ((67, 5, 3), (24, 20, 16)))
def test_one_call_with_n_views_is_n_calls_with_one(dims):
    spec = mc.volume_spec(dims)
    views = mc.sphere_views(COUNTS[-1], sizes=mc.IMAGES)
    start = mc.seeded_volume(dims)
    once, each = gpu_volume(dims, spec, start), gpu_volume(dims, spec, start)
    gv = gpu_views(views, True, True, 3.6)
    once.integrate_many(gv)
    for v in gv:
        each.integrate(**v)
    assert_same_state(state_of(once), state_of(each), f"{dims}")
    assert not np.array_equal(mc.bits(state_of(once)[0]), mc.bits(start[0]))


# ---- extraction ---------------------------------------------------------------------------------------------------------------------
def mesh_cases():
    """(name, dims, origin, voxel, (tsdf, weight, colour or None))"""
    dims = (12, 12, 12)
    origin, voxel, _t = mc.volume_spec(dims)
    yield "clipped sphere", dims, origin, voxel, mc.sphere_field(dims, origin, voxel, 1.0) + (None,)
    yield "lattice-aligned sphere", dims, (-5.0, -5.0, -5.0), 1.0, mc.sphere_field(dims, (-5.0, -5.0, -5.0), 1.0, 3.0) + (None,)
    for dims in mc.GRIDS + ((12, 11, 10), (33, 32, 5)):
        origin, voxel, _t = mc.volume_spec(dims)
        yield f"random {dims}", dims, origin, voxel, mc.random_field(dims, seed=dims[0], observed=0.93)


def hip_extract(dims, origin, voxel, field, **kw):
    vol = gpu_volume(dims, (origin, voxel, 4 * voxel), field)
    v, f, c = vol.extract_mesh(drop_unreferenced=False, **kw)
    return dict(vertices=v, faces=f, colors=c)


def assert_same_mesh(got, want, name):
    v, f, c = got["vertices"].cpu().numpy(), got["faces"].cpu().numpy(), None if got["colors"] is None else got["colors"].cpu().numpy()
    assert v.shape == want["vertices"].shape and f.shape == want["faces"].shape and f.dtype == np.int32, f"{name}: counts differ"
    assert np.array_equal(f, want["faces"]), f"{name}: faces differ"
    assert np.array_equal(mc.bits(v), mc.bits(want["vertices"])), f"{name}: vertex bits differ"
    assert (c is None) == (want["colors"] is None) and (c is None or np.array_equal(mc.bits(c), mc.bits(want["colors"]))), f"{name}: colour bits differ"


def test_extract_equals_the_harness():
    used = np.zeros((6, 16), np.int64)
    for name, dims, origin, voxel, field in mesh_cases():
        want = mc.harness_extract(*field, origin, voxel)
        used += want["used"]
        assert_same_mesh(hip_extract(dims, origin, voxel, field), want, name)
        if name.startswith("random (12"):
            assert (want["used"][:, 1:15] > 0).all(), "the random field must meet all 6 x 14 non-trivial table entries"
            for iso, mw in ((0.25, 1.0), (-0.1, 3.0)):
                assert_same_mesh(hip_extract(dims, origin, voxel, field, iso=iso, min_weight=mw), mc.harness_extract(*field, origin, voxel, iso, mw), f"{name} iso {iso}")
    assert (used[:, 1:15] > 0).all()
    # drop_unreferenced on the device: the torch ops after the kernels
    name, dims, origin, voxel, field = [c for c in mesh_cases() if c[0].startswith("random (12")][0]
    vol = gpu_volume(dims, (origin, voxel, 4 * voxel), field)
    v, f, c = vol.extract_mesh()
    want = mc.harness_extract(*field, origin, voxel)
    ref = np.unique(want["faces"])
    assert len(v) == len(ref) < len(want["vertices"]) and np.array_equal(mc.bits(v.cpu().numpy()), mc.bits(want["vertices"][ref]))
    assert np.array_equal(ref[f.cpu().numpy()], want["faces"]) and np.array_equal(mc.bits(c.cpu().numpy()), mc.bits(want["colors"][ref]))


def test_emit_holds_its_arguments_against_the_counts():
    dims = (12, 11, 10)
    origin, voxel, _t = mc.volume_spec(dims)
    field = mc.random_field(dims, seed=12, observed=0.93)
    vol = gpu_volume(dims, (origin, voxel, 4 * voxel), field)
    lib, s = mesh.load(), vol._struct()
    scratch = _lib.scratch(lib.lg_mesh_scratch_bytes(*dims), DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    st = _lib.stream(DEV)
    assert lib.lg_mesh_count(C.byref(s), 0.0, 1.0, _lib.ptr(scratch), _lib.ptr(counts), 0, st) == _lib.LG_OK
    nv, nf = counts.tolist()
    assert (nv, nf) == mc.harness_counts(field[0], field[1])
    guard = torch.full((nv + 8, 3), -1, dtype=torch.int32, device=DEV)
    v, f = guard.view(torch.float32), torch.full((nf + 8, 3), -1, dtype=torch.int32, device=DEV)
    for a, b, word in ((nv - 1, nf, "n_vertices differs"), (nv, nf + 1, "n_faces differs"), (nv + 1, nf - 1, "n_vertices differs")):
        assert lib.lg_mesh_emit(C.byref(s), 0.0, 1.0, _lib.ptr(scratch), a, b, _lib.ptr(v), None, _lib.ptr(f), 0, st) == _lib.LG_ERR_INVALID_ARGUMENT
        assert word in lib.lg_last_error().decode()
    torch.cuda.synchronize()
    assert bool((guard == -1).all()) and bool((f == -1).all()), "a refused call wrote something"
    assert lib.lg_mesh_emit(C.byref(s), 0.0, 1.0, _lib.ptr(scratch), nv, nf, _lib.ptr(v), None, _lib.ptr(f), 0, st) == _lib.LG_OK
    torch.cuda.synchronize()
    assert bool((guard[nv:] == -1).all()) and bool((f[nf:] == -1).all()) and bool((f[:nf] >= 0).all()) and bool(torch.isfinite(v[:nv]).all())


# ---- memory and streams ----------------------------------------------------------------------------------------------------------------
def _whole_pipeline(dims, n_views, color=True):
    spec = mc.volume_spec(dims)
    views = mc.sphere_views(n_views, sizes=mc.IMAGES)
    start = mc.seeded_volume(dims, color=color)

    def run():
        vol = gpu_volume(dims, spec, start)
        vol.integrate_many(gpu_views(views, color, True, 3.6))
        v, f, c = vol.extract_mesh(drop_unreferenced=False)
        return dict(tsdf=vol.tsdf, weight=vol.weight, color=vol.color, vertices=v, faces=f, colors=c)
    return run


@pytest.mark.parametrize("dims,color", [((24, 20, 16), True), ((67, 5, 3), False)])
def test_outputs_do_not_depend_on_what_memory_held(dims, color):
    runs = pz.run_all(_whole_pipeline(dims, mc.B + 1, color))
    pz.assert_identical(runs, f"integrate + extract {dims}")
    assert runs[0][1]["faces"].shape[0] > 0


def test_two_streams_give_the_same_bits():
    run = _whole_pipeline((24, 20, 16), 2 * mc.B + 1)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(DEV)
        with torch.cuda.stream(s):
            outs.append(run())
        s.synchronize()
    pz.assert_identical([("first stream", outs[0]), ("second stream", outs[1])], "two streams")
    dims = (24, 20, 16)
    want = mc.harness_integrate(dims, *mc.volume_spec(dims), mc.seeded_volume(dims), mc.sphere_views(2 * mc.B + 1, sizes=mc.IMAGES), use_alpha=True, depth_max=3.6)
    assert_same_state(tuple(outs[0][k].cpu().numpy() for k in ("tsdf", "weight", "color")), want, "two streams against the harness")


def test_profile_names():
    run = _whole_pipeline((24, 20, 16), 2 * mc.B + 1)
    _lib.profile_reset()
    mesh.set_profile(True)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        mesh.set_profile(False)
    seen = _lib.profile_read()
    assert seen.get("tsdf_integrate", (0, 0))[1] == 3, seen                 # 17 views: launches of 8, 8 and 1
    for name in ("mesh_count", "mesh_scan", "mesh_emit"):
        assert seen.get(name, (0, 0))[1] == 1, (name, seen)
    _lib.profile_reset()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_backends_and_refusals_on_the_device():
    dims = (24, 20, 16)
    spec = mc.volume_spec(dims)
    views = mc.sphere_views(3)
    start = mc.fresh_volume(dims)
    want = mc.harness_integrate(dims, *spec, start, views)
    # CPU tensors take the torch path, whatever the backend says
    cpu = mesh.TSDFVolume(spec[0], dims, spec[1], trunc=spec[2], device="cpu", backend="hip")
    cpu.integrate_many([dict(depth=torch.from_numpy(v["depth"]), camera=v["cam"], color=torch.from_numpy(v["color"])) for v in views])
    assert np.array_equal(cpu.weight.numpy(), want[1]) and np.abs(cpu.tsdf.numpy() - want[0]).max() <= 1e-5
    # the torch backend on the device is the comparand: same decisions away from the margins, same mesh order
    _r, _d, near = mc.twin_integrate(dims, *spec, start, views)
    keep = ~near.any(axis=0)
    tor = gpu_volume(dims, spec, start, backend="torch")
    tor.integrate_many(gpu_views(views, True, False, 0.0))
    got = state_of(tor)
    assert np.array_equal(got[1].reshape(-1)[keep], want[1].reshape(-1)[keep])
    tolerance.assert_rule3(got[0].reshape(-1)[keep], want[0].reshape(-1)[keep].astype(np.float64), want[0].reshape(-1)[keep], "torch backend on the device: tsdf")
    hip = gpu_volume(dims, spec, want)
    tor = gpu_volume(dims, spec, want, backend="torch")
    (v1, f1, c1), (v2, f2, c2) = hip.extract_mesh(), tor.extract_mesh()
    assert torch.equal(f1, f2) and v1.shape == v2.shape and float((v1 - v2).abs().max()) <= 1e-5 and float((c1 - c2).abs().max()) <= 1e-5
    # non-contiguous GPU tensors with backend="hip" raise
    v = gpu_views(views[:1], True, False, 0.0)[0]
    with pytest.raises(ValueError, match="contiguous"):
        hip.integrate(v["depth"].t().contiguous().t(), v["camera"], color=v["color"])
    hip.tsdf = hip.tsdf.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    with pytest.raises(ValueError, match="contiguous"):
        hip.extract_mesh()
    # no view: LG_OK, nothing launched, nothing changed
    seeded = mc.seeded_volume(dims)
    vol = gpu_volume(dims, spec, seeded)
    vol.integrate_many([])
    s = vol._struct()
    assert mesh.load().lg_tsdf_integrate(C.byref(s), 0, None, 0, _lib.stream(DEV)) == _lib.LG_OK
    assert_same_state(state_of(vol), seeded, "no view")


def test_fuse_views_against_render_geometry_and_the_torch_backend():
    W, H, N = 70, 45, 3000
    model = syn.make_gaussians(N, seed=11, extent=(1.2, 0.9, 1.2), log_scale_mean=math.log(0.08), opacity_mean=1.0).to(DEV)
    cams = [syn.orbit_camera(k, 4, W, H, radius=4.0, height_y=-1.5 if k % 2 == 0 else 0.8).to(DEV) for k in range(4)]
    pipe = syn.PipelineParams()
    dims = (24, 20, 16)
    spec = mc.volume_spec(dims)
    for which in ("median_depth", "depth"):
        vol = mesh.TSDFVolume(spec[0], dims, spec[1], trunc=spec[2], device=DEV)
        assert mesh.fuse_views(cams, model, pipe, vol, depth=which) == 4
        views = []
        with torch.no_grad():
            for cam in cams:
                pkg = render_geometry(cam, model, pipe, distortion=(which == "median_depth"), geometry_grad=False)
                views.append(dict(cam=cam, W=W, H=H, tanfov=mesh.tanfov(cam), vm=cam.world_view_transform.cpu().numpy().astype(np.float32).reshape(16),
                                  depth=pkg[which].cpu().numpy(), color=pkg["render"].cpu().numpy(), alpha=pkg["alpha"].cpu().numpy()))
        tor = mesh.TSDFVolume(spec[0], dims, spec[1], trunc=spec[2], device=DEV, backend="torch")
        tor.integrate_many(gpu_views(views, True, True, 0.0))
        start = mc.fresh_volume(dims)
        r64, d64, near = mc.twin_integrate(dims, *spec, start, views, use_alpha=True)
        keep = ~near.any(axis=0)
        print(f"{which}: {100 * near.mean():.3f} % of the pairs within a margin, {100 * d64.mean():.1f} % update")
        assert near.mean() <= mc.MAX_LEFT_OUT and d64.any()
        got, ref = state_of(vol), state_of(tor)
        assert np.array_equal(got[1].reshape(-1)[keep], r64[1].reshape(-1)[keep]) and np.array_equal(ref[1].reshape(-1)[keep], r64[1].reshape(-1)[keep])
        tolerance.assert_rule3(got[0].reshape(-1)[keep], r64[0].reshape(-1)[keep], ref[0].reshape(-1)[keep], f"{which} tsdf")
        tolerance.assert_rule3(got[2].reshape(-1, 3)[keep], r64[2].reshape(-1, 3)[keep], ref[2].reshape(-1, 3)[keep], f"{which} colour")
        # and the same maps through the harness: the bits
        want = mc.harness_integrate(dims, *spec, start, views, use_alpha=True)
        assert_same_state(got, want, f"fuse_views {which}")
        v, f, c = vol.extract_mesh()
        assert f.shape[0] > 0 and int(f.max()) < v.shape[0] and c.shape == v.shape
