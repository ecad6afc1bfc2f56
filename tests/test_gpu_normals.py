"""Normals on the GPU: lg_normal_rows and lg_depth_normals bit for bit against the g++ build of the same
lg_math.h text, the backwards and the loss scalar against the float64 twin by rule 3, stream determinism, poisoned memory, the
argument checks of include/lightgaussian_normals.h, and render_geometry + normal_consistency_loss end to end against the dense twin."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import dense_twin
import features_geom_common as fg
import normals_common as nc
import tolerance
from common import syn
from lightgaussian_amd import _lib, normals
from lightgaussian_amd.gaussian_renderer import render_features, render_geometry

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TX, TY = nc.TANFOV
KINDS = ("noisy", "plane")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def off16(a):
    """The same values in device memory that is 4-byte but not 16-byte aligned."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return view


def poisoned(*shape):
    """Uninitialised-looking output memory: every byte 0xFF (a NaN pattern)."""
    return torch.full(shape, -1, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def stream_arg(s=None):
    return C.c_void_p((s or torch.cuda.current_stream(DEV)).cuda_stream)


def p(t):
    return _lib.ptr(t)


def hip_rows(xyz, sc, q, vm, out=None, stream=None):
    N = xyz.shape[0]
    out = poisoned(N, 4) if out is None else out
    _lib.check(normals.load().lg_normal_rows(N, p(xyz), p(sc), p(q), p(vm), p(out), 0, stream_arg(stream)))
    return out


def hip_rows_bwd(xyz, sc, q, vm, g, stream=None):
    N = xyz.shape[0]
    d_xyz, d_rot = poisoned(N, 3), poisoned(N, 4)
    _lib.check(normals.load().lg_normal_rows_bwd(N, p(xyz), p(sc), p(q), p(vm), p(g), p(d_xyz), p(d_rot), 0, stream_arg(stream)))
    return d_xyz, d_rot


def hip_depth_normals(depth, stream=None):
    H, W = depth.shape
    nd = poisoned(3, H, W)
    _lib.check(normals.load().lg_depth_normals(H, W, p(depth), TX, TY, p(nd), 0, stream_arg(stream)))
    return nd


def hip_depth_normals_bwd(depth, g, stream=None):
    H, W = depth.shape
    d = poisoned(H, W)
    _lib.check(normals.load().lg_depth_normals_bwd(H, W, p(depth), TX, TY, p(g), p(d), 0, stream_arg(stream)))
    return d


def hip_loss(nr, depth, alpha, weight, want_nd=True, stream=None):
    H, W = depth.shape
    lib = normals.load()
    nbytes = lib.lg_normal_loss_scratch_bytes(H, W)
    assert nbytes > 0
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    loss, nd = poisoned(1), poisoned(3, H, W) if want_nd else None
    _lib.check(lib.lg_normal_loss(H, W, p(nr), p(depth), p(alpha), p(weight), TX, TY, p(loss), p(nd), p(scratch), 0, stream_arg(stream)))
    return loss, nd


def hip_loss_bwd(nr, depth, alpha, weight, g_loss=nc.G_LOSS, stream=None):
    H, W = depth.shape
    g = torch.tensor([g_loss], dtype=torch.float32, device=DEV)
    d_nr, d_depth = poisoned(3, H, W), poisoned(H, W)
    _lib.check(normals.load().lg_normal_loss_bwd(H, W, p(nr), p(depth), p(alpha), p(weight), TX, TY, p(g), p(d_nr), p(d_depth), 0, stream_arg(stream)))
    return d_nr, d_depth


# ---- forward bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", nc.NS)
def test_rows_forward_bit_identical_to_the_harness(N):
    for ci, cam in enumerate(nc.cameras()):
        xyz, sc, q = nc.rows_inputs(N, seed=ci)
        vm = nc.view_matrix(cam)
        want = nc.harness_rows(xyz, sc, q, vm)[0]
        for put in (dev, off16):                     # whole 16-byte words, and one dword at a time
            got = hip_rows(put(xyz), put(sc), put(q), dev(vm), out=put(np.full((N, 4), np.nan, np.float32)))
            bad = np.nonzero((bits(got) != want.view(np.uint32)).any(axis=1))[0]
            assert bad.size == 0, f"N {N} camera {ci} {put.__name__}: rows {bad[:8]} differ, e.g. {got[bad[0]].tolist()} vs {want[bad[0]].tolist()}"


@pytest.mark.parametrize("W,H", nc.SIZES)
def test_depth_normals_forward_bit_identical_to_the_harness(W, H):
    nr, alpha, weight, _g = nc.loss_maps(W, H)
    for kind in KINDS:
        depth = nc.depth_maps(W, H)[kind]
        want = nc.harness_depth_normals(depth)
        got = hip_depth_normals(dev(depth))
        assert same(got.cpu().numpy(), want), f"{W}x{H} {kind}: {int((bits(got) != want.view(np.uint32)).sum())} words differ"
        loss, nd = hip_loss(dev(nr), dev(depth), dev(alpha), dev(weight))
        assert same(nd.cpu().numpy(), want), f"{W}x{H} {kind}: the loss kernel's N_d differs"
        # the scalar: the same float32 terms, summed per lane over at most 32 rows and over the lanes in 6 steps in float32 (each step
        # within u of its partial sum), then in double, then rounded once: 38 u mean |term| + u |L| against the harness's double sum
        ref = nc.harness_loss(nr, depth, alpha, weight)
        terms = 1.0 - (alpha * weight).astype(np.float64) * (nr.astype(np.float64) * want).sum(axis=0)
        bound = 38 * nc.U * np.abs(terms).mean() + nc.U * abs(ref)
        print(f"{W}x{H} {kind}: loss {float(loss):.7f} (harness, double sum {ref:.7f}), difference {abs(float(loss) - ref):.2e}, bound {bound:.2e}")
        assert abs(float(loss) - ref) <= bound


# ---- backwards and the scalar against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cam_index", [(65, 0), (257, 1)])
def test_rows_backward_against_float64(N, cam_index):
    ref = nc.rows_grad_reference(N, cam_index)
    xyz, sc, q, vm, g = ref["inputs"]
    want = nc.harness_rows_bwd(xyz, sc, q, vm, g)
    for put in (dev, off16):
        got = hip_rows_bwd(put(xyz), put(sc), put(q), dev(vm), put(g))
        for k, name in enumerate(("d_xyz", "d_rotation")):
            tolerance.assert_rule3(got[k].cpu().numpy(), ref["float64"][k], ref["float32"][k], f"rows backward N {N} {put.__name__} {name}")
            print(f"    bit-identical to the harness: {same(got[k].cpu().numpy(), want[k])}")
    # the autograd Function is the same two launches
    x, r = dev(xyz).requires_grad_(), dev(q).requires_grad_()
    cam = nc.cameras()[cam_index]
    rows = normals.gaussian_normals(x, dev(sc), r, cam.to(DEV))
    assert same(rows.detach().cpu().numpy(), hip_rows(dev(xyz), dev(sc), dev(q), dev(vm)).cpu().numpy())
    (rows * dev(g)).sum().backward()
    assert same(x.grad.cpu().numpy(), got[0].cpu().numpy()) and same(r.grad.cpu().numpy(), got[1].cpu().numpy())
    torch_rows = normals.gaussian_normals(dev(xyz), dev(sc), dev(q), cam.to(DEV), backend="torch")
    keep = nc.keep_rows(xyz, sc, q, vm)[3]
    assert float((torch_rows - rows.detach())[torch.from_numpy(keep).to(DEV)].abs().max()) <= 4 * nc.NORMAL_BOUND * 8


@pytest.mark.parametrize("W,H", nc.SIZES)
def test_image_backwards_against_float64(W, H):
    for kind in KINDS:
        ref = nc.image_reference(W, H, kind)
        depth, nr, alpha, weight, g = ref["inputs"]
        d_nr, d_depth = hip_loss_bwd(dev(nr), dev(depth), dev(alpha), dev(weight))
        got = dict(d_depth_plain=hip_depth_normals_bwd(dev(depth), dev(g)).cpu().numpy(), d_nr=d_nr.cpu().numpy(), d_depth=d_depth.cpu().numpy())
        nc.assert_image_gradients(got, ref, f"{W}x{H} {kind}", ("d_depth_plain", "d_nr", "d_depth"))
        loss = float(hip_loss(dev(nr), dev(depth), dev(alpha), dev(weight), want_nd=False)[0])
        print(f"{W}x{H} {kind}: loss {loss:.7f}, float64 twin {ref['float64']['loss']:.7f}, float32 twin {ref['float32']['loss']:.7f}")
        assert abs(loss - ref["float64"]["loss"]) <= max(1e-4 * abs(ref["float64"]["loss"]), 3 * abs(ref["float32"]["loss"] - ref["float64"]["loss"]))


def test_autograd_functions_are_the_entry_points():
    W, H = 70, 45
    ref = nc.image_reference(W, H, "plane", weighted=False)
    depth, nr, alpha, _none, g = ref["inputs"]
    cam = nc.Camera()
    assert tuple(np.float32(v) for v in normals.tanfov(cam)) == (np.float32(TX), np.float32(TY))      # the same float32 arguments as hip_*
    d, n = dev(depth).requires_grad_(), dev(nr).requires_grad_()
    nd = normals.depth_to_normal(d, cam)
    assert same(nd.detach().cpu().numpy(), hip_depth_normals(dev(depth)).cpu().numpy())
    (nd * dev(g)).sum().backward()
    assert same(d.grad.cpu().numpy(), hip_depth_normals_bwd(dev(depth), dev(g)).cpu().numpy())
    d.grad = None
    loss = normals.normal_consistency_loss(n, d, dev(alpha), cam)
    assert loss.dim() == 0 and same(loss.detach().cpu().numpy().reshape(1), hip_loss(dev(nr), dev(depth), dev(alpha), None)[0].cpu().numpy())
    (nc.G_LOSS * loss).backward()
    want = hip_loss_bwd(dev(nr), dev(depth), dev(alpha), None)
    assert same(n.grad.cpu().numpy(), want[0].cpu().numpy()) and same(d.grad.cpu().numpy(), want[1].cpu().numpy())
    nc.assert_image_gradients(dict(d_nr=n.grad.cpu().numpy(), d_depth=d.grad.cpu().numpy()), ref, "unweighted", ("d_nr", "d_depth"))
    # the torch backend on the device is the comparand: the same numbers within the float32 bound
    d2 = dev(depth).requires_grad_()
    lt = normals.normal_consistency_loss(dev(nr), d2, dev(alpha), cam, backend="torch")
    (nc.G_LOSS * lt).backward()
    assert abs(float(lt.detach()) - float(loss.detach())) <= 1e-5
    tolerance.assert_rule3(d2.grad.cpu().numpy(), ref["float64"]["d_depth"], ref["float32"]["d_depth"], "torch backend d_depth")
    with pytest.raises(ValueError, match="contiguous"):
        normals.depth_to_normal(dev(depth).t(), cam)


def test_hand_placed_maps_on_the_device():
    W, H = 9, 7
    nr, alpha, weight, g = nc.loss_maps(W, H)
    depth = nc.depth_maps(W, H)["noisy"]
    depth[3, 4] = np.nan
    assert same(hip_depth_normals(dev(depth)).cpu().numpy(), nc.harness_depth_normals(depth))
    d_nr, d_depth = hip_loss_bwd(dev(nr), dev(depth), dev(alpha), dev(weight))
    assert bool(torch.isfinite(d_nr).all()) and bool(torch.isfinite(d_depth).all()) and float(d_depth[3, 4]) == 0
    zero = np.zeros((H, W), np.float32)
    depth = nc.depth_maps(W, H)["plane"]
    assert float(hip_loss(dev(nr), dev(depth), dev(alpha), dev(zero))[0]) == 1.0
    d_nr, d_depth = hip_loss_bwd(dev(nr), dev(depth), dev(alpha), dev(zero))
    assert not bool(d_nr.any()) and not bool(d_depth.any())
    nd = hip_depth_normals(dev(np.full((H, W), 3.25, np.float32)))
    assert bool((nd[:, 1:-1, 1:-1] == torch.tensor([0.0, 0.0, -1.0], device=DEV)[:, None, None]).all())


# ---- determinism and memory -----------------------------------------------------------------------------------------------------
def test_two_streams_give_the_same_bits():
    """Every entry point twice, on two streams, into poisoned outputs and poisoned scratch: the same bits."""
    N, (W, H) = 257, (70, 45)
    xyz, sc, q = nc.rows_inputs(N)
    vm = nc.view_matrix(nc.cameras()[0])
    depth = nc.depth_maps(W, H)["noisy"]
    nr, alpha, weight, g = nc.loss_maps(W, H)
    grow = np.random.RandomState(3).randn(N, 4).astype(np.float32)
    t = {k: dev(v) for k, v in dict(xyz=xyz, sc=sc, q=q, vm=vm, depth=depth, nr=nr, alpha=alpha, weight=weight, g=g, grow=grow).items()}
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream(DEV)
        with torch.cuda.stream(s):          # the poison fills and the upstream scalar are made on the stream the kernels run on
            out = [hip_rows(t["xyz"], t["sc"], t["q"], t["vm"]), *hip_rows_bwd(t["xyz"], t["sc"], t["q"], t["vm"], t["grow"]),
                   hip_depth_normals(t["depth"]), hip_depth_normals_bwd(t["depth"], t["g"]),
                   *hip_loss(t["nr"], t["depth"], t["alpha"], t["weight"]), *hip_loss_bwd(t["nr"], t["depth"], t["alpha"], t["weight"])]
            assert stream_arg().value == s.cuda_stream
        s.synchronize()
        runs.append([bits(o) for o in out])
    for k, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a, b), f"output {k} differs between the two streams"
        assert np.isfinite(a.view(np.float32)).all(), f"output {k} kept poisoned words"


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    lib = normals.load()
    N, W, H = 8, 6, 5
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    xyz, sc, q, vm, rows, g = f(N, 3), f(N, 3), f(N, 4), f(16), f(N, 4), f(N, 4)
    depth, nd, nr, alpha, loss, one = f(H, W), f(3, H, W), f(3, H, W), f(H, W), f(1), f(1)
    scratch = _lib.scratch(lib.lg_normal_loss_scratch_bytes(H, W), DEV)
    st = stream_arg()
    odd = C.c_void_p(depth.data_ptr() + 2)
    nan = float("nan")

    def refused(rc, word):
        assert rc == _lib.LG_ERR_INVALID_ARGUMENT
        msg = lib.lg_last_error().decode()
        assert word in msg, msg

    rows_args = [p(xyz), p(sc), p(q), p(vm), p(rows)]
    for k, name in enumerate(("xyz", "scaling", "rotation", "viewmatrix", "rows")):
        for bad, word in ((None, "null " + name), (odd, name + " must be 4-byte aligned")):
            a = list(rows_args); a[k] = bad
            refused(lib.lg_normal_rows(N, *a, 0, st), word)
    bwd_args = [p(xyz), p(sc), p(q), p(vm), p(g), p(xyz.clone()), p(q.clone())]
    for k, name in enumerate(("xyz", "scaling", "rotation", "viewmatrix", "dL_drows", "dL_dxyz", "dL_drotation")):
        for bad, word in ((None, "null " + name), (odd, name + " must be 4-byte aligned")):
            a = list(bwd_args); a[k] = bad
            refused(lib.lg_normal_rows_bwd(N, *a, 0, st), word)
    for bad_n in (-1, 1 << 30):
        refused(lib.lg_normal_rows(bad_n, *rows_args, 0, st), "N outside")
        refused(lib.lg_normal_rows_bwd(bad_n, *bwd_args, 0, st), "N outside")
    # N == 0: LG_OK, nothing launched, the outputs untouched
    keep = poisoned(N, 4)
    assert lib.lg_normal_rows(0, p(xyz), p(sc), p(q), p(vm), p(keep), 0, st) == _lib.LG_OK
    assert lib.lg_normal_rows_bwd(0, *bwd_args, 0, st) == _lib.LG_OK
    torch.cuda.synchronize()
    assert bool((keep.view(torch.int32) == -1).all())

    calls = {
        "lg_depth_normals": lambda h, w, tx, ty, a: lib.lg_depth_normals(h, w, a[0], tx, ty, a[1], 0, st),
        "lg_depth_normals_bwd": lambda h, w, tx, ty, a: lib.lg_depth_normals_bwd(h, w, a[0], tx, ty, a[1], a[2], 0, st),
        "lg_normal_loss": lambda h, w, tx, ty, a: lib.lg_normal_loss(h, w, a[0], a[1], a[2], a[3], tx, ty, a[4], a[5], a[6], 0, st),
        "lg_normal_loss_bwd": lambda h, w, tx, ty, a: lib.lg_normal_loss_bwd(h, w, a[0], a[1], a[2], a[3], tx, ty, a[4], a[5], a[6], 0, st),
    }
    args = {
        "lg_depth_normals": ([p(depth), p(nd)], ("depth", "normals"), ()),
        "lg_depth_normals_bwd": ([p(depth), p(nd), p(alpha)], ("depth", "dL_dnormals", "dL_ddepth"), ()),
        "lg_normal_loss": ([p(nr), p(depth), p(alpha), p(alpha.clone()), p(loss), p(nd), p(scratch)],
                           ("normal_map", "depth", "alpha", "weight", "loss", "depth_normals", "scratch"), ("weight", "depth_normals")),
        "lg_normal_loss_bwd": ([p(nr), p(depth), p(alpha), p(alpha.clone()), p(one), p(nd), p(depth.clone())],
                               ("normal_map", "depth", "alpha", "weight", "dL_dloss", "dL_dnormal_map", "dL_ddepth"), ("weight",)),
    }
    for fn, call in calls.items():
        base, names, optional = args[fn]
        assert call(H, W, TX, TY, base) == _lib.LG_OK, fn
        for h, w, word in ((0, W, "H outside"), (-3, W, "H outside"), (H, 0, "W outside"), (H, 32769, "W outside"), (32769, W, "H outside")):
            refused(call(h, w, TX, TY, base), word)
        refused(call(H, W, nan, TY, base), "tanfovx is NaN")
        refused(call(H, W, TX, nan, base), "tanfovy is NaN")
        for k, name in enumerate(names):
            a = list(base); a[k] = odd
            refused(call(H, W, TX, TY, a), name + " must be 4-byte aligned")
            a = list(base); a[k] = None
            if name in optional:
                assert call(H, W, TX, TY, a) == _lib.LG_OK, (fn, name)
            else:
                refused(call(H, W, TX, TY, a), "null " + name)
        assert fn in lib.lg_last_error().decode()
    assert lib.lg_normal_loss_scratch_bytes(0, W) == 0 and lib.lg_normal_loss_scratch_bytes(H, -1) == 0
    torch.cuda.synchronize()


def test_profile_names():
    W, H = 33, 17
    depth, (nr, alpha, weight, g) = nc.depth_maps(W, H)["noisy"], nc.loss_maps(W, H)
    xyz, sc, q = nc.rows_inputs(65)
    cam = nc.cameras()[0].to(DEV)
    _lib.profile_reset()
    normals.set_profile(True)
    try:
        x, r = dev(xyz).requires_grad_(), dev(q).requires_grad_()
        normals.gaussian_normals(x, dev(sc), r, cam).sum().backward()
        d, n = dev(depth).requires_grad_(), dev(nr).requires_grad_()
        normals.depth_to_normal(d, nc.Camera()).sum().backward()
        normals.normal_consistency_loss(n, d, dev(alpha), nc.Camera(), weight=dev(weight)).backward()
        torch.cuda.synchronize()
    finally:
        normals.set_profile(False)
    seen = _lib.profile_read()
    for name in ("normal_rows", "normal_rows_bwd", "depth_normals", "depth_normals_bwd", "normal_loss", "normal_loss_reduce", "normal_loss_bwd"):
        assert seen.get(name, (0, 0))[1] == 1, (name, seen)
    _lib.profile_reset()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
LAMBDA = 0.7
_E2E = {}


def e2e_scene(name):
    """The scene with its rows outside the decision margins of every Gaussian (nudged in this copy if one is not)."""
    c, g, cam = fg.scene(name)
    vm = nc.view_matrix(cam)
    xyz, sc, q = (getattr(g, n).detach().numpy().copy() for n in ("_xyz", "_scaling", "_rotation"))
    keep = nc.keep_rows(xyz, sc, q, vm)[3]
    if not keep.all():
        bad = np.nonzero(~keep)[0]
        sc[bad, np.argmin(sc[bad], axis=1)] -= 1e-3                  # widen the scale gap ...
        xyz[bad] += np.float32(1e-2)                                  # ... and move the point off the plane of the disc
        g._xyz, g._scaling = torch.from_numpy(xyz), torch.from_numpy(sc)
    assert nc.keep_rows(xyz, sc, q, vm)[3].all(), f"{name}: a row lies within a decision margin"
    return c, g, cam


def e2e_reference(name):
    """{dtype name: {raw parameter: gradient}} of LAMBDA * loss(normal, depth, alpha, weight = mask) + sum(normal * gimg) by the dense
    twin: two renders of colors_precomp -- the twin's normal triple, and (z, 1, 0) -- from the raw parameters; "mask": alpha64 >= 1e-3;
    "maps": the float64 normal, depth, alpha.  Computed once per scene."""
    if name in _E2E:
        return _E2E[name]
    c, g, cam = e2e_scene(name)
    W, H, N = c["W"], c["H"], c["N"]
    kw = common.scene_kwargs(g, cam, W, H, precolor=torch.zeros(N, 3), as_torch=True)
    gimg = torch.from_numpy(np.random.RandomState(23).randn(3, H, W))
    tx, ty = kw["tanfovx"], kw["tanfovy"]
    _r, k64, s64, _gap, _ndp = nc.rows_twin(*(getattr(g, n).double() for n in ("_xyz", "_scaling", "_rotation")), cam.world_view_transform.double())
    out, mask = {}, None
    for dd, dname in dense_twin.DTYPES:
        raw = {n: getattr(g, n).to(dd).detach().clone().requires_grad_() for n in fg.RAW}
        rows = nc.rows_twin(raw["_xyz"], raw["_scaling"], raw["_rotation"], cam.world_view_transform.to(dd), k=k64, s=s64.to(dd))[0]
        act = dict(means3D=raw["_xyz"], opacities=torch.sigmoid(raw["_opacity"]), scales=torch.exp(raw["_scaling"]),
                   rotations=torch.nn.functional.normalize(raw["_rotation"]))
        z = rows[:, 3:4]
        normal = dense_twin.render(kw, dd, leaves=dict(act, colors_precomp=rows[:, :3]), front_only=False)[0]
        second = dense_twin.render(kw, dd, leaves=dict(act, colors_precomp=torch.cat([z, torch.ones_like(z), torch.zeros_like(z)], 1)), front_only=False)[0]
        alpha = second[1]
        depth = second[0] / alpha.clamp_min(1e-6)
        if mask is None:
            mask = (alpha.detach() >= 1e-3).to(torch.float64)
        loss = nc.loss_twin(normal, depth, alpha, mask.to(dd), tx, ty)
        (LAMBDA * loss + (normal * gimg.to(dd)).sum()).backward()
        out[dname] = {n: raw[n].grad.numpy().astype(np.float64) for n in fg.RAW}
        out[dname]["loss"] = float(loss.detach())
        if dd == torch.float64:
            out["maps"] = (normal.detach().numpy(), depth.detach().numpy(), alpha.detach().numpy())
    out["mask"], out["gimg"] = mask.numpy().astype(np.float32), gimg.numpy().astype(np.float32)
    _E2E[name] = out
    return out


@pytest.mark.parametrize("name", ("N300_70x45", "N64_33x17"))
def test_render_geometry_and_the_loss_against_the_dense_twin(name):
    ref = e2e_reference(name)
    c, g, cam = e2e_scene(name)
    W, H, N = c["W"], c["H"], c["N"]
    pipe = syn.PipelineParams()
    model = g.to(DEV)
    for n in fg.RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    camd = cam.to(DEV)
    opts = {"fast_exp": False}
    pkg = render_geometry(camd, model, pipe, options=opts)
    assert set(pkg) == {"render", "alpha", "normal", "depth", "radii", "visibility_filter", "viewspace_points"}
    assert pkg["normal"].shape == (3, H, W) and pkg["depth"].shape == (H, W) and pkg["alpha"].shape == (H, W)
    mask = dev(ref["mask"])
    loss = normals.normal_consistency_loss(pkg["normal"], pkg["depth"], pkg["alpha"], camd, weight=mask)
    (LAMBDA * loss + (pkg["normal"] * dev(ref["gimg"])).sum()).backward()
    n64, d64, a64 = ref["maps"]
    ok = ref["mask"] > 0
    en, ea = np.abs(pkg["normal"].detach().cpu().numpy() - n64).max(), np.abs(pkg["alpha"].detach().cpu().numpy() - a64).max()
    # maps: the 1e-5 of a float32 render against the float64 one (|N_r| <= 1, alpha in [0, 1]); depth: fg.assert_depth_maps' first-order
    # bound through the quotient, (1e-5 max |num| + 1e-5 |depth|) / alpha, where alpha >= 1e-3
    scale = np.abs(d64 * np.maximum(a64, 1e-6)).max()
    dbound = 1.01 * (1e-5 * scale + np.abs(d64) * 1e-5) / np.maximum(a64, 1e-3)
    ed = (np.abs(pkg["depth"].detach().cpu().numpy() - d64)[ok] / dbound[ok]).max()
    print(f"{name}: normal map error {en:.3e}, alpha {ea:.3e}, depth error {ed:.3f} x its bound where alpha >= 1e-3; {int(ok.sum())} pixels")
    assert en <= 1e-5 and ea <= 1e-5 and ed <= 1.0 and ok.sum() > 100
    print(f"{name}: loss {float(loss.detach()):.7f}, float64 twin {ref['float64']['loss']:.7f}, float32 twin {ref['float32']['loss']:.7f}")
    assert abs(float(loss.detach()) - ref["float64"]["loss"]) <= max(1e-4 * abs(ref["float64"]["loss"]), 3 * abs(ref["float32"]["loss"] - ref["float64"]["loss"]))
    got = {}
    for n in fg.RAW:
        v = getattr(model, n).grad
        assert v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, n
        got[n] = v.cpu().numpy()
    for n in fg.RAW:
        tolerance.assert_rule3(got[n], ref["float64"][n], ref["float32"][n], f"{name} {n}")
    assert pkg["viewspace_points"].grad is not None

    # the maps against render_features on the same forward inputs
    with torch.no_grad():
        rows = normals.gaussian_normals(model.get_xyz, model.get_scaling, model.get_rotation, camd)
        triple = render_features(camd, model, pipe, rows[:, :3].contiguous(), options=opts)
        dep = render_features(camd, model, pipe, "depth", options=opts)
    assert np.array_equal(bits(triple["features"]), bits(pkg["normal"])), "normal differs from render_features of the same three columns"
    assert np.array_equal(bits(dep["alpha"]), bits(pkg["alpha"]))
    # depth: the two z evaluations (torch's matmul there, lg_view_point here) are each within 4 u Z of the exact z, Z = max_j (|xyz_j| .
    # |vm[:3, 2]| + |vm[3, 2]|); the blend is the same operation sequence on both, linear in z with weights summing to alpha, and rounds
    # each of its L + 1 partial sums and the quotient once per run: |depth_a - depth_b| <= (8 + 2 (L + 2)) u Z, L <= N contributors
    vmn = nc.view_matrix(cam).astype(np.float64)
    Z = float((np.abs(model.get_xyz.detach().cpu().numpy().astype(np.float64)) @ np.abs(vmn[:3, 2]) + abs(vmn[3, 2])).max())
    diff = float((dep["depth"][0] - pkg["depth"].detach())[torch.from_numpy(ok).to(DEV)].abs().max())
    bound = (8 + 2 * (N + 2)) * nc.U * Z
    print(f"{name}: depth against render_features('depth'): {diff:.3e} (bound {bound:.3e}, Z {Z:.3f})")
    assert diff <= bound
