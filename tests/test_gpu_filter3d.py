"""-m gpu: the 3D smoothing filter on the device (lg_filter3d_update / _apply / _apply_bwd, lightgaussian_amd/filter3d.py, and the
"filter_3d" option of gaussian_renderer).  References and shapes: tests/filter3d_common.py.

4. lg_filter3d_update: filter and seen are BIT-IDENTICAL to the g++ build of the same lg_math.h text (fma, correctly rounded divide,
   compares, min / max only), over every row; unseen rows get the maximum, nobody seen gives zeros, two streams give the same bits.
5. lg_filter3d_apply in both domains against float64, in the activated domain (exp(r'), sigmoid(o')):
       elementwise relative error <= max(4 err32, 2^-20),   err32 = the float32 torch formula's own error on the same rows
   (the device's expf / logf may be 1-2 ulp where the host's are below 1); hand-placed rows; lg_filter3d_apply_bwd against float64
   autograd by the rule of tests/camera_grad_common.py:  rel_err(got, d64) <= max(1e-4, 3 rel_err(d32, d64)).
   Every figure is printed before it is asserted; the measured ones are in DESIGN.md section 10.6.
6. End to end on "N300_70x45" and "N64_33x17": render() of a model with filter_3D equals, bit for bit, a plain render() of a model
   whose raw tensors are the apply kernel's outputs -- image, radii, visibility_filter, and every raw-parameter gradient (the second
   model's graph runs lg_filter3d_apply_bwd behind its rasterizer backward); the raw gradients also meet the dense float64 twin with
   s' = sqrt(s^2 + f^2), sigma' = sigma c, canonical and hardware-exp; the same bit-identity for count_render, render_features and the
   unfused path.
7. Off = absent: an all-zero filter, options={"filter_3d": False} and a model without the attribute give the same bits;
   fuse_filter_3d + a plain render equals the filtered render."""
import ctypes as C

import numpy as np
import pytest
import torch

import antialias_common as aa
import camera_grad_common as cg
import features_geom_common as fg
import filter3d_common as fc
from common import bits as _bits
from common import syn
from lightgaussian_amd import _lib, filter3d, gaussian_renderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENES = ("N300_70x45", "N64_33x17")
RAW = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")


def _same(a, b):
    if a.dtype.is_floating_point:
        return np.array_equal(_bits(a), _bits(b))
    return torch.equal(a, b)


# ---- 4. lg_filter3d_update -----------------------------------------------------------------------------------------------------
def _update(means, V, W, H, stream=None):
    table = filter3d.camera_table(fc.cameras(V, W, H))
    xyz = torch.from_numpy(means).to(DEV)
    if stream is None:
        f, seen = filter3d.compute_filter_3d(xyz, table, return_seen=True)
    else:
        with torch.cuda.stream(stream):
            f, seen = filter3d.compute_filter_3d(xyz, table, return_seen=True)
        stream.synchronize()
    torch.cuda.synchronize()
    assert tuple(f.shape) == (means.shape[0], 1) and f.dtype == torch.float32 and seen.dtype == torch.bool
    return f.cpu().numpy().reshape(-1), seen.cpu().numpy()


@pytest.mark.parametrize("size", fc.SIZES)
@pytest.mark.parametrize("V", fc.VS)
@pytest.mark.parametrize("N", fc.NS)
def test_update_is_bit_identical_to_the_harness(N, V, size):
    W, H = size
    means, rows = fc.points(N, V, W, H)
    want = fc.run_harness(means, rows)
    f, seen = _update(means, V, W, H)
    assert np.array_equal(seen, want["seen"])
    assert np.array_equal(_bits(f), _bits(want["filter"]))


def test_update_unseen_rows_nobody_seen_and_two_streams():
    means, rows = fc.points(1000, 3, 70, 45)
    f, seen = _update(means, 3, 70, 45)
    assert seen.any() and not seen.all()
    top = f[seen].max()
    assert top > 0 and (f[~seen] == top).all()
    away = np.ascontiguousarray(means[~seen])
    f0, s0 = _update(away, 3, 70, 45)
    assert not s0.any() and not _bits(f0).any()
    fa, sa = _update(means, 3, 70, 45, torch.cuda.Stream())
    fb, sb = _update(means, 3, 70, 45, torch.cuda.Stream())
    assert np.array_equal(_bits(fa), _bits(f)) and np.array_equal(_bits(fb), _bits(f)) and np.array_equal(sa, seen) and np.array_equal(sb, seen)
    # without the seen output, and through camera objects instead of a table
    g = filter3d.compute_filter_3d(torch.from_numpy(means).to(DEV), fc.cameras(3, 70, 45))
    assert np.array_equal(_bits(g.reshape(-1)), _bits(f))


def test_update_argument_checks():
    lib = _lib.load()
    x = torch.zeros(4, 3, device=DEV)
    t = filter3d.camera_table(fc.cameras(1, 33, 17)).to(DEV)
    out = torch.zeros(4, device=DEV)
    sc = torch.zeros(lib.lg_filter3d_scratch_bytes(4), dtype=torch.uint8, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731  (not common.ptr: the device pointer of a tensor)
    assert lib.lg_filter3d_update(-1, p(x), 1, p(t), p(out), None, p(sc), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_filter3d_update(1 << 30, p(x), 1, p(t), p(out), None, p(sc), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_filter3d_update(4, p(x), 0, p(t), p(out), None, p(sc), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_filter3d_update(4, None, 1, p(t), p(out), None, p(sc), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_filter3d_apply(4, None, p(out), p(out), p(x), p(out), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_filter3d_apply_bwd(-1, p(x), p(out), p(out), p(x), p(out), p(x), p(out), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_filter3d_update(0, p(x), 1, p(t), p(out), None, p(sc), 0, None) == _lib.LG_OK
    e = torch.zeros(0, 3, device=DEV)
    assert tuple(filter3d.compute_filter_3d(e, t).shape) == (0, 1)


# ---- 5. lg_filter3d_apply / _bwd -----------------------------------------------------------------------------------------------
def _apply(a_s, a_o, f, raw):
    fn = filter3d.apply_filter_3d if raw else filter3d.apply_filter_3d_activated
    return fn(a_s.to(DEV), a_o.to(DEV), f.to(DEV))


def _off(t):
    """A device copy of t whose address is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    buf[1:] = t.reshape(-1).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[1:].view(t.shape)


def _apply_bwd(place, a_s, a_o, f, gs, go, raw):
    """lg_filter3d_apply_bwd called directly on place(tensor) of all seven tensors; (dL/dscaling, dL/dopacity) on the CPU."""
    ins = [place(t) for t in (a_s, a_o, f, gs, go)]
    outs = [place(torch.full_like(a_s, float("nan"))), place(torch.full_like(a_o, float("nan")))]
    _lib.check(_lib.load().lg_filter3d_apply_bwd(a_s.shape[0], *(_lib.ptr(t) for t in ins + outs), _lib.FILTER3D_RAW if raw else 0, _lib.stream()))
    torch.cuda.synchronize()
    return outs[0].cpu(), outs[1].cpu()


# the row counts below 8 are the branches of the four-rows-per-lane walk: a tail alone (1 - 3), one full lane (4), a full lane and a tail (5, 7)
@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("N", fc.NS + (2, 3, 4, 5, 7))
def test_apply_against_float64(N, raw):
    e = fc.err32(N, raw)
    a_s, a_o, f = e["inputs"]
    out_s, out_o = _apply(a_s, a_o, f, raw)
    assert out_s.shape == a_s.shape and out_o.shape == a_o.shape
    got = fc.activated(out_s, out_o, raw)
    for k, n in enumerate(("scaling", "opacity")):
        err, bound = fc.rel_elem(got[k], e["ref"][k]), max(4.0 * e[n], 2.0 ** -20)
        print(f"N{N} raw={raw} {n}: relative error {err:.3e} (err32 {e[n]:.3e}, bound {bound:.3e})")
        assert err <= bound
    zero = (f == 0).reshape(-1)
    assert zero.any() or N < 4
    assert np.array_equal(_bits(out_s.cpu()[zero]), _bits(a_s[zero])) and np.array_equal(_bits(out_o.cpu()[zero]), _bits(a_o[zero]))
    # pointers off 16 bytes take the dword path: same bits
    m_s, m_o = _apply(_off(a_s), _off(a_o), _off(f), raw)
    assert np.array_equal(_bits(m_s), _bits(out_s)) and np.array_equal(_bits(m_o), _bits(out_o))


def test_apply_hand_placed_rows():
    ls = float(np.log(0.05))
    r = torch.tensor([[ls, ls - 1, ls + 1],         # 0  f == 0: bit copy
                      [ls, ls, ls],                 # 1  f a thousand times the scale: c ~ 1e-9
                      [-30.0, -30.0, -30.0],        # 2  y underflows to 0: -inf, rendered opacity 0
                      [ls, ls + 0.5, ls - 0.5]])    # 3  logit +15
    o = torch.tensor([[0.3], [2.0], [-80.0], [15.0]])
    f = torch.tensor([[0.0], [50.0], [1.0e6], [0.02]])
    out_s, out_o = _apply(r, o, f, True)
    out_s, out_o = out_s.cpu(), out_o.cpu()
    assert np.array_equal(_bits(out_s[0]), _bits(r[0])) and np.array_equal(_bits(out_o[0]), _bits(o[0]))
    ref_s, ref_o = fc.apply_formula(r.double(), o.double(), f.double(), True)
    c1 = float(torch.sigmoid(out_o[1].double()) / torch.sigmoid(o[1].double()))
    assert 0.5e-9 < c1 < 2e-9 and abs(c1 / 1e-9 - 1) < 1e-3                                 # (0.05 / 50)^3
    assert abs(float(torch.exp(out_s[1, 0].double())) / 50.0 - 1) < 1e-6
    assert out_o[2].item() == float("-inf") and torch.sigmoid(out_o[2]).item() == 0.0
    assert torch.isfinite(out_s[2]).all()
    assert torch.isfinite(out_o[3]).all()
    assert abs(torch.sigmoid(out_o[3].double()).item() / torch.sigmoid(ref_o[3]).item() - 1) <= 2.0 ** -20
    assert fc.rel_elem(torch.exp(out_s[3].double()).numpy(), torch.exp(ref_s[3]).numpy()) <= 2.0 ** -20
    # the row with -inf renders as nothing: K1's sigmoid gives opacity 0
    g = syn.make_gaussians(1, seed=1)
    cam = syn.orbit_camera(0, 4, 33, 17)
    one = syn.SyntheticGaussians(torch.zeros(1, 3), g._features_dc, g._features_rest, out_s[2:3].clone(), g._rotation, out_o[2:3].clone(), 3, 3)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    pkg = gaussian_renderer.render(cam.to(DEV), one.to(DEV), syn.PipelineParams(), bg)
    assert torch.equal(pkg["render"], bg[:, None, None].expand(3, 17, 33))


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("N", [65, 1000, 3, 4, 5])
def test_apply_backward_against_float64_autograd(N, raw):
    ref = fc.grad_reference(N, raw)
    a_s, a_o, f = fc.err32(N, raw)["inputs"]
    gs, go = fc.upstream_gradients(N)
    s, o = a_s.to(DEV).requires_grad_(), a_o.to(DEV).requires_grad_()
    out_s, out_o = (filter3d.apply_filter_3d if raw else filter3d.apply_filter_3d_activated)(s, o, f.to(DEV))
    ((out_s * gs.to(DEV)).sum() + (out_o * go.to(DEV)).sum()).backward()
    aa.assert_rule({"scaling": s.grad.cpu().numpy(), "opacity": o.grad.cpu().numpy()}, ref, ("scaling", "opacity"), f"N{N} raw={raw}")
    zero = (f == 0).reshape(-1)
    assert np.array_equal(_bits(s.grad.cpu()[zero]), _bits(gs[zero])) and np.array_equal(_bits(o.grad.cpu()[zero]), _bits(go[zero]))
    # all seven tensors off 16 bytes take the dword path: the same bits as the aligned call, which is the one behind autograd
    d_s, d_o = _apply_bwd(lambda t: t.to(DEV), a_s, a_o, f, gs, go, raw)
    assert np.array_equal(_bits(d_s), _bits(s.grad.cpu())) and np.array_equal(_bits(d_o), _bits(o.grad.cpu()))
    m_s, m_o = _apply_bwd(_off, a_s, a_o, f, gs, go, raw)
    assert np.array_equal(_bits(m_s), _bits(d_s)) and np.array_equal(_bits(m_o), _bits(d_o))
    # only one output differentiated: the other incoming gradient counts as zero
    s2, o2 = a_s.to(DEV).requires_grad_(), a_o.to(DEV).requires_grad_()
    only_s, _unused = (filter3d.apply_filter_3d if raw else filter3d.apply_filter_3d_activated)(s2, o2, f.to(DEV))
    (only_s * gs.to(DEV)).sum().backward()
    assert torch.isfinite(s2.grad).all() and (o2.grad is None or not o2.grad.any())


# ---- 6. / 7. end to end ----------------------------------------------------------------------------------------------------------
def _scene(name):
    g, cam, W, H = cg.small_scene(name)
    f = filter3d.compute_filter_3d(g._xyz.to(DEV), fc.cameras(3, W, H))          # camera 0 of the set is the scene's own
    torch.cuda.synchronize()
    return g, cam, W, H, f


def _leafed(g, filter_3d=None):
    m = g.to(DEV)
    for n in RAW:
        setattr(m, n, getattr(m, n).detach().clone().requires_grad_(True))
    if filter_3d is not None:
        m.filter_3D = filter_3d
    return m


def _prefiltered(g, f):
    """A model without the attribute whose _scaling / _opacity are the raw apply's outputs, attached to leaves of their own."""
    m = _leafed(g)
    leaves = {n: getattr(m, n) for n in RAW}
    m._scaling, m._opacity = filter3d.apply_filter_3d(leaves["_scaling"], leaves["_opacity"], f)
    return m, leaves


def _grads(leaves):
    return {n: leaves[n].grad for n in RAW}


@pytest.mark.parametrize("fast_exp", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_fused_render_equals_a_plain_render_of_the_filtered_tensors(name, fast_exp):
    g, cam, W, H, f = _scene(name)
    assert float((f > 0).float().mean()) == 1.0
    gimg, bg, pipe = cg.image_gradient(H, W).to(DEV), torch.tensor(cg.BG, device=DEV), syn.PipelineParams()
    opts = {"fast_exp": fast_exp}
    a = _leafed(g, f)
    pa = gaussian_renderer.render(cam.to(DEV), a, pipe, bg, options=opts)
    assert "Raw" in type(pa["render"].grad_fn).__name__                                     # the fused path stays
    (pa["render"] * gimg).sum().backward()
    b, leaves = _prefiltered(g, f)
    pb = gaussian_renderer.render(cam.to(DEV), b, pipe, bg, options=opts)
    (pb["render"] * gimg).sum().backward()
    torch.cuda.synchronize()
    for k in ("render", "radii", "visibility_filter"):
        assert _same(pa[k], pb[k]), k
    assert pa["visibility_filter"].any()
    for n in RAW:
        assert _same(getattr(a, n).grad, leaves[n].grad), n
    assert _same(pa["viewspace_points"].grad, pb["viewspace_points"].grad)
    # the filter changes the picture (scales of ~0.05 against filters of ~0.03)
    plain = gaussian_renderer.render(cam.to(DEV), _leafed(g), pipe, bg, options=opts)
    assert not _same(plain["render"], pa["render"])


_TWIN = {}


def _twin_reference(name, g, f, kw, gimg):
    if name in _TWIN:
        return _TWIN[name]
    out = {}
    for dd in (torch.float64, torch.float32):
        raw = {n: getattr(g, n).to(dd).detach().clone().requires_grad_() for n in RAW}
        s, sig, fd = torch.exp(raw["_scaling"]), torch.sigmoid(raw["_opacity"]), f.cpu().to(dd)
        s2, sig2 = fc.apply_formula(s, sig, fd, False)                                        # s' = sqrt(s^2 + f^2), sigma' = sigma c
        act = dict(means3D=raw["_xyz"], opacities=sig2, scales=s2, rotations=torch.nn.functional.normalize(raw["_rotation"]),
                   shs=torch.cat([raw["_features_dc"], raw["_features_rest"]], 1))
        k2 = dict(kw)
        k2.update(act)
        (cg.dense_render(k2, dd) * gimg.to(dd)).sum().backward()
        out["float64" if dd == torch.float64 else "float32"] = {n: raw[n].grad.numpy().astype(np.float64) for n in RAW}
    _TWIN[name] = out
    return out


@pytest.mark.parametrize("fast_exp", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_raw_gradients_against_the_dense_twin(name, fast_exp):
    g, cam, W, H, f = _scene(name)
    kw = cg.combo_kwargs(g, cam, W, H, "sh3")
    gimg = cg.image_gradient(H, W)
    ref = _twin_reference(name, g, f, kw, gimg)
    a = _leafed(g, f)
    pkg = gaussian_renderer.render(cam.to(DEV), a, syn.PipelineParams(), torch.tensor(cg.BG, device=DEV), options={"fast_exp": fast_exp})
    (pkg["render"] * gimg.to(DEV)).sum().backward()
    aa.assert_rule({n: getattr(a, n).grad.cpu().numpy() for n in RAW}, ref, RAW, f"{name} fast_exp={fast_exp}")


class _Getters:
    """A model of foreign getters: the base model's, with get_scaling / get_opacity replaced by given tensors (no raw fields, so
    render() takes the unfused path)."""

    def __init__(self, base, scales, opacity):
        self._base, self.get_scaling, self.get_opacity = base, scales, opacity
        self.active_sh_degree, self.max_sh_degree = base.active_sh_degree, base.max_sh_degree

    get_xyz = property(lambda self: self._base.get_xyz)
    get_rotation = property(lambda self: self._base.get_rotation)
    get_features = property(lambda self: self._base.get_features)


def _activated_pair(g, f):
    """(model with the filter, leaves) and (a foreign-getter model over the activated apply's outputs, its leaves)."""
    a = _leafed(g, f)
    base = _leafed(g)
    s, o = filter3d.apply_filter_3d_activated(base.get_scaling, base.get_opacity, f)
    return a, {n: getattr(a, n) for n in RAW}, _Getters(base, s, o), {n: getattr(base, n) for n in RAW}


@pytest.mark.parametrize("name", SCENES)
def test_unfused_count_and_feature_paths_equal_plain_calls_of_the_filtered_tensors(name):
    g, cam, W, H, f = _scene(name)
    camd, bg, pipe = cam.to(DEV), torch.tensor(cg.BG, device=DEV), syn.PipelineParams()
    gimg = cg.image_gradient(H, W).to(DEV)
    # the unfused path
    a, la, b, lb = _activated_pair(g, f)
    pa = gaussian_renderer.render(camd, a, pipe, bg, options={"fuse_getters": False, "fast_exp": False})
    pb = gaussian_renderer.render(camd, b, pipe, bg, options={"fast_exp": False})
    assert "Raw" not in type(pa["render"].grad_fn).__name__
    (pa["render"] * gimg).sum().backward()
    (pb["render"] * gimg).sum().backward()
    for k in ("render", "radii", "visibility_filter"):
        assert _same(pa[k], pb[k]), k
    for n in RAW:
        assert _same(la[n].grad, lb[n].grad), n
    # count_render: counts and scores
    with torch.no_grad():
        a, la, b, lb = _activated_pair(g, f)
        ca, cb = gaussian_renderer.count_render(camd, a, pipe, bg), gaussian_renderer.count_render(camd, b, pipe, bg)
    for k in ("render", "radii", "gaussians_count", "important_score"):
        assert _same(ca[k], cb[k]), k
    assert int(ca["gaussians_count"].sum()) > 0
    # render_features("depth", geometry_grad=True)
    a, la, b, lb = _activated_pair(g, f)
    gd, ga = (torch.from_numpy(m).float().to(DEV) for m in fg.depth_loss_maps(H, W))
    fa = gaussian_renderer.render_features(camd, a, pipe, "depth", geometry_grad=True, options={"fast_exp": False})
    fb = gaussian_renderer.render_features(camd, b, pipe, "depth", geometry_grad=True, options={"fast_exp": False})
    (fa["depth"] * gd + fa["alpha"] * ga).sum().backward()
    (fb["depth"] * gd + fb["alpha"] * ga).sum().backward()
    for k in ("features", "alpha", "depth", "render", "radii"):
        assert _same(fa[k], fb[k]), k
    for n in ("_xyz", "_opacity", "_scaling", "_rotation"):
        assert _same(la[n].grad, lb[n].grad), n
    torch.cuda.synchronize()


@pytest.mark.parametrize("fast_exp", [False, True])
def test_off_equals_absent_and_fuse_equals_the_filtered_render(fast_exp):
    name = "N300_70x45"
    g, cam, W, H, f = _scene(name)
    camd, bg, pipe = cam.to(DEV), torch.tensor(cg.BG, device=DEV), syn.PipelineParams()
    gimg = cg.image_gradient(H, W).to(DEV)

    def run(model, options):
        pkg = gaussian_renderer.render(camd, model, pipe, bg, options=dict(options, fast_exp=fast_exp))
        (pkg["render"] * gimg).sum().backward()
        return pkg, {n: getattr(model, n).grad for n in RAW}

    absent = run(_leafed(g), {})
    zeros = run(_leafed(g, torch.zeros_like(f)), {})
    off = run(_leafed(g, f), {"filter_3d": False})
    for other in (zeros, off):
        for k in ("render", "radii", "visibility_filter"):
            assert _same(absent[0][k], other[0][k]), k
        for n in RAW:
            assert _same(absent[1][n], other[1][n]), n
    # fuse: a model that carries the fused tensors and no filter renders what the filtered model renders
    on = run(_leafed(g, f), {})
    fs, fo = filter3d.fuse_filter_3d(_leafed(g, f))
    assert not fs.requires_grad and not fo.requires_grad
    fused = g.to(DEV)
    fused._scaling, fused._opacity = fs, fo
    with torch.no_grad():
        pf = gaussian_renderer.render(camd, fused, pipe, bg, options={"fast_exp": fast_exp})
    for k in ("render", "radii", "visibility_filter"):
        assert _same(on[0][k], pf[k]), k
    assert not _same(on[0]["render"], absent[0]["render"])
    torch.cuda.synchronize()
