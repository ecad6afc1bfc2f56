"""Shared by tests/test_features_geom_host.py and tests/test_gpu_features_geom.py (test infrastructure): the scenes, the reference for
the geometry gradient of a loss on feature / alpha / colour maps -- the oracle's own backward, summed over channel triples -- the
tolerance rule of tests/test_gpu_parity.py::test_backward_parity, and the g++ build of tests/cpu_harness/lg_features_geom_harness.cpp."""
import ctypes as C
import math

import numpy as np
import torch

import common
import dense_twin
import tolerance
from common import f32, ptr, syn
from oracle import oracle
from tolerance import TOL, rel_err  # noqa: F401  (the tests of this feature take them from here)

GEOMETRY = ("means2D", "means3D", "opacities", "scales", "rotations")

# tests/test_gpu_features.py's scenes (seed 3, extent (1.5, 1, 1.5), orbit_camera(1, 7, ..., radius 4)), plus an opaque one in which
# pixels terminate before their list ends (opacity_mean chosen on the CPU: sigmoid(4) = 0.98, test_features_geom_host.py asserts it)
SCENES = {
    "N300_70x45": dict(N=300, W=70, H=45, scale=0.06, opm=0.0),
    "N64_33x17": dict(N=64, W=33, H=17, scale=0.1, opm=0.0),
    "N400_48x48": dict(N=400, W=48, H=48, scale=0.25, opm=-2.0),
    "N400_48x48_seg64": dict(N=400, W=48, H=48, scale=0.25, opm=-2.0, seg=64),
    "N200_40x40_opaque": dict(N=200, W=40, H=40, scale=0.25, opm=4.0),
}


def scene(name, camera=None):
    """camera: None = the orbit camera every scene was chosen under, or a name of tests/camera_common.py (pitched, rolled, inside)."""
    c = SCENES[name]
    g = syn.make_gaussians(c["N"], seed=3, extent=(1.5, 1.0, 1.5), log_scale_mean=math.log(c["scale"]), opacity_mean=c["opm"])
    if camera is None:
        cam = syn.orbit_camera(1, 7, c["W"], c["H"], radius=4.0)
    else:
        import camera_common
        cam = camera_common.camera(camera, c["W"], c["H"])
    return c, g, cam


def loss_inputs(N, Cn, H, W, bg=True, seed=11):
    """features [N, C], bg_features [C] or None, dL_dout [C,H,W], dL_dalpha [H,W], dL_dcolor [3,H,W]: float32, fixed seed."""
    rs = np.random.RandomState(seed + Cn)
    F = rs.randn(N, Cn).astype(np.float32)
    bgf = rs.randn(Cn).astype(np.float32) if bg else None
    return F, bgf, rs.randn(Cn, H, W).astype(np.float32), rs.randn(H, W).astype(np.float32), rs.randn(3, H, W).astype(np.float32)


_REF = {}


def reference(name, Cn, bg, kind, color_bg=(0.1, 0.2, 0.3), camera=None):
    """{dtype name: {tensor: float64 array}} for float64 and float32 oracles: the sum over channel triples of oracle.backward -- the
    feature columns (and a column of ones with background 0 for alpha) padded to whole triples as colors_precomp, plus, for kind
    "c" in kind, the backward of the scene's own SH colours over color_bg.  kind: the maps in the loss, letters of "oac" (out, alpha,
    colour).  camera: as for scene().  Computed once per key."""
    name = name.replace("_seg64", "")         # the same scene: the segment length is the rasterizer's business
    key = (name, Cn, bool(bg), kind, camera)
    if key in _REF:
        return _REF[key]
    c, g, cam = scene(name, camera)
    N, W, H = c["N"], c["W"], c["H"]
    F, bgf, dout, dalpha, dcolor = loss_inputs(N, Cn, H, W, bg)
    cols, grads, bgs = [], [], []
    if "o" in kind:
        cols.append(F); grads.append(dout); bgs.append(bgf if bgf is not None else np.zeros(Cn, np.float32))
    if "a" in kind:
        cols.append(np.ones((N, 1), np.float32)); grads.append(dalpha[None]); bgs.append(np.zeros(1, np.float32))
    cols, grads, bgs = np.concatenate(cols, 1), np.concatenate(grads, 0), np.concatenate(bgs)
    pad = (-cols.shape[1]) % 3
    cols = np.concatenate([cols, np.zeros((N, pad), np.float32)], 1)
    grads = np.concatenate([grads, np.zeros((pad, H, W), np.float32)], 0)
    bgs = np.concatenate([bgs, np.zeros(pad, np.float32)])
    out = {}
    for dt in (np.float64, np.float32):
        acc = {n: 0.0 for n in GEOMETRY}
        for c0 in range(0, cols.shape[1], 3):
            kw = common.scene_kwargs(g, cam, W, H, precolor=torch.from_numpy(cols[:, c0:c0 + 3].copy()), bg=tuple(float(b) for b in bgs[c0:c0 + 3]))
            gr = oracle.backward(oracle.forward(dtype=dt, **kw), grads[c0:c0 + 3])
            for n in GEOMETRY:
                acc[n] = acc[n] + np.asarray(gr[n], np.float64)
        if "c" in kind:
            kw = common.scene_kwargs(g, cam, W, H, bg=color_bg)
            gr = oracle.backward(oracle.forward(dtype=dt, **kw), dcolor)
            for n in GEOMETRY:
                acc[n] = acc[n] + np.asarray(gr[n], np.float64)
        out[np.dtype(dt).name] = acc
    _REF[key] = out
    return out


def assert_within(got, ref, what="", names=GEOMETRY):
    """The rule of test_backward_parity: rule 3 and the element-wise bound, against the float32 oracle's own error against the float64
    one on the same sums."""
    for n in names:
        tolerance.assert_rule3(got[n], ref["float64"][n], ref["float32"][n], f"{what} {n}", ref="oracle", nonzero=False)
        tolerance.assert_elementwise(got[n], ref["float64"][n], ref["float32"][n], f"{what} {n}")


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("features_geom", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_feature_bwd_step": (I, [I] + [F] * 7 + [C.POINTER(F)] * 2 + [P, C.POINTER(F)]),
        "h_features_geom": (C.c_longlong, [I] * 4 + [P] * 6 + [F, F] + [P] * 13)})


def harness_grads(kw, features, bg=None, dL_dout=None, dL_dalpha=None):
    """kw: common.scene_kwargs(...) (numpy, scales / rotations).  Returns ({tensor: array}, out [C,H,W], alpha [H,W], radii, pixels that
    ended before their list did)."""
    lib = harness()
    means3D = f32(kw["means3D"]); N = means3D.shape[0]
    feats = f32(features); Cn = feats.shape[1]
    W, H = kw["W"], kw["H"]
    op = f32(kw["opacities"]).reshape(-1); sc = f32(kw["scales"]); rot = f32(kw["rotations"])
    vm = f32(kw["viewmatrix"]); pm = f32(kw["projmatrix"])
    bgc, g, ga = f32(bg), f32(dL_dout), f32(dL_dalpha)
    out = np.zeros((Cn, H, W), np.float32); alpha = np.zeros((H, W), np.float32); radii = np.zeros(N, np.int32)
    gr = dict(means2D=np.zeros((N, 3), np.float32), means3D=np.zeros((N, 3), np.float32), opacities=np.zeros((N, 1), np.float32),
              scales=np.zeros((N, 3), np.float32), rotations=np.zeros((N, 4), np.float32))
    early = np.zeros(1, np.int64)
    lib.h_features_geom(N, Cn, W, H, ptr(means3D), ptr(op), ptr(sc), ptr(rot), ptr(vm), ptr(pm), float(kw["tanfovx"]), float(kw["tanfovy"]), ptr(feats),
                        ptr(bgc), ptr(g), ptr(ga), ptr(out), ptr(alpha), ptr(radii), ptr(gr["means2D"]), ptr(gr["means3D"]), ptr(gr["opacities"]),
                        ptr(gr["scales"]), ptr(gr["rotations"]), ptr(early))
    return gr, out, alpha, radii, int(early[0])


def early_pixels(name):
    """Number of pixels of the scene whose front-to-back walk ended (T (1 - alpha) < 1e-4) before the end of their tile's list, from the
    ORACLE's state alone: its n_contrib, final_T and the tile ranges of its reference rectangles.  The first entry behind a pixel's
    last contributor that passes the power / alpha tests can only be the entry that ended the walk."""
    c, g, cam = scene(name)
    W, H = c["W"], c["H"]
    f = oracle.forward(**common.scene_kwargs(g, cam, W, H))
    s = f.saved
    x, y = s["xy"][:, 0].astype(np.float64), s["xy"][:, 1].astype(np.float64)
    A, B, Cc, op = (s["conic_opacity"][:, k].astype(np.float64) for k in range(4))
    rad = f.radii.astype(np.float64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rx0 = np.clip(np.trunc((x - rad) / 16), 0, gx); rx1 = np.clip(np.trunc((x + rad + 15) / 16), 0, gx)
    ry0 = np.clip(np.trunc((y - rad) / 16), 0, gy); ry1 = np.clip(np.trunc((y + rad + 15) / 16), 0, gy)
    n_contrib, final_T = s["n_contrib"].reshape(H, W), s["final_T"].reshape(H, W)
    n = 0
    for ty in range(gy):
        for tx in range(gx):
            ids = np.nonzero((f.radii > 0) & (rx0 <= tx) & (tx < rx1) & (ry0 <= ty) & (ty < ry1))[0]
            order = ids[np.argsort(s["depth"][ids], kind="stable")]
            for py in range(ty * 16, min(H, ty * 16 + 16)):
                for px in range(tx * 16, min(W, tx * 16 + 16)):
                    for j in order[n_contrib[py, px]:]:
                        dx, dy = x[j] - px, y[j] - py
                        power = -0.5 * (A[j] * dx * dx + Cc[j] * dy * dy) - B[j] * dx * dy
                        alpha = min(0.99, op[j] * math.exp(min(power, 0.0)))
                        if power <= 0 and alpha >= 1.0 / 255.0:
                            assert final_T[py, px] * (1.0 - alpha) < 1.0001e-4
                            n += 1
                            break
    return n


RAW = ("_xyz", "_opacity", "_scaling", "_rotation")


def depth_loss_maps(H, W, seed=5):
    rs = np.random.RandomState(seed)
    return rs.randn(H, W), rs.randn(H, W)


_DEPTH_REF = {}


def dense_depth_reference(name, camera=None, antialias=False):
    """{dtype name: {raw parameter: gradient}} of  sum(depth gd + alpha ga),  depth = num / alpha.clamp_min(1e-6),  by the dense autograd
    twin (tests/dense_twin.py, all N Gaussians) rendering colors_precomp = [z(means3D), 1, 0] from the model's RAW parameters through its
    activations, in float64 and in float32; plus "maps": the float64 twin's (numerator, alpha, radii).  camera: as for scene();
    antialias: with rho wrapped around the opacity.  Computed once per key."""
    key = (name, camera, antialias)
    if key in _DEPTH_REF:
        return _DEPTH_REF[key]
    c, g, cam = scene(name, camera)
    kw = common.scene_kwargs(g, cam, c["W"], c["H"], precolor=torch.zeros(c["N"], 3), as_torch=True)
    gd, ga = depth_loss_maps(c["H"], c["W"])
    out = {}
    for dd, dname in dense_twin.DTYPES:
        raw = {n: getattr(g, n).to(dd).detach().clone().requires_grad_() for n in RAW}
        vm = cam.world_view_transform.to(dd)
        z = raw["_xyz"] @ vm[:3, 2:3] + vm[3, 2]
        act = dict(means3D=raw["_xyz"], opacities=torch.sigmoid(raw["_opacity"]), scales=torch.exp(raw["_scaling"]),
                   rotations=torch.nn.functional.normalize(raw["_rotation"]), colors_precomp=torch.cat([z, torch.ones_like(z), torch.zeros_like(z)], 1))
        color, radii, _cnt = dense_twin.render(kw, dd, leaves=act, antialias=antialias, front_only=False)
        depth = color[0] / color[1].clamp_min(1e-6)
        (depth * torch.from_numpy(gd).to(dd) + color[1] * torch.from_numpy(ga).to(dd)).sum().backward()
        out[dname] = {n: raw[n].grad.numpy().astype(np.float64) for n in RAW}
        if dd == torch.float64:
            out["maps"] = (color[0].detach().numpy(), color[1].detach().numpy(), radii.numpy())
    _DEPTH_REF[key] = out
    return out


def assert_depth_maps(num, alpha, ref_maps, what=""):
    """A float32 depth numerator / alpha / depth = num / max(alpha, 1e-6) against the float64 twin's maps.  Numerator and alpha: the 1e-5
    of a float32 render against the float64 one (absolute for alpha in [0, 1], relative to max |num| for the numerator: the bounds of
    tests/test_features_geom_host.py).  Depth: first-order propagation of those two bounds through the quotient,
    |d depth| <= (|d num| + |depth| |d alpha|) / alpha, asserted where alpha >= 1e-3 (where first order holds: |d alpha| / alpha <= 1e-2)."""
    num, alpha = np.asarray(num, np.float64), np.asarray(alpha, np.float64)
    n64, a64, _r = ref_maps
    scale = np.abs(n64).max()
    e_n, e_a = np.abs(num - n64).max(), np.abs(alpha - a64).max()
    print(f"{what}: numerator max error {e_n:.3e} (max |num| {scale:.3e}), alpha max error {e_a:.3e}")
    assert scale > 0 and e_n <= 1e-5 * scale and e_a <= 1e-5
    ok = a64 >= 1e-3
    d, d64 = num / np.maximum(alpha, 1e-6), n64 / np.maximum(a64, 1e-6)
    bound = 1.01 * (1e-5 * scale + np.abs(d64) * 1e-5) / np.maximum(a64, 1e-3)
    worst = float((np.abs(d - d64)[ok] / bound[ok]).max())
    print(f"{what}: depth error at most {worst:.3f}x its bound over {int(ok.sum())} pixels")
    assert ok.sum() > 100 and worst <= 1.0
