"""tests/golden/lg_math_bits.npz: the bits the per-Gaussian backward functions of an lg_math.h return (tests/test_math_frozen_host.py).

    python tests/golden/make_golden_math_bits.py PATH/TO/lg_math.h

PATH is the header to freeze -- the one of the commit the tree must keep computing what it computed, NEVER the tree's own after a change to
the arithmetic.  tests/cpu_harness/lg_math_harness.cpp is compiled against it in a temporary directory with the flags of common.harness()
(STRICT_FP_FMA) and run on:
  orbit           the scene of test_math_harness.test_backward_geometry_stage_matches_oracle cut to its first 512 Gaussians
  pitched_rolled  camera_common's scene under a camera with a full view rotation
  inside          ... under the camera among the splats: clamped t.x / t.y lanes, depths down to 0.2
with acc = RandomState(5).randn(N, 9) as _backward_geometry_stage draws it.  Only visible Gaussians (oracle radii > 0) are fed: the
kernels call these functions on no others.  To keep the file under 300 KB, each scene contributes N_GEOM Gaussians -- every one with a
clamped t.x / t.y first, the rest spread evenly over the visible ones -- and the SH functions run on the first N_SH of them.
Asserted: every scene has at least 200 visible Gaussians; the scenes with an off-axis or inside camera together, and `inside` alone,
have at least 10 x-clamped and 10 y-clamped ones IN the fixture.  (Measured on the visible Gaussians: orbit 0 / 0 -- a level camera
outside the scene cannot clamp --, pitched_rolled 0 x / 13 y, inside 23 x / 43 y.)"""
import ctypes
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import camera_common  # noqa: E402
import common  # noqa: E402
import test_math_frozen_host as frozen  # noqa: E402
from common import f32, syn  # noqa: E402
from oracle import oracle  # noqa: E402

N_GEOM = 96


def build(header):
    """The math harness compiled against `header`, in the layout its #include expects."""
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "tests", "cpu_harness"))
    os.makedirs(os.path.join(tmp, "lightgaussian_amd", "csrc"))
    src = os.path.join(tmp, "tests", "cpu_harness", "lg_math_harness.cpp")
    shutil.copy(os.path.join(common.ROOT, "tests", "cpu_harness", "lg_math_harness.cpp"), src)
    shutil.copy(header, os.path.join(tmp, common.LG_MATH_H))
    so = os.path.join(tmp, "liblg_math_harness.so")
    old = () if "lg_backward_sh_one_pass" in open(header).read() else ("-DLG_HARNESS_NO_ONE_PASS",)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", *common.STRICT_FP_FMA, *old, src, "-o", so])
    lib = ctypes.CDLL(so)
    for symbol, (restype, argtypes) in common.math_signatures().items():
        getattr(lib, symbol).restype, getattr(lib, symbol).argtypes = restype, list(argtypes)
    return lib


def scene(name):
    if name == "orbit":
        g = syn.make_gaussians(4000, seed=21, log_scale_mean=math.log(0.03))
        kw = common.scene_kwargs(g, syn.orbit_camera(1, 6, 160, 120), 160, 120)
        kw = {k: (v[:512] if getattr(v, "shape", None) and v.shape[0] == 4000 else v) for k, v in kw.items()}
        raw = g._rotation.detach().numpy()[:512]
    else:
        g = camera_common.gaussians()
        kw = camera_common.scene_kwargs(name)
        raw = g._rotation.detach().numpy()
    return kw, raw


def inputs(name):
    kw, rot_raw = scene(name)
    N = kw["means3D"].shape[0]
    radii = oracle.forward(**kw).radii
    vis = radii > 0
    acc = (np.random.RandomState(5).randn(N, 9) * vis[:, None]).astype(np.float32)
    fa = camera_common.view_facts(kw, radii)
    assert fa["visible"] >= 200, (name, fa)
    vm, p = f32(kw["viewmatrix"]).reshape(-1), f32(kw["means3D"])
    v = [vm[k] * p[:, 0] + vm[4 + k] * p[:, 1] + vm[8 + k] * p[:, 2] + vm[12 + k] for k in range(3)]
    limx, limy = np.float32(1.3) * np.float32(kw["tanfovx"]), np.float32(1.3) * np.float32(kw["tanfovy"])
    xc, yc = vis & (np.abs(v[0] / v[2]) > limx), vis & (np.abs(v[1] / v[2]) > limy)
    assert int(xc.sum()) == fa["xclamp"] and int(yc.sum()) == fa["yclamp"]
    clamped = np.flatnonzero(xc | yc)
    assert len(clamped) <= N_GEOM - 16, (name, len(clamped))
    others = np.flatnonzero(vis & ~(xc | yc))
    others = others[np.linspace(0, len(others) - 1, N_GEOM - len(clamped)).astype(int)]
    sel = np.concatenate([clamped, others])
    assert len(set(sel.tolist())) == N_GEOM
    rs = np.random.RandomState(6)
    take = lambda a: np.ascontiguousarray(f32(a)[sel])  # noqa: E731
    s = dict(means3D=take(kw["means3D"]), scales=take(kw["scales"]), rotations=take(kw["rotations"]), rot_raw=take(rot_raw),
             op=take(kw["opacities"]).reshape(-1), acc=take(acc), shs=take(kw["shs"]).reshape(N_GEOM, 48)[:frozen.N_SH].copy(),
             dS=rs.randn(N_GEOM, 6).astype(np.float32), noise=rs.randn(N_GEOM, 3).astype(np.float32),
             d=rs.randn(N_GEOM, 3).astype(np.float32), dRGB=rs.randn(N_GEOM, 3).astype(np.float32),
             viewmatrix=f32(kw["viewmatrix"]), projmatrix=f32(kw["projmatrix"]), campos=f32(kw["campos"]),
             W=np.int32(kw["W"]), H=np.int32(kw["H"]), tanfovx=np.float32(kw["tanfovx"]), tanfovy=np.float32(kw["tanfovy"]))
    s["dRGB"][::5, 1] = 0.0     # clamped colour channels arrive as zeros
    return s, int(xc[sel].sum()), int(yc[sel].sum())


def main(header):
    lib = build(header)
    torch.manual_seed(0)
    data, clamps = {}, {}
    for name in frozen.SCENES:
        s, nx, ny = inputs(name)
        clamps[name] = (nx, ny)
        out = frozen.outputs(lib, s, forms=(0, 1))
        for k, v in out.items():
            assert np.isfinite(v).all(), (name, k)
        data.update({f"{name}_in_{k}": v for k, v in s.items()})
        data.update({f"{name}_out_{k}": v for k, v in out.items() if "_jac1_" not in k})     # asserted equal to the _jac0_ ones
    print("x / y clamped Gaussians in the fixture:", clamps)
    why = f"x / y clamped Gaussians per scene {clamps}; when the scenes were chosen: orbit 0 / 0, pitched_rolled 0 / 13, inside 23 / 43"
    assert min(clamps["inside"]) >= 10, why
    assert clamps["pitched_rolled"][0] + clamps["inside"][0] >= 10 and clamps["pitched_rolled"][1] + clamps["inside"][1] >= 10, why
    path = os.path.join(HERE, "lg_math_bits.npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < 300 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
