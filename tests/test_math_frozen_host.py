"""The per-Gaussian backward arithmetic of lightgaussian_amd/csrc/lg_math.h, frozen bit for bit.  No GPU.

tests/golden/lg_math_bits.npz holds inputs (Gaussians of three scenes, the clamped ones of each first) and what the g++ build of the
header returned for them when the fixture was made (tests/golden/make_golden_math_bits.py, from the commit BEFORE the backward chain, the SH
backward and the quaternion matrix were given one copy each).  The tree's header must return the same bits: under -ffp-contract=off the
association and operand order of every expression fix them, so a helper that reorders a sum, drops the clamp convention of dtx / dty
or swaps a view-matrix index shows here.  Functions that call libm transcendentals are left out (their bits are the C library's);
lg_project's bits are pinned against the oracle in test_math_harness."""
import os

import numpy as np
import pytest

import common
from common import ptr as P

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lg_math_bits.npz")
SCENES = ("orbit", "pitched_rolled", "inside")
N_SH = 32       # the SH functions run on the first N_SH Gaussians of a scene (their outputs are 3 (D + 1)^2 floats each)


def outputs(lib, s, forms=(0, 1, 2)):
    """Every pinned output for one scene's inputs s (a dict of float32 arrays and the scalars W, H, tanfovx, tanfovy)."""
    n = s["means3D"].shape[0]
    W, H, tx, ty = int(s["W"]), int(s["H"]), float(s["tanfovx"]), float(s["tanfovy"])
    vm, pm, cp = s["viewmatrix"], s["projmatrix"], s["campos"]
    z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    o = dict(cov3D=z(n, 6), dscale=z(n, 3), drot=z(n, 4), child=z(n, 3))
    lib.h_cov3d(n, P(s["scales"]), 1.0, P(s["rotations"]), P(s["dS"]), P(o["cov3D"]), P(o["dscale"]), P(o["drot"]))
    lib.h_child_xyz(n, P(s["rot_raw"]), P(s["scales"]), P(s["noise"]), P(s["means3D"]), P(o["child"]))
    for aa, tag in ((-1, "plain"), (0, "t_false"), (1, "t_true")):
        o["geom_" + tag], o["camera_" + tag] = z(n, 12), z(n, 27)
        lib.h_geom(n, aa, P(vm), P(pm), P(s["means3D"]), P(o["cov3D"]), P(s["acc"]), W, H, tx, ty, P(s["op"]), P(o["geom_" + tag]))
        lib.h_camera(n, aa, P(vm), P(pm), P(s["means3D"]), P(o["cov3D"]), P(s["acc"]), W, H, tx, ty, P(s["d"]), P(s["op"]),
                     P(o["camera_" + tag]))
    m = min(n, N_SH)
    for D in range(4):
        for jac in forms:     # 0: lg_backward_sh, 1: lg_sh_dir_jacobian + lg_backward_sh_jac, 2: lg_backward_sh_one_pass
            dsh, dmean, J = z(m, (D + 1) ** 2, 3), z(m, 3), z(m, 9)
            lib.h_sh_bwd(m, D, jac, P(s["shs"]), P(s["means3D"]), P(cp), P(s["dRGB"]), P(dsh), P(dmean), P(J))
            o[f"sh{D}_jac{jac}_dsh"], o[f"sh{D}_jac{jac}_dmean"] = dsh, dmean
            if jac == 1:
                o[f"sh{D}_J"] = J
    return o


def scene_inputs(fx, scene):
    return {k[len(scene) + 4:]: fx[k] for k in fx.files if k.startswith(scene + "_in_")}


@pytest.mark.parametrize("scene", SCENES)
def test_lg_math_backward_bits_are_those_of_the_fixture(scene):
    fx = np.load(FIXTURE)
    out = outputs(common.harness(), scene_inputs(fx, scene))
    for D in range(4):      # lg_backward_sh is lg_sh_dir_jacobian followed by lg_backward_sh_jac, and equals its one-pass form
        for part in ("dsh", "dmean"):
            for jac in (1, 2):
                assert np.array_equal(out[f"sh{D}_jac0_{part}"].view(np.uint32), out[f"sh{D}_jac{jac}_{part}"].view(np.uint32)), (D, part, jac)
    pinned = [k for k in fx.files if k.startswith(scene + "_out_")]
    assert sorted(pinned) == sorted(scene + "_out_" + k for k in out if "_jac1_" not in k and "_jac2_" not in k)
    for k in pinned:
        got = out[k[len(scene) + 5:]]
        assert got.shape == fx[k].shape and np.array_equal(got.view(np.uint32), fx[k].view(np.uint32)), k
