"""General cameras for the parity tests (test infrastructure): pitched, rolled, and standing inside the scene.

Every other camera of the suite is synthetic.orbit_camera: level, on a circle of constant y, outside the scene -- a view rotation about
world y (four of its nine entries exactly 0, one exactly 1), depths in [1, 9], no splat near the 0.2 near plane, the +-1.3 tan(fov)
clamp of the EWA Jacobian all but idle.  The four cameras below have a full rotation matrix; the two inside ones stand among the
splats: Gaussians in 0 < z_view <= 0.2 and behind the camera, both clamps engaged on visible splats, radii of hundreds of pixels next
to 3 px ones, sort-key depths that start at the near plane.

check_preconditions() asserts, once per process and on the host (float32 oracle forward + the float32 view transform), that the scene
and the cameras still have these properties: the tests that use them cannot silently go soft if a generator changes."""
import math

import numpy as np
import torch

import common
from common import syn
from oracle import oracle

W, H = 161, 83
# the scene of tests/test_gpu_parity.py CASES[3]'s shape with splats large enough to fill the screen from inside
CAMERA_SCENE = dict(N=2000, seed=4, log_scale_mean=math.log(0.03), log_scale_std=0.9, opacity_mean=0.0, extent=(2.0, 1.2, 2.0))
BG = (0.1, 0.2, 0.3)

# name: (eye, target, roll in degrees, horizontal field of view in degrees)
CAMERAS = {
    "pitched_rolled": ((3.0, -2.5, -3.5), (0.3, 0.2, -0.1), 25.0, 60.0),
    "steep_offcentre": ((1.0, -4.5, 1.5), (-0.8, 0.5, 0.4), -70.0, 60.0),
    "inside": ((0.3, 0.1, -0.4), (1.0, 0.6, 1.0), 10.0, 60.0),
    "inside_wide": ((-0.2, 0.05, 0.1), (-1.0, -0.3, 1.0), -35.0, 100.0),
}
NAMES = tuple(CAMERAS)
INSIDE = ("inside", "inside_wide")


def camera(name, width=W, height=H):
    eye, target, roll, fovx = CAMERAS[name]
    return syn.look_at_camera(eye, target, width, height, roll_deg=roll, fovx_deg=fovx)


def gaussians(sh_degree=3):
    return syn.make_gaussians(CAMERA_SCENE["N"], sh_degree=sh_degree, **{k: v for k, v in CAMERA_SCENE.items() if k != "N"})


def precolors():
    return torch.rand(CAMERA_SCENE["N"], 3, generator=torch.Generator().manual_seed(7))


def scene_kwargs(name, deg=3, precolor=False, precov=False, as_torch=False):
    """Rasterizer kwargs of CAMERA_SCENE under camera `name` (numpy, or CPU torch tensors with as_torch)."""
    check_preconditions()
    return common.scene_kwargs(gaussians(), camera(name), W, H, deg=deg, precolor=precolors() if precolor else None, precov=precov,
                               bg=BG, as_torch=as_torch)


def view_facts(kw, radii):
    """What a view exercises, from the float32 inputs the kernels see and the oracle's radii: the smallest |entry| of the view rotation,
    Gaussians between the camera plane and the near plane, Gaussians behind the camera, visible Gaussians on which the x / y clamp of
    t/z engages (the test of the oracle's ewa_T, in float32), the largest radius, the number of visible Gaussians."""
    f32 = np.float32
    vm = np.asarray(kw["viewmatrix"], f32).reshape(-1)
    p = np.asarray(kw["means3D"], f32)
    v = [vm[k] * p[:, 0] + vm[4 + k] * p[:, 1] + vm[8 + k] * p[:, 2] + vm[12 + k] for k in range(3)]
    vis = np.asarray(radii) > 0
    assert not (vis & (v[2] <= f32(0.2))).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        txtz, tytz = v[0] / v[2], v[1] / v[2]
    limx, limy = f32(1.3) * f32(kw["tanfovx"]), f32(1.3) * f32(kw["tanfovy"])
    return dict(min_rot=float(np.abs(vm.reshape(4, 4)[:3, :3]).min()),
                near=int(((v[2] > 0) & (v[2] <= f32(0.2))).sum()), behind=int((v[2] <= 0).sum()),
                xclamp=int((vis & ((txtz < -limx) | (txtz > limx))).sum()), yclamp=int((vis & ((tytz < -limy) | (tytz > limy))).sum()),
                max_radius=int(np.asarray(radii).max()), visible=int(vis.sum()),
                min_depth=float(v[2][vis].min()) if vis.any() else float("nan"))


_CHECKED = {}


def check_preconditions():
    """Conditions (not measurements) that make the cameras worth testing; measured when they were chosen, in the order of NAMES:
    min |rotation entry| 0.033, 0.133, 0.165, 0.277; and on the two inside cameras: 0 < z_view <= 0.2: 116, 136; behind: 880, 1123;
    x clamp 23, 19; y clamp 43, 59; largest radius 320, 251; visible 1925, 1512, 271, 443."""
    if _CHECKED:
        return _CHECKED
    g = gaussians()
    facts = {}
    for name in NAMES:
        kw = common.scene_kwargs(g, camera(name), W, H, bg=BG)
        facts[name] = fa = view_facts(kw, oracle.forward(**kw).radii)
        assert fa["min_rot"] >= 0.03, (name, fa)
        assert fa["visible"] >= 200, (name, fa)
        if name in INSIDE:
            assert fa["near"] >= 50 and fa["behind"] >= 500, (name, fa)
            assert fa["xclamp"] >= 10 and fa["yclamp"] >= 10, (name, fa)
            assert fa["max_radius"] >= 200, (name, fa)
    _CHECKED.update(facts)
    return _CHECKED
