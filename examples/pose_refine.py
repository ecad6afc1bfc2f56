#!/usr/bin/env python3
"""Recover a perturbed camera pose against a frozen model, on a synthetic scene:

    target        render() of the model from the TRUE pose (a look_at_camera)
    start         the true pose rotated by a few degrees and moved by a few centimetres (pose.PoseCamera of the perturbed camera)
    refine        Adam on the camera's 6-vector (rotation vector, translation): per step ONE render(..., options={"camera_grad": True});
                  its backward is the usual lg_backward followed by lg_backward_camera on the same gradient rows, and autograd carries
                  dL/dworld_view_transform, dL/dfull_proj_transform and dL/dcamera_center through the se(3) exponential to the 6-vector

    python examples/pose_refine.py [--n-gaussians 20000] [--steps 200]

Printed every 10 steps: the L1 loss and the pose error against the true camera -- the angle of the residual rotation in degrees and
the distance between the camera centres in centimetres (scene units x 100)."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402
from lightgaussian_amd.pose import PoseCamera  # noqa: E402


def pose_error(cam, true_cam):
    """(degrees, centimetres) between the camera and the true one."""
    with torch.no_grad():
        r = cam.world_view_transform[:3, :3].t() @ true_cam.world_view_transform[:3, :3]       # residual rotation
        ang = math.degrees(math.acos(max(-1.0, min(1.0, (float(r.trace()) - 1.0) * 0.5))))
        return ang, 100.0 * float((cam.camera_center - true_cam.camera_center).norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=20_000)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--degrees", type=float, default=3.0, help="size of the rotation perturbation")
    ap.add_argument("--centimetres", type=float, default=5.0, help="size of the translation perturbation")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    model = syn.make_gaussians(args.n_gaussians, extent=(2.0, 1.2, 2.0), log_scale_mean=math.log(0.03)).to(dev)
    true_cam = syn.look_at_camera((3.0, -1.5, -4.0), (0.0, 0.0, 0.0), args.width, args.height, roll_deg=10.0).to(dev)
    with torch.no_grad():
        target = render(true_cam, model, pipe, bg)["render"]
        # the perturbed start: the true camera with a fixed se(3) offset baked in
        off = PoseCamera(true_cam).to(dev)
        a, t = math.radians(args.degrees) / math.sqrt(3.0), args.centimetres / 100.0 / math.sqrt(3.0)
        off.xi.copy_(torch.tensor([a, -a, a, t, t, -t]))
        start = syn.MiniCam(args.width, args.height, true_cam.FoVy, true_cam.FoVx, true_cam.znear, true_cam.zfar,
                            off.world_view_transform.clone(), off.full_proj_transform.clone(), off.camera_center.clone())
    cam = PoseCamera(start).to(dev)
    opt = torch.optim.Adam(cam.parameters(), lr=args.lr)
    for it in range(args.steps + 1):
        loss = (render(cam, model, pipe, bg, options={"camera_grad": True})["render"] - target).abs().mean()
        if it % 10 == 0:
            ang, cm = pose_error(cam, true_cam)
            print(f"step {it:4d}: L1 {float(loss):.6f}   rotation error {ang:.4f} deg   centre error {cm:.3f} cm")
        if it == args.steps:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()


if __name__ == "__main__":
    main()
