#!/usr/bin/env python3
"""The 3D smoothing filter from training cameras to an exportable model (lightgaussian_amd/filter3d.py):

    filter_3D = compute_filter_3d(xyz, orbit of training cameras)      one pass over the Gaussians
    render(model with filter_3D)                                         the filter applied raw -> raw in front of the fused kernels
    _scaling', _opacity' = fuse_filter_3d(model)                         the filter baked into the raw tensors (save_fused_ply)
    render(model with _scaling', _opacity' and no filter)                the same picture, bit for bit

    python examples/filter3d_fuse.py [--n-gaussians 300000] [--width 480] [--height 270] [--views 24]

A Gaussian that no training camera samples finer than one pixel per t world units is not allowed to be narrower than sqrt(0.2) t: when
the camera later moves closer, or the focal length grows, it does not erode into a needle or a bright spike.  Printed: how many
Gaussians the filter widened by more than 10 % on some axis, how many no camera saw, and the largest difference between the two
renders of every view (0 expected).  The fused tensors are what the reference's save_ply, the prune pass and the VecTree compressor
take: after the fusion the model needs no filter anywhere."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import filter3d, synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=300_000)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--log-scale-mean", type=float, default=math.log(0.006))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    model = syn.make_gaussians(args.n_gaussians, log_scale_mean=args.log_scale_mean).to(dev)
    cams = [syn.orbit_camera(k, args.views, args.width, args.height).to(dev) for k in range(args.views)]
    with torch.no_grad():
        model.filter_3D, seen = filter3d.compute_filter_3d(model.get_xyz, cams, return_seen=True)
        s = model.get_scaling
        widened = (torch.sqrt(s * s + model.filter_3D ** 2) > 1.1 * s).any(1)
        print(f"{args.n_gaussians} Gaussians, {args.views} cameras of {args.width} x {args.height}: filter_3D from "
              f"{float(model.filter_3D.min()):.5f} to {float(model.filter_3D.max()):.5f} world units")
        print(f"widened by more than 10 % on some axis: {int(widened.sum())}   seen by no camera: {int((~seen).sum())}")
        fused = model.to(dev)
        fused._scaling, fused._opacity = filter3d.fuse_filter_3d(model)
        fused.filter_3D = None
        worst, changed = 0.0, 0.0
        for cam in cams:
            a = render(cam, model, pipe, bg)["render"]
            b = render(cam, fused, pipe, bg)["render"]
            plain = render(cam, model, pipe, bg, options={"filter_3d": False})["render"]
            worst = max(worst, float((a - b).abs().max()))
            changed = max(changed, float((a - plain).abs().max()))
        print(f"largest |filtered render - plain render of the fused model| over {args.views} views: {worst:g}")
        print(f"largest |filtered render - unfiltered render|: {changed:.4f}")


if __name__ == "__main__":
    main()
