#!/usr/bin/env python3
"""Why densification wants ABSOLUTE view-space gradients (option "absgrad"): one oversized Gaussian over a checkerboard target.

    python examples/absgrad_densify.py [--width 256] [--height 256] [--cells 16] [--small 400]

The scene is a grey background plane of small Gaussians plus ONE large, blurry, light-grey Gaussian in front of it that covers many cells of a
black-and-white checkerboard target.  The L1 image loss pulls it towards every white cell and away from every black one: the per-pixel
gradients of its screen position have opposite signs from cell to cell and cancel in the sum.  GaussianModel.add_densification_stats
thresholds the norm of that sum, so the Gaussian that most needs splitting never crosses densify_grad_threshold (the over-reconstruction
failure AbsGS describes).  With options={"absgrad": True} the backward also leaves the sum of the per-pixel magnitudes in
viewspace_points.absgrad.  Printed: the two norms for the large Gaussian and their medians over the small ones, and the rank of the
large one under both criteria."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--cells", type=int, default=16, help="checkerboard cell size in pixels")
    ap.add_argument("--small", type=int, default=400, help="small Gaussians of the background plane")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    cam = syn.look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), W, H)
    # the background: small grey Gaussians scattered over the plane z = 0.5; in front of them, at the origin, the oversized one
    g = syn.make_gaussians(args.small + 1, seed=5, extent=(2.0, 2.0, 0.0), log_scale_mean=math.log(0.05), opacity_mean=1.0, rest_std=0.0)
    with torch.no_grad():
        g._xyz[:, 2] = 0.5
        g._features_dc[:] = syn.RGB2SH(torch.full((1, 1, 3), 0.5))
        g._features_dc[-1] = syn.RGB2SH(torch.full((1, 3), 0.8))      # lighter than what lies behind it: moving it changes the image
        g._xyz[-1] = torch.tensor([0.03, -0.02, 0.0])
        g._scaling[-1] = math.log(0.7)
        g._opacity[-1] = 0.0
    model = g.to(dev).requires_grad_(True)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    target = (((xx // args.cells) + (yy // args.cells)) % 2).float()[None].expand(3, H, W)
    pkg = render(cam.to(dev), model, syn.PipelineParams(), torch.full((3,), 0.5, device=dev), options={"absgrad": True})
    (pkg["render"] - target).abs().mean().backward()
    vp = pkg["viewspace_points"]
    signed, absolute = vp.grad[:, :2].norm(dim=-1), vp.absgrad[:, :2].norm(dim=-1)
    vis = pkg["visibility_filter"]
    big = args.small
    small = vis.clone()
    small[big] = False

    def rank(v):
        return int((v[vis] > v[big]).sum()) + 1

    print(f"{W} x {H}, cells of {args.cells} px, {int(vis.sum())} visible Gaussians; the large one has radius {int(pkg['radii'][big])} px")
    print(f"{'':>24s} {'|grad|':>12s} {'|absgrad|':>12s} {'ratio':>8s}")
    print(f"{'the large Gaussian':>24s} {float(signed[big]):12.4e} {float(absolute[big]):12.4e} {float(absolute[big] / signed[big]):8.1f}")
    ms, ma = float(signed[small].median()), float(absolute[small].median())
    print(f"{'median of the small ones':>24s} {ms:12.4e} {ma:12.4e} {ma / ms:8.1f}")
    print(f"rank of the large Gaussian among the visible ones: {rank(signed)} by |grad|, {rank(absolute)} by |absgrad|")
    thr = 0.0002            # the reference's default densify_grad_threshold; AbsGS and gsplat use 2-4 x with absolute gradients
    print(f"densify_grad_threshold {thr}: |grad| {'crosses' if float(signed[big]) > thr else 'stays below'} it, "
          f"|absgrad| {'crosses' if float(absolute[big]) > 4 * thr else 'stays below'} 4 x it")


if __name__ == "__main__":
    main()
