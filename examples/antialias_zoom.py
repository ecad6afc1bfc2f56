#!/usr/bin/env python3
"""Zooming out of a model with and without the opacity compensation of the screen-space blur (option "antialiasing"):

    full-resolution render  ->  box-filtered to 1/2, 1/4, 1/8 resolution: what a camera with larger pixels would see
    render at 1/2, 1/4, 1/8 resolution, option off and on                -> PSNR of each against the box-filtered image

    python examples/antialias_zoom.py [--n-gaussians 300000] [--width 1920] [--height 1080]

Every splat gets a fixed 0.3-pixel blur on its 2D covariance.  At full resolution it is small against the splats; at 1/8 most splats
are below a pixel, the blur multiplies their footprint, and without the compensation (opacity times sqrt(det S / det(S + 0.3 I)))
they come out too thick and too bright.  Also printed: the (pixel, Gaussian) hit count of each render (alpha >= 1/255: what the
significance pass counts) -- uncompensated sub-pixel splats collect hits over their inflated footprint."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import count_render, render  # noqa: E402


def psnr(a, b):
    mse = float(((a - b) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=300_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--log-scale-mean", type=float, default=math.log(0.006))
    args = ap.parse_args()
    if args.width % 8 or args.height % 8:
        raise SystemExit("--width and --height must be multiples of 8 (the box filter)")
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    model = syn.make_gaussians(args.n_gaussians, log_scale_mean=args.log_scale_mean).to(dev)
    canonical = {"fast_exp": False}
    print(f"{args.n_gaussians} Gaussians, {args.views} views, full resolution {args.width} x {args.height}")
    print(f"{'scale':>6s} {'size':>11s} {'PSNR off':>9s} {'PSNR on':>9s} {'hits off':>11s} {'hits on':>11s}")
    with torch.no_grad():
        for f in (1, 2, 4, 8):
            w, h = args.width // f, args.height // f
            rows = []
            for k in range(args.views):
                full = render(syn.orbit_camera(k, args.views, args.width, args.height).to(dev), model, pipe, bg, options=canonical)["render"]
                target = torch.nn.functional.avg_pool2d(full[None], f)[0] if f > 1 else full
                cam = syn.orbit_camera(k, args.views, w, h).to(dev)
                off = count_render(cam, model, pipe, bg, options={"antialiasing": False})
                on = count_render(cam, model, pipe, bg, options={"antialiasing": True})
                rows.append((psnr(off["render"], target), psnr(on["render"], target), int(off["gaussians_count"].sum()),
                             int(on["gaussians_count"].sum())))
            m = [sum(r[i] for r in rows) / len(rows) for i in range(4)]
            print(f"{'1/' + str(f):>6s} {w:>5d}x{h:<5d} {m[0]:9.2f} {m[1]:9.2f} {int(m[2]):11d} {int(m[3]):11d}")


if __name__ == "__main__":
    main()
