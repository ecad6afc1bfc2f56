#!/usr/bin/env python3
"""Cost of the camera pose gradient: render() forward + backward with and without option camera_grad, two legs on one GPU in one run.

    plain    render(cam, model, pipe, bg) and the backward of an image loss: K1 .. K6, K7, K9
    camera   the same with options={"camera_grad": True}: lg_backward_camera (lg_camera_bwd + lg_camera_reduce) behind K9, and
             autograd's three small gradient tensors on the camera

    python tools/camera_bench.py [--n 1000000 3000000] [--steps 20] [--blocks 5]

Frozen benchmark scene (synthetic.make_gaussians, sigma 0.004) at 1920 x 1080, SH degree 3, orbit cameras.  Per N: `--blocks`
alternating blocks of `--steps` views per leg after a warm-up, each block between two hipEvents; printed as median (min..max) of the
per-view time over the blocks, and one JSON line per N.  A difference is real only where the two intervals do not overlap."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402


def timed(legs, cams, args):
    """{leg: [ms per view of each block]}: a warm-up, then alternating blocks of args.steps views per leg between two events."""
    for fn in legs.values():
        for k in range(args.warmup):
            fn(cams[k % len(cams)])
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.steps):
                fn(cams[k % len(cams)])
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.steps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    G = torch.randn(3, args.height, args.width, device=dev, generator=torch.Generator(dev).manual_seed(0))
    for N in args.n:
        pc = syn.make_gaussians(N).to(dev).requires_grad_(True)
        leaves = [pc._xyz, pc._features_dc, pc._features_rest, pc._scaling, pc._rotation, pc._opacity]
        cams = [syn.orbit_camera(k, args.views, args.width, args.height).to(dev) for k in range(args.views)]
        pose_cams = []
        for c in cams:
            p = syn.MiniCam(c.image_width, c.image_height, c.FoVy, c.FoVx, c.znear, c.zfar, c.world_view_transform.clone().requires_grad_(True),
                            c.full_proj_transform.clone().requires_grad_(True), c.camera_center.clone().requires_grad_(True))
            pose_cams.append(p)
        by_id = {id(c): p for c, p in zip(cams, pose_cams)}

        def plain(cam):
            (render(cam, pc, pipe, bg)["render"] * G).sum().backward()
            for t in leaves:
                t.grad = None

        def camera(cam):
            p = by_id[id(cam)]
            (render(p, pc, pipe, bg, options={"camera_grad": True})["render"] * G).sum().backward()
            for t in leaves + [p.world_view_transform, p.full_proj_transform, p.camera_center]:
                t.grad = None

        times = timed({"plain": plain, "camera": camera}, cams, args)
        row = {"N": N, "W": args.width, "H": args.height, "build": _lib.build_id(), "steps": args.steps, "blocks": args.blocks}
        for name, ts in times.items():
            row[name + "_ms"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            print(f"N={N:>8d} {name:>7s}: {statistics.median(ts):.3f} ms per view ({min(ts):.3f}..{max(ts):.3f})")
        print(json.dumps(row))
        del pc, leaves


if __name__ == "__main__":
    main()
