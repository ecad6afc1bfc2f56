#!/usr/bin/env python3
"""Cost of the absolute mean gradients: render() forward + backward with and without option absgrad, two legs on one GPU in one run.

    plain    render(cam, model, pipe, bg) and the backward of an image loss: K1 .. K6, K7, K9
    absgrad  the same with options={"absgrad": True}: lg_backward_abs -- K7's ABS variant (11 partial sums per entry instead of 9) and
             lg_absgrad_rows (one more read of 16 of every 48 row bytes) between K7 and K9

    python tools/absgrad_bench.py [--n 1000000 3000000] [--steps 20] [--blocks 5]

Frozen benchmark scene (synthetic.make_gaussians, sigma 0.004) at 1920 x 1080, SH degree 3, orbit cameras.  Per N: `--blocks`
alternating blocks of `--steps` views per leg after a warm-up, each block between two hipEvents; printed as median (min..max) of the
per-view time over the blocks.  A difference is real only where the two intervals do not overlap.  Then, per leg, `--steps` views
with option profile (hipEvents around every kernel, which serialises the step: these figures are per-kernel times, not a breakdown of
the per-view time above): K7 (blend_bwd) and lg_absgrad_rows per view.  One JSON line per N."""
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
            fn(cams[k % len(cams)], {})
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.steps):
                fn(cams[k % len(cams)], {})
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.steps)
    return times


def kernels(fn, cams, args, names=("blend_bwd", "absgrad_rows")):
    """{kernel: ms per view} over args.steps profiled views."""
    torch.cuda.synchronize()
    _lib.profile_reset()
    for k in range(args.steps):
        fn(cams[k % len(cams)], {"profile": True})
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    return {n: prof[n][0] / args.steps for n in names if n in prof}


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

        def plain(cam, extra):
            (render(cam, pc, pipe, bg, options=extra)["render"] * G).sum().backward()
            for t in leaves:
                t.grad = None

        def absgrad(cam, extra):
            pkg = render(cam, pc, pipe, bg, options=dict(extra, absgrad=True))
            (pkg["render"] * G).sum().backward()
            assert pkg["viewspace_points"].absgrad.shape == (N, 3)
            for t in leaves:
                t.grad = None

        legs = {"plain": plain, "absgrad": absgrad}
        times = timed(legs, cams, args)
        row = {"N": N, "W": args.width, "H": args.height, "build": _lib.build_id(), "steps": args.steps, "blocks": args.blocks}
        for name, ts in times.items():
            row[name + "_ms"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            print(f"N={N:>8d} {name:>7s}: {statistics.median(ts):.3f} ms per view ({min(ts):.3f}..{max(ts):.3f})")
        for name, fn in legs.items():
            row[name + "_kernels_ms"] = kernels(fn, cams, args)
            print(f"N={N:>8d} {name:>7s}: " + ", ".join(f"{k} {v:.3f} ms" for k, v in row[name + "_kernels_ms"].items()) + " per view (profiled)")
        print(json.dumps(row))
        del pc, leaves


if __name__ == "__main__":
    main()
