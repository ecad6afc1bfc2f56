#!/usr/bin/env python3
"""Cost of antialiased splatting (option "antialiasing", LG_FLAG_ANTIALIAS): alternating legs on one GPU in one run.

    train      render(cam, model, pipe, bg) and the backward of an image loss: K1 .. K6, K7, K9
    count      count_render(..., options={"skip_color_in_count": True}) under no_grad: the significance pass
each with the option off and on (--legs), at every --size.

    python tools/antialias_bench.py [--n 3000000] [--size 1920x1080 480x270] [--legs off on] [--steps 20] [--blocks 5]

Frozen benchmark scene (synthetic.make_gaussians, sigma 0.004), SH degree 3, orbit cameras.  Per size: `--blocks` alternating blocks of
`--steps` views per leg after a warm-up, each block between two hipEvents; printed as median (min..max) of the per-view time over the
blocks.  Then, per leg, one profiled view (option profile: per-kernel hipEvent times of K1 "preprocess" and K9 "preprocess_bwd") and
the view's visible count and instance count R (exact forward): the compensation removes instances, so K3 .. K7 may get cheaper.  One
JSON line per size.  A difference is real only where the two intervals do not overlap.

The comparand of the option-off legs is the PARENT commit's library on the same box, never the code under test: build it aside
(make -C lightgaussian_amd/csrc OUT=../variants/lib_parent.so at the parent), run this tool once with
LIGHTGAUSSIAN_HIP_LIB=<that file> --legs off and once without the variable --legs off on, and compare the `build` fields.  (A library
that predates the flag ignores it: never time an "on" leg through it.)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import count_render, render  # noqa: E402


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
    ap.add_argument("--n", type=int, default=3_000_000)
    ap.add_argument("--size", nargs="+", default=["1920x1080", "480x270"])
    ap.add_argument("--legs", nargs="+", default=["off", "on"], choices=["off", "on"])
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    pc = syn.make_gaussians(args.n).to(dev).requires_grad_(True)
    leaves = [pc._xyz, pc._features_dc, pc._features_rest, pc._scaling, pc._rotation, pc._opacity]
    for size in args.size:
        W, H = (int(v) for v in size.split("x"))
        G = torch.randn(3, H, W, device=dev, generator=torch.Generator(dev).manual_seed(0))
        cams = [syn.orbit_camera(k, args.views, W, H).to(dev) for k in range(args.views)]

        def train(cam, opts):
            (render(cam, pc, pipe, bg, options=opts)["render"] * G).sum().backward()
            for t in leaves:
                t.grad = None

        def count(cam, opts):
            with torch.no_grad():
                count_render(cam, pc, pipe, bg, options=dict(opts, skip_color_in_count=True))

        legs = {}
        for leg in args.legs:
            opts = {"antialiasing": leg == "on"}
            legs["train_" + leg] = lambda cam, o=opts: train(cam, o)
            legs["count_" + leg] = lambda cam, o=opts: count(cam, o)
        times = timed(legs, cams, args)
        row = {"N": args.n, "W": W, "H": H, "build": _lib.build_id(), "steps": args.steps, "blocks": args.blocks}
        for name, ts in times.items():
            row[name + "_ms"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            print(f"{size:>9s} {name:>9s}: {statistics.median(ts):.3f} ms per view ({min(ts):.3f}..{max(ts):.3f})")
        for leg in args.legs:
            # one view on the exact path (its num_rendered is the instance count R), profiled
            opts = {"antialiasing": leg == "on", "sync_free": False, "profile": True}
            _lib.profile_reset()
            pkg = render(cams[0], pc, pipe, bg, options=opts)
            (pkg["render"] * G).sum().backward()
            torch.cuda.synchronize()
            prof = _lib.profile_read()
            for t in leaves:
                t.grad = None
            row["view_" + leg] = {"visible": int((pkg["radii"] > 0).sum()), "R": int(pkg["render"].grad_fn.num_rendered),
                                  "kernel_ms": {k: round(v[0] / max(v[1], 1), 4) for k, v in prof.items()}}
            v = row["view_" + leg]
            print(f"{size:>9s} view 0 {leg:>3s}: visible {v['visible']}, R {v['R']}, K1 {v['kernel_ms'].get('preprocess')} ms, "
                  f"K9 {v['kernel_ms'].get('preprocess_bwd')} ms")
        print(json.dumps(row))


if __name__ == "__main__":
    main()
