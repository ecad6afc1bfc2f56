#!/usr/bin/env python3
"""The normals entry points alone and inside a training step, on one GPU in one run:

    rows        gaussian_normals forward + backward over N Gaussians             hip: lg_normal_rows + lg_normal_rows_bwd (two launches)
    depth       depth_to_normal forward + backward at W x H                       hip: lg_depth_normals + lg_depth_normals_bwd
    loss        normal_consistency_loss forward + backward at W x H               hip: lg_normal_loss (+ reduce) + lg_normal_loss_bwd
                each against backend="torch" of the same call on the same tensors: the op sequence a user writes without the library
    step        render_geometry + normal_consistency_loss, forward and backward, against render_features("depth", geometry_grad=True)
                with an L1 on depth and alpha, forward and backward: what the normals add to a geometry fine-tune step

    python tools/normals_bench.py [--n-gaussians 3000000] [--width 1920] [--height 1080] [--reps 10] [--blocks 7] [--only-hip] [--no-step]

The scene is bench.py's frozen workload (make_gaussians(N, log_scale_mean = log 0.004), orbit camera 0 of 200).  Per leg: a warm-up,
then `--blocks` alternating blocks of `--reps` calls, each block between two device events; printed as median (min..max) of the per-call
time over the blocks.  Byte models, stated before the run (float32, every tensor read or written once):
    rows    fwd 56 B per Gaussian (xyz 12, scaling 12, rotation 16, rows 16), bwd 84 B (+ dL/drows 16, dL/dxyz 12, dL/drotation 16 - rows)
    loss    fwd 20 B per pixel (N_r 12, depth 4, alpha 4), bwd 36 B (+ dL/dN_r 12, dL/ddepth 4); the strips' halo columns (2 of 64 lanes
            forward, 4 of 64 backward) and rows (2 of 34, 4 of 36) are re-read from cache
--only-hip runs the hip legs alone, for `rocprofv3 --kernel-trace --stats -- python tools/normals_bench.py --only-hip`."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, normals  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render_features, render_geometry  # noqa: E402

RAW = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=3_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scale", type=float, default=0.004)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench.py measures on a GPU; there is none")
    dev = torch.device("cuda", 0)
    N, W, H = args.n_gaussians, args.width, args.height
    kinds = ("hip",) if args.only_hip else ("torch", "hip")
    model = syn.make_gaussians(N, log_scale_mean=math.log(args.scale)).to(dev)
    cam = syn.orbit_camera(0, 200, W, H).to(dev)
    pipe = syn.PipelineParams()
    for n in RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    with torch.no_grad():
        pkg = render_geometry(cam, model, pipe, geometry_grad=False)
    normal, depth, alpha = (pkg[k].detach().clone() for k in ("normal", "depth", "alpha"))
    g_rows = torch.randn(N, 4, device=dev)
    g_nd = torch.randn(3, H, W, device=dev)
    print(f"library build {_lib.build_id()}, N = {N}, {W} x {H}, {args.blocks} blocks of {args.reps} calls per leg; "
          f"coverage (alpha > 0.5) {float((alpha > 0.5).float().mean()):.3f}")

    def rows_leg(kind):
        x, s, r = model._xyz.detach().clone().requires_grad_(), model._scaling.detach().clone(), model._rotation.detach().clone().requires_grad_()

        def call():
            torch.autograd.grad(normals.gaussian_normals(x, s, r, cam, backend=kind), (x, r), g_rows)
        return call

    def depth_leg(kind):
        d = depth.clone().requires_grad_()

        def call():
            torch.autograd.grad(normals.depth_to_normal(d, cam, backend=kind), (d,), g_nd)
        return call

    def loss_leg(kind):
        d, n = depth.clone().requires_grad_(), normal.clone().requires_grad_()

        def call():
            torch.autograd.grad(normals.normal_consistency_loss(n, d, alpha, cam, backend=kind), (n, d))
        return call

    def params():
        return [getattr(model, n) for n in RAW]

    def step_geometry():
        p = render_geometry(cam, model, pipe)
        loss = normals.normal_consistency_loss(p["normal"], p["depth"], p["alpha"], cam) + p["render"].mean()
        torch.autograd.grad(loss, params(), allow_unused=True)

    def step_depth():
        p = render_features(cam, model, pipe, "depth", geometry_grad=True)
        loss = p["depth"].mean() + p["alpha"].mean() + p["render"].mean()
        torch.autograd.grad(loss, params(), allow_unused=True)

    legs = {}
    for what, make in (("rows", rows_leg), ("depth", depth_leg), ("loss", loss_leg)):
        legs.update({(what, k): make(k) for k in kinds})
    if not args.no_step:
        legs[("step", "render_features_depth")] = step_depth
        legs[("step", "render_geometry_loss")] = step_geometry
    for fn in legs.values():
        timed(fn, 2)
    torch.cuda.synchronize()
    times = {key: [] for key in legs}
    for _ in range(args.blocks):
        for key, fn in legs.items():
            times[key].append(timed(fn, args.reps))
    model_bytes = {"rows": N * (56 + 84), "depth": W * H * (16 + 20), "loss": W * H * (20 + 36)}
    for key, t in times.items():
        line = f"  {key[0]:6s} {key[1]:22s} {statistics.median(t):9.4f} ms ({min(t):.4f}..{max(t):.4f})"
        if key[1] == "hip":
            b = model_bytes[key[0]]
            line += f"   {b / 1e6:.0f} MB by the byte model: {b / statistics.median(t) / 1e6:.0f} GB/s effective, forward + backward"
        print(line)
    print(json.dumps({"normals_bench": {"N": N, "W": W, "H": H, "reps": args.reps, "blocks": args.blocks, "build": _lib.build_id(),
                                        "model_bytes": model_bytes, "ms": {f"{a}_{b}": [round(x, 4) for x in t] for (a, b), t in times.items()}}}))


if __name__ == "__main__":
    main()
