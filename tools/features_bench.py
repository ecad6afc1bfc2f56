#!/usr/bin/env python3
"""C feature channels of one view, two legs on one GPU in one run:

    features   gaussian_renderer.render_features: ONE forward, then lg_blend_features over its tile lists
               (forward + backward: lg_blend_features_backward, the gradient with respect to the features)
    passes     what the library offered before: the colour forward plus ceil(C / 3) further render(..., override_color=...)
               forwards, each with its own K1 / scan / duplicate / sort / tile sort (forward + backward: each pass's backward
               through K7 / K9, the gradient with respect to its three colours)

    geom       (--geom-channels, default 1 8 32; 1 = "depth") forward + backward with geometry_grad=True: one forward, one
               lg_backward_features (a list walk per group of channels, K9 once) -- against the only way the library had to carry
               channel gradients to the geometry: ceil(C / 3) render(..., override_color=...) forward + backward passes

    python tools/features_bench.py [--n 1000000 3000000] [--channels 3 8 32] [--geom-channels 1 8 32] [--steps 20] [--blocks 5]

Frozen benchmark scene (synthetic.make_gaussians, sigma 0.004) at 1920 x 1080, SH degree 3, orbit cameras.  Per (N, C): `--blocks`
alternating blocks of `--steps` views per leg after a warm-up, each block between two hipEvents; printed as median (min..max) of the
per-view time over the blocks, and one JSON line per (N, C).  A speed-up is real only where the two intervals do not overlap."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render, render_features  # noqa: E402


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


def geometry_legs(pc, C, N, H, W, dev, gen, pipe, bg):
    """The two legs of the geometry-gradient comparison on a grad-enabled copy of the model."""
    pcg = syn.SyntheticGaussians(*(getattr(pc, n).detach().clone().requires_grad_(True) for n in ("_xyz", "_features_dc", "_features_rest", "_scaling",
                                                                                                   "_rotation", "_opacity")),
                                 pc.active_sh_degree, pc.max_sh_degree)
    leaves = [pcg._xyz, pcg._features_dc, pcg._features_rest, pcg._scaling, pcg._rotation, pcg._opacity]
    F = torch.randn(N, C, device=dev, generator=gen)
    G = torch.randn(C, H, W, device=dev, generator=gen)
    npass = (C + 2) // 3
    Fp = torch.cat([F, torch.zeros(N, 3 * npass - C, device=dev)], 1)
    Gp = torch.cat([G, torch.zeros(3 * npass - C, H, W, device=dev)], 0)
    triples = [Fp[:, 3 * k:3 * k + 3].contiguous() for k in range(npass)]

    def clear():
        for p in leaves:
            p.grad = None

    def geom_fwdbwd(cam):
        clear()
        (render_features(cam, pcg, pipe, "depth" if C == 1 else F, geometry_grad=True)["features"] * G).sum().backward()

    def passes_geom_fwdbwd(cam):
        clear()
        for k, t in enumerate(triples):
            (render(cam, pcg, pipe, bg, override_color=t)["render"] * Gp[3 * k:3 * k + 3]).sum().backward()

    return {"geom fwd+bwd": geom_fwdbwd, "passes fwd+bwd (geometry)": passes_geom_fwdbwd}, npass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--channels", type=int, nargs="*", default=[3, 8, 32])
    ap.add_argument("--geom-channels", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--scale", type=float, default=0.004)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    print(f"library build {_lib.build_id()}, {W}x{H}, SH degree {args.degree}, {args.blocks} blocks of {args.steps} views per leg")
    for N in args.n:
        pc = syn.make_gaussians(N, sh_degree=args.degree, log_scale_mean=math.log(args.scale)).to(dev)
        cams = [syn.orbit_camera(k, args.views, W, H).to(dev) for k in range(args.views)]
        gen = torch.Generator(device=dev).manual_seed(N)
        for C in args.channels:
            F = torch.randn(N, C, device=dev, generator=gen)
            G = torch.randn(C, H, W, device=dev, generator=gen)
            npass = (C + 2) // 3
            Fp = torch.cat([F, torch.zeros(N, 3 * npass - C, device=dev)], 1)
            Gp = torch.cat([G, torch.zeros(3 * npass - C, H, W, device=dev)], 0)
            triples = [Fp[:, 3 * k:3 * k + 3].contiguous() for k in range(npass)]
            Fg = F.clone().requires_grad_(True)
            triples_g = [t.clone().requires_grad_(True) for t in triples]

            def features_fwd(cam):
                with torch.no_grad():
                    render_features(cam, pc, pipe, F)

            def features_fwdbwd(cam):
                Fg.grad = None
                (render_features(cam, pc, pipe, Fg)["features"] * G).sum().backward()

            def passes_fwd(cam):
                with torch.no_grad():
                    render(cam, pc, pipe, bg)
                    for t in triples:
                        render(cam, pc, pipe, bg, override_color=t)

            def passes_fwdbwd(cam):
                with torch.no_grad():
                    render(cam, pc, pipe, bg)
                for k, t in enumerate(triples_g):
                    t.grad = None
                    (render(cam, pc, pipe, bg, override_color=t)["render"] * Gp[3 * k:3 * k + 3]).sum().backward()

            legs = {"features fwd": features_fwd, "passes fwd": passes_fwd, "features fwd+bwd": features_fwdbwd, "passes fwd+bwd": passes_fwdbwd}
            times = timed(legs, cams, args)
            print(f"N = {N}, C = {C} ({npass} override_color passes in the `passes` leg)")
            for name, t in times.items():
                print(f"  {name:18s} {statistics.median(t):8.3f} ms ({min(t):.3f}..{max(t):.3f})")
            print(json.dumps({"features_bench": {"N": N, "C": C, "W": W, "H": H, "steps": args.steps, "blocks": args.blocks, "build": _lib.build_id(),
                                                 "ms_per_view": {k: [round(x, 4) for x in v] for k, v in times.items()}}}))
            del F, G, Fp, Gp, triples, Fg, triples_g
        for C in args.geom_channels:
            legs, npass = geometry_legs(pc, C, N, H, W, dev, gen, pipe, bg)
            times = timed(legs, cams, args)
            print(f"N = {N}, C = {C}{' (depth)' if C == 1 else ''}, gradients to the geometry ({npass} override_color passes in the `passes` leg)")
            for name, t in times.items():
                print(f"  {name:26s} {statistics.median(t):8.3f} ms ({min(t):.3f}..{max(t):.3f})")
            print(json.dumps({"features_bench_geom": {"N": N, "C": C, "W": W, "H": H, "steps": args.steps, "blocks": args.blocks, "build": _lib.build_id(),
                                                      "ms_per_view": {k: [round(x, 4) for x in v] for k, v in times.items()}}}))
            del legs
        del pc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
