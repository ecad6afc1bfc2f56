#!/usr/bin/env python3
"""Cost of the 3D smoothing filter (lightgaussian_amd/filter3d.py): alternating legs on one GPU in one run.

    update   filter3d.compute_filter_3d over --cams cameras of --size (lg_filter3d_update: one pass over the Gaussians)
             against the loop over cameras written in torch from the same semantics (about 15 elementwise launches per camera)
    apply    filter3d.apply_filter_3d forward + backward (lg_filter3d_apply / _apply_bwd, raw -> raw)
             against the same expression in torch under autograd
    render   render(cam, model, pipe, bg) and the backward of an image loss with the model's filter_3D honoured ("on")
             against the same call with options={"filter_3d": False} ("off")

    python tools/filter3d_bench.py [--n 3000000] [--size 1920x1080] [--cams 200] [--legs update apply render] [--steps 20] [--blocks 5]

Frozen benchmark scene (synthetic.make_gaussians, sigma 0.004), SH degree 3, orbit cameras.  Per pair of legs: `--blocks` alternating
blocks of `--steps` calls per leg after a warm-up (the update legs run --update-steps calls per block), each block between two
hipEvents; printed as median (min..max) of the per-call time over the blocks, and as one JSON line.  A difference is real only where the
two intervals do not overlap.

The comparand of the render "off" leg is the PARENT commit on the same box, never the code under test.  The parent's library lacks the
lg_filter3d_* entry points this tree's binding resolves at load, so it cannot be loaded through LIGHTGAUSSIAN_HIP_LIB here: time the
parent's checkout with its own `tools/antialias_bench.py --legs off --size 1920x1080` -- its train_off leg is this tool's render_off
leg, statement for statement -- and this tree with the same command, alternating the two processes."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, filter3d, rasterizer, synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402


def timed(legs, steps, blocks, warmup):
    """{leg: [ms per call of each block]}: a warm-up, then alternating blocks of `steps` calls per leg between two events."""
    for fn in legs.values():
        for k in range(warmup):
            fn(k)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(blocks):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(steps):
                fn(k)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / steps)
    return times


def torch_filter_3d(xyz, cams):
    """The update written in torch from the semantics of include/lightgaussian.h: one pass of elementwise launches per camera."""
    N = xyz.shape[0]
    t = torch.full((N,), float("inf"), device=xyz.device)
    seen = torch.zeros(N, dtype=torch.bool, device=xyz.device)
    for c in cams:
        vm = c.world_view_transform
        p = xyz @ vm[:3, :3] + vm[3, :3]
        z = p[:, 2]
        W, H = c.image_width, c.image_height
        fx, fy = W / (2.0 * math.tan(c.FoVx * 0.5)), H / (2.0 * math.tan(c.FoVy * 0.5))
        u, v = p[:, 0] / z * fx + 0.5 * W, p[:, 1] / z * fy + 0.5 * H
        s = (z > 0.2) & (u >= -0.15 * W) & (u <= 1.15 * W) & (v >= -0.15 * H) & (v <= 1.15 * H)
        t = torch.where(s, torch.minimum(t, z / fx), t)
        seen |= s
    f = math.sqrt(0.2) * t
    top = torch.where(seen, f, torch.zeros_like(f)).max()          # (0 when nobody is seen; no host read-back)
    return torch.where(seen, f, top)[:, None]


def torch_apply(r, o, f):
    s2 = torch.exp(r) ** 2
    u = s2 + f * f
    c = torch.sqrt((s2 / u).prod(1, keepdim=True))
    y = torch.sigmoid(o) * c
    return 0.5 * torch.log(u), torch.log(y / (1 - y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--legs", nargs="+", default=["update", "apply", "render"], choices=["update", "apply", "render"])
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--update-steps", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    pc = syn.make_gaussians(args.n).to(dev).requires_grad_(True)
    leaves = [pc._xyz, pc._features_dc, pc._features_rest, pc._scaling, pc._rotation, pc._opacity]
    train_cams = [syn.orbit_camera(k, args.cams, W, H).to(dev) for k in range(args.cams)]
    table = filter3d.camera_table(train_cams).to(dev)
    f, seen = filter3d.compute_filter_3d(pc._xyz, table, return_seen=True)
    row = {"N": args.n, "W": W, "H": H, "cams": args.cams, "build": _lib.build_id(), "steps": args.steps, "blocks": args.blocks,
           "seen": int(seen.sum()), "widened_10pct": int((torch.sqrt(torch.exp(pc._scaling.detach()) ** 2 + f * f) > 1.1 * torch.exp(pc._scaling.detach())).any(1).sum())}

    def report(times, unit):
        for name, ts in times.items():
            row[name + "_ms"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            print(f"{name:>12s}: {statistics.median(ts):.3f} ms per {unit} ({min(ts):.3f}..{max(ts):.3f})")

    if "update" in args.legs:
        with torch.no_grad():
            ref = torch_filter_3d(pc._xyz, train_cams)
            # agreement with the torch loop (its matmul rounds differently; a mean on a frustum border can flip one camera's decision)
            rel = (f - ref).abs() / ref.abs().clamp_min(1e-30)
            row["update_vs_torch"] = {"median_rel_diff": float(rel.median()), "max_rel_diff": float(rel.max()), "rows_over_1e-5": int((rel > 1e-5).sum())}
            print("update against the torch loop:", row["update_vs_torch"])
            report(timed({"update_hip": lambda k: filter3d.compute_filter_3d(pc._xyz, table),
                          "update_torch": lambda k: torch_filter_3d(pc._xyz, train_cams)}, args.update_steps, args.blocks, 1), "update")
    if "apply" in args.legs:
        gs, go = torch.randn_like(pc._scaling), torch.randn_like(pc._opacity)

        def apply_leg(fn):
            a, b = fn(pc._scaling, pc._opacity, f)
            torch.autograd.backward((a, b), (gs, go))
            pc._scaling.grad = pc._opacity.grad = None

        report(timed({"apply_hip": lambda k: apply_leg(filter3d.apply_filter_3d), "apply_torch": lambda k: apply_leg(torch_apply)},
                     args.steps, args.blocks, args.warmup), "forward + backward")
    if "render" in args.legs:
        G = torch.randn(3, H, W, device=dev, generator=torch.Generator(dev).manual_seed(0))
        cams = [syn.orbit_camera(k, args.views, W, H).to(dev) for k in range(args.views)]
        pc.filter_3D = f

        def train(cam, opts):
            (render(cam, pc, pipe, bg, options=opts)["render"] * G).sum().backward()
            for t in leaves:
                t.grad = None

        report(timed({"render_off": lambda k: train(cams[k % len(cams)], {"filter_3d": False}),
                      "render_on": lambda k: train(cams[k % len(cams)], {"filter_3d": True})}, args.steps, args.blocks, args.warmup), "view")
    # the four kernels on their own (option profile: per-kernel hipEvent times), one call each after a warm call
    for profiled in (False, True):
        _lib.profile_reset()
        with rasterizer.options(profile=profiled):
            filter3d.compute_filter_3d(pc._xyz, table)
            a, b = filter3d.apply_filter_3d(pc._scaling, pc._opacity, f)
            torch.autograd.backward((a, b), (torch.ones_like(a), torch.ones_like(b)))
            pc._scaling.grad = pc._opacity.grad = None
        torch.cuda.synchronize()
    row["kernel_ms"] = {k: round(v[0] / max(v[1], 1), 4) for k, v in _lib.profile_read().items() if k.startswith("filter3d")}
    print("kernels:", row["kernel_ms"])
    print(json.dumps(row))


if __name__ == "__main__":
    main()
