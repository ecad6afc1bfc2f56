#!/usr/bin/env python3
"""What the depth distortion and median depth maps add to a geometry fine-tune step, on one GPU in one run:

    a  render_geometry(distortion=True) + normal_consistency_loss + distortion.mean()      the feature: one forward, lg_blend_features +
                                                                                            lg_blend_distortion, ONE lg_backward_distortion
    b  render_features([n, z, z z], geometry_grad=True) + the same consistency loss        the composed step, the comparand and nothing else:
       + (alpha F2 - F1^2).mean() in torch                                                 five blended channels, A M2 - M1^2 (which cancels
                                                                                            in float32 on thin, distant surfaces)
    c  render_geometry() + normal_consistency_loss                                          the parent's step of section 10.11

each forward AND backward to every raw parameter (the colour image's mean joins each loss, as in tools/normals_bench.py).

    python tools/distortion_bench.py [--n-gaussians 3000000] [--width 1920] [--height 1080] [--reps 10] [--blocks 7] [--only a]

The scene is bench.py's frozen workload (make_gaussians(N, log_scale_mean = log 0.004), orbit camera 0 of 200).  A warm-up, then
`--blocks` alternating blocks of `--reps` calls per leg, each block between two device events; printed as median (min..max) of the
per-call time over the blocks, then the two new kernels' own times from one profiled call of leg a (LG_FLAG_PROFILE: device events around
each launch).  --only a runs leg a alone, for `rocprofv3 --kernel-trace --stats -- python tools/distortion_bench.py --only a`."""
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
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distortion_bench.py measures on a GPU; there is none")
    dev = torch.device("cuda", 0)
    N, W, H = args.n_gaussians, args.width, args.height
    model = syn.make_gaussians(N, log_scale_mean=math.log(args.scale)).to(dev)
    cam = syn.orbit_camera(0, 200, W, H).to(dev)
    pipe = syn.PipelineParams()
    for n in RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))

    def params():
        return [getattr(model, n) for n in RAW]

    def step_a(options=None):
        p = render_geometry(cam, model, pipe, distortion=True, options=options)
        loss = normals.normal_consistency_loss(p["normal"], p["depth"], p["alpha"], cam) + p["distortion"].mean() + p["render"].mean()
        torch.autograd.grad(loss, params(), allow_unused=True)
        return p

    def step_b():
        rows = normals.gaussian_normals(model.get_xyz.contiguous(), model.get_scaling.contiguous(), model.get_rotation.contiguous(), cam)
        z = rows[:, 3:4]
        p = render_features(cam, model, pipe, torch.cat([rows, z * z], 1).contiguous(), geometry_grad=True)
        f, alpha = p["features"], p["alpha"]
        depth = f[3] / alpha.clamp_min(1e-6)
        loss = normals.normal_consistency_loss(f[:3], depth, alpha, cam) + (alpha * f[4] - f[3] * f[3]).mean() + p["render"].mean()
        torch.autograd.grad(loss, params(), allow_unused=True)

    def step_c():
        p = render_geometry(cam, model, pipe)
        loss = normals.normal_consistency_loss(p["normal"], p["depth"], p["alpha"], cam) + p["render"].mean()
        torch.autograd.grad(loss, params(), allow_unused=True)

    legs = {"a_render_geometry_distortion": step_a, "b_composed_render_features": step_b, "c_render_geometry": step_c}
    if args.only:
        legs = {k: v for k, v in legs.items() if k.startswith(args.only)}
    with torch.no_grad():
        p = render_geometry(cam, model, pipe, geometry_grad=False, distortion=True)
    print(f"library build {_lib.build_id()}, N = {N}, {W} x {H}, {args.blocks} blocks of {args.reps} calls per leg; "
          f"coverage (alpha > 0.5) {float((p['alpha'] > 0.5).float().mean()):.3f}, mean distortion {float(p['distortion'].mean()):.3e}")
    for fn in legs.values():
        timed(fn, 2)
    torch.cuda.synchronize()
    times = {key: [] for key in legs}
    for _ in range(args.blocks):
        for key, fn in legs.items():
            times[key].append(timed(fn, args.reps))
    for key, t in times.items():
        print(f"  {key:30s} {statistics.median(t):9.4f} ms ({min(t):.4f}..{max(t):.4f})")
    med = {k: statistics.median(t) for k, t in times.items()}
    if len(med) == 3:
        a, b, c = (med[k] for k in legs)
        print(f"  a - c = {a - c:+.4f} ms ({100.0 * (a - c) / c:+.1f} % of c);  a / b = {a / b:.3f}  (boxes differ by +-3 %: inside that is 'equal')")
    kernels = {}
    if "a_render_geometry_distortion" in legs:
        _lib.profile_reset()
        step_a(options={"profile": True})
        torch.cuda.synchronize()
        kernels = {k: (round(ms, 4), n) for k, (ms, n) in _lib.profile_read().items()}
        for k, (ms, n) in sorted(kernels.items(), key=lambda kv: -kv[1][0]):
            print(f"  profiled call of a: {k:24s} {ms:8.4f} ms in {n} launch(es)")
    print(json.dumps({"distortion_bench": {"N": N, "W": W, "H": H, "reps": args.reps, "blocks": args.blocks, "build": _lib.build_id(),
                                           "ms": {k: [round(x, 4) for x in t] for k, t in times.items()}, "profiled_a": kernels}}))


if __name__ == "__main__":
    main()
