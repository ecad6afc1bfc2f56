#!/usr/bin/env python3
"""What one view of the sensitivity pass costs next to one view of the significance pass of the same build, on one GPU in one run
(DESIGN section 10.14):

    a  sensitivity.accumulate      an ordinary colour forward without autograd, lg_sensitivity_walk (twelve moments per instance, one
                                   back-to-front walk of the lists), lg_sensitivity_accum (A^T M A per Gaussian into H [N, 21] float64)
    b  count_render                the significance forward (hit counts and the sum of alpha T) of prune_list
    c  render (no grad)            the forward alone: a - c is what the two new launches add

    python tools/sensitivity_bench.py [--n-gaussians 3000000] [--width 1920] [--height 1080] [--reps 10] [--blocks 7] [--only a]

The scene is bench.py's frozen workload (make_gaussians(N, log_scale_mean = log 0.004), orbit camera 0 of 200); the getters are
evaluated once for all three legs (prune._FrozenGetters, as sensitivity_list and the sharded significance pass do).  A warm-up, then
`--blocks` alternating blocks of `--reps` calls per leg, each block between two device events; printed as median (min..max) of the
per-call time over the blocks, then the kernels' own times from one profiled call of leg a (LG_FLAG_PROFILE: device events around each
launch), then lg_sensitivity_score over the N blocks.  --only a runs leg a alone, for
`rocprofv3 --kernel-trace --stats -- python tools/sensitivity_bench.py --only a`."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, sensitivity  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import count_render, render  # noqa: E402
from lightgaussian_amd.prune import _FrozenGetters  # noqa: E402


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
        raise SystemExit("sensitivity_bench.py measures on a GPU; there is none")
    dev = torch.device("cuda", 0)
    N, W, H = args.n_gaussians, args.width, args.height
    model = _FrozenGetters(syn.make_gaussians(N, log_scale_mean=math.log(args.scale)).to(dev))
    cam = syn.orbit_camera(0, 200, W, H).to(dev)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    Hacc = sensitivity.new_accumulator(N, dev)

    def step_a(options=None):
        sensitivity.accumulate(cam, model, pipe, bg, Hacc, options=options)

    def step_b():
        with torch.no_grad():
            count_render(cam, model, pipe, bg)

    def step_c():
        with torch.no_grad():
            render(cam, model, pipe, bg)

    legs = {"a_sensitivity_accumulate": step_a, "b_count_render": step_b, "c_render_no_grad": step_c}
    if args.only:
        legs = {k: v for k, v in legs.items() if k.startswith(args.only)}
    print(f"library build {_lib.build_id()}, N = {N}, {W} x {H}, {args.blocks} blocks of {args.reps} calls per leg")
    for fn in legs.values():
        timed(fn, 2)
    torch.cuda.synchronize()
    times = {key: [] for key in legs}
    for _ in range(args.blocks):
        for key, fn in legs.items():
            times[key].append(timed(fn, args.reps))
    for key, t in times.items():
        print(f"  {key:28s} {statistics.median(t):9.4f} ms ({min(t):.4f}..{max(t):.4f})")
    med = {k: statistics.median(t) for k, t in times.items()}
    if len(med) == 3:
        a, b, c = (med[k] for k in legs)
        print(f"  a - c = {a - c:+.4f} ms;  a / b = {a / b:.3f}  (boxes differ by +-3 %: inside that is 'equal')")
    kernels, score_ms = {}, None
    if "a_sensitivity_accumulate" in legs:
        _lib.profile_reset()
        step_a(options={"profile": True})
        torch.cuda.synchronize()
        kernels = {k: (round(ms, 4), n) for k, (ms, n) in _lib.profile_read().items()}
        for k, (ms, n) in sorted(kernels.items(), key=lambda kv: -kv[1][0]):
            print(f"  profiled call of a: {k:24s} {ms:8.4f} ms in {n} launch(es)")
        score_ms = timed(lambda: sensitivity.score(Hacc, model, "log"), args.reps)
        s = sensitivity.score(Hacc, model, "log")
        print(f"  lg_sensitivity_score over {N} blocks: {score_ms:.4f} ms; after {2 + args.blocks * args.reps + 1} accumulations of one view "
              f"{int(torch.isfinite(s).sum())} finite scores (one view spans five directions: -inf is expected)")
    print(json.dumps({"sensitivity_bench": {"N": N, "W": W, "H": H, "reps": args.reps, "blocks": args.blocks, "build": _lib.build_id(),
                                            "ms": {k: [round(x, 4) for x in t] for k, t in times.items()}, "profiled_a": kernels,
                                            "score_ms": score_ms}}))


if __name__ == "__main__":
    main()
