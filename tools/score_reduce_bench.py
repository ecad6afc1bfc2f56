#!/usr/bin/env python3
"""Cost of score_reduce="max" against "sum" in the significance pass: alternating legs on one GPU in one run.

    python tools/score_reduce_bench.py [--n 3000000] [--size 1920x1080] [--views 200] [--blocks 7] [--policy alpha_t]

Each leg is prune_list_sharded(weight_policy=--policy, score_reduce=leg) over --views orbit cameras of the frozen benchmark scene
(synthetic.make_gaussians, SH degree 3): the significance-only kernels, 4 views in flight, sync-free forwards -- the pass as the prune
step runs it.  After a warm-up pass per leg, --blocks alternating blocks of one pass per leg, each between two hipEvents; printed as
median (min..max) of the per-view time over the blocks, and one JSON line.  A difference is real only where the two intervals do not
overlap.  The "sum" leg runs kernels that are instruction-identical to those before the option existed (tools/isa_diff.py): it is the
comparand.  Before the timing the two legs' hit counts are compared (they must be equal) and max <= sum is checked per Gaussian."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, synthetic as syn  # noqa: E402
from lightgaussian_amd.prune import prune_list_sharded  # noqa: E402

LEGS = ("sum", "max")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--policy", default="alpha_t", choices=["alpha", "alpha_t"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    pc = syn.make_gaussians(args.n).to(dev)
    cams = [syn.orbit_camera(k, args.views, W, H).to(dev) for k in range(args.views)]
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)

    def run(leg):
        with torch.no_grad():
            return prune_list_sharded(pc, cams, pipe, bg, weight_policy=args.policy, score_reduce=leg, streams=args.streams)

    first = {leg: run(leg) for leg in LEGS}                # warm-up of every shape the timed window uses, and the sanity of the comparison
    torch.cuda.synchronize()
    assert torch.equal(first["sum"][0], first["max"][0]), "hit counts differ between the legs"
    assert bool((first["max"][1] <= first["sum"][1] * (1 + 1e-6) + 1e-12).all()), "a maximum above its sum"
    times = {leg: [] for leg in LEGS}
    for _ in range(args.blocks):
        for leg in LEGS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(leg)
            b.record()
            b.synchronize()
            times[leg].append(a.elapsed_time(b) / args.views)
    row = {"N": args.n, "W": W, "H": H, "views": args.views, "blocks": args.blocks, "streams": args.streams, "policy": args.policy,
           "build": _lib.build_id(), "hits": int(first["sum"][0].sum())}
    for leg, ts in times.items():
        row[leg + "_ms_per_view"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
        print(f"{args.size:>9s} {args.policy} {leg}: {statistics.median(ts):.3f} ms per view ({min(ts):.3f}..{max(ts):.3f}), "
              f"{1e3 / statistics.median(ts):.0f} views/s")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
