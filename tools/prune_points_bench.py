#!/usr/bin/env python3
"""prune.prune_points alone, on the stand-in model of tests/test_gpu_compact.py (six parameters at SH degree 3 with both Adam moments and
the three bookkeeping tensors: 21 tensors), 66 % of the rows pruned, on one GPU:

    python tools/prune_points_bench.py [--n 1000000 3000000] [--reps 5] [--blocks 7]

Every call starts from a fresh copy of the same state (building it is outside the timed region) and is timed between two hipEvents; printed
as median (min..max) of the per-call time over the blocks, after a warm-up call.  The time includes the Python layer: the optimizer walk, the
one read-back of the kept count, the new Parameters and the re-keyed state (lightgaussian_amd.model_rows)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_compact as tc  # noqa: E402
from lightgaussian_amd import _lib, prune  # noqa: E402

DEV = "cuda:0"
NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def copy_of(src):
    m = object.__new__(tc._Model)
    for n in NAMES:
        setattr(m, n, torch.nn.Parameter(getattr(src, n).detach().clone()))
    groups = [{"params": [getattr(m, n)], "lr": 1e-3, "name": g["name"]} for n, g in zip(NAMES, src.optimizer.param_groups)]
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for n in NAMES:
        m.optimizer.state[getattr(m, n)] = {k: v.clone() for k, v in src.optimizer.state[getattr(src, n)].items()}
    m.xyz_gradient_accum, m.denom, m.max_radii2D = src.xyz_gradient_accum.clone(), src.denom.clone(), src.max_radii2D.clone()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=7)
    args = ap.parse_args()
    print(f"library build {_lib.build_id()}, {args.blocks} blocks of {args.reps} calls")
    for N in args.n:
        src = tc._Model(N, 3, steps=1)
        mask = (torch.rand(N, generator=torch.Generator().manual_seed(9)) < 0.66).to(DEV)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def call():
            m = copy_of(src)
            torch.cuda.synchronize()
            a.record()
            prune.prune_points(m, mask)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        call()
        t = [sum(call() for _ in range(args.reps)) / args.reps for _ in range(args.blocks)]
        print(f"  prune_points N = {N}: {statistics.median(t):9.4f} ms ({min(t):.4f}..{max(t):.4f})")
        del src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
