#!/usr/bin/env python3
"""The block-sparse TSDF volume against the dense one, and where the dense one cannot exist, on one GPU in one run:

    a  --lattice cubed (512): the unit sphere's shell in a box of 3 units, mesh.TSDFVolume over the whole box against
       blocks.BlockTSDFVolume over the blocks the views touch: allocate + integrate from an empty volume, integrate into the allocated
       blocks, and extract_mesh(drop_unreferenced=False), for --views (8 64) views; the bytes of both volumes
    b  the same shell at the voxel size of a --big cubed (4096) box, which no dense volume can hold (2^36 points): the sparse legs alone,
       with the blocks and bytes

    python tools/blocks_bench.py [--lattice 512] [--big 4096] [--views 8 64] [--width 1920] [--height 1080] [--blocks 5] [--seconds 0.3] [--only a|b]

The views are tools/mesh_bench.py's analytic z-depth maps of the unit sphere with random colour images, n cameras on an eighth of an orbit
(radius 4, two heights), so that case b stays below the 2^20 blocks a volume holds (a leg whose volume is refused is left out and
named).  Per leg: a warm-up, then `--blocks` alternating blocks, each of as many calls as fill `--seconds`, each block between two device events; printed as median (min..max) of the per-call
time over the blocks.  "allocate + integrate" starts from clear() every call: lg_blocks_touch, lg_blocks_merge, the read-back of the
block count, lg_blocks_regrid and lg_blocks_integrate."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lightgaussian_amd import _lib, blocks, mesh  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402
from mesh_bench import sphere_view, timed  # noqa: E402

ORIGIN = (-1.5 + 0.0123, -1.5 - 0.0071, -1.5 + 0.0049)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--big", type=int, default=4096)
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--only", choices=("a", "b"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blocks_bench.py measures on a GPU; there is none")
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    gen = torch.Generator().manual_seed(0)
    views = {n: [sphere_view(syn.orbit_camera(k, 8 * n, W, H, radius=4.0, height_y=-1.5 if k % 2 == 0 else 0.8), W, H, dev, gen) for k in range(n)] for n in args.views}
    print(f"library build {_lib.build_id()}, {W} x {H} maps, lattice {args.lattice}^3 and {args.big}^3, views {args.views}, {args.blocks} blocks of >= {args.seconds} s per leg")

    legs, facts = {}, {}

    def sparse_legs(case, size):
        voxel = 3.0 / (size - 1)
        for n in args.views:
            vol = blocks.BlockTSDFVolume(voxel, origin=ORIGIN, device=dev)
            try:
                stats = vol.allocate(views[n])
            except ValueError as e:
                facts[f"{case} sparse {size}^3 n={n}"] = dict(refused=str(e))
                continue
            facts[f"{case} sparse {size}^3 n={n}"] = dict(blocks=vol.n_blocks, bytes=vol.nbytes(), skipped_pixels=stats["skipped_pixels"])

            def fresh(vol=vol, n=n):
                vol.clear()
                vol.integrate_many(views[n])
            legs[(f"{case} allocate + integrate {size}^3 n={n}", "sparse")] = fresh
            legs[(f"{case} integrate {size}^3 n={n}", "sparse")] = (lambda vol=vol, n=n: vol.integrate_many(views[n], allocate=False))
        fused = blocks.BlockTSDFVolume(voxel, origin=ORIGIN, device=dev)
        try:
            fused.integrate_many(views[args.views[0]])
        except ValueError:
            return None
        legs[(f"{case} extract {size}^3 n={args.views[0]}", "sparse")] = lambda: fused.extract_mesh(drop_unreferenced=False)
        return fused

    fused = {}
    if args.only != "b":
        size = args.lattice
        dense = mesh.TSDFVolume(ORIGIN, (size, size, size), 3.0 / (size - 1), device=dev)
        facts[f"a dense {size}^3"] = dict(points=size ** 3, bytes=sum(t.numel() * 4 for t in (dense.tsdf, dense.weight, dense.color)))
        for n in args.views:
            legs[(f"a integrate {size}^3 n={n}", "dense")] = (lambda n=n: dense.integrate_many(views[n]))
        dfused = mesh.TSDFVolume(ORIGIN, (size, size, size), 3.0 / (size - 1), device=dev)
        dfused.integrate_many(views[args.views[0]])
        legs[(f"a extract {size}^3 n={args.views[0]}", "dense")] = lambda: dfused.extract_mesh(drop_unreferenced=False)
        fused["a"] = (sparse_legs("a", size), dfused)
    if args.only != "a":
        fused["b"] = (sparse_legs("b", args.big), None)

    reps = {}
    for key, fn in legs.items():                     # warm-up, and the number of calls that fill a block
        timed(fn, 1)
        reps[key] = max(1, int(math.ceil(args.seconds * 1e3 / max(timed(fn, 1), 1e-3))))
    torch.cuda.synchronize()
    times = {key: [] for key in legs}
    for _ in range(args.blocks):
        for key, fn in legs.items():
            times[key].append(timed(fn, reps[key]))
    for case, (s, d) in fused.items():
        if s is None:
            continue
        v, f, _c = s.extract_mesh(drop_unreferenced=False)
        facts[f"{case} sparse mesh"] = dict(blocks=s.n_blocks, vertices=int(v.shape[0]), faces=int(f.shape[0]))
        if d is not None:
            v, f, _c = d.extract_mesh(drop_unreferenced=False)
            facts[f"{case} dense mesh"] = dict(vertices=int(v.shape[0]), faces=int(f.shape[0]))
    for name, fact in facts.items():
        print(f"  {name:28s} " + ", ".join(f"{k} {v}" for k, v in fact.items()))
    out = {}
    for key, t in times.items():
        med = statistics.median(t)
        print(f"  {key[0]:38s} {key[1]:7s} {med:10.4f} ms ({min(t):.4f}..{max(t):.4f}), {reps[key]} calls per block")
        out[f"{key[0]} {key[1]}"] = [round(x, 4) for x in t]
    print(json.dumps({"blocks_bench": {"W": W, "H": H, "lattice": args.lattice, "big": args.big, "views": args.views, "blocks": args.blocks,
                                       "build": _lib.build_id(), "facts": facts, "ms": out}}))


if __name__ == "__main__":
    main()
