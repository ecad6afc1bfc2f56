#!/usr/bin/env python3
"""TSDF fusion and mesh extraction on one GPU in one run:

    integrate   TSDFVolume.integrate_many over n views (one lg_tsdf_integrate call, 8 views per pass over the volume) against n
                integrate calls of one view each (the same kernel, one pass per view), at --sizes cubed with colour, and against
                backend="torch" at the first size
    extract     extract_mesh(drop_unreferenced=False) of the fused first-size volume, hip against backend="torch"

    python tools/mesh_bench.py [--sizes 256 512] [--views 8 64] [--width 1920] [--height 1080] [--blocks 5] [--seconds 0.3] [--only-hip]

The views are analytic z-depth maps of the unit sphere under orbit cameras (radius 4, two heights) with random colour images; the volume
spans 3 units about the origin.  Per leg: a warm-up, then `--blocks` alternating blocks, each of as many calls as fill `--seconds`, each
block between two device events; printed as median (min..max) of the per-call time over the blocks.  Byte model, stated before the run
(float32): a pass over the volume reads and writes tsdf, weight and colour of every point once, 20 + 20 B per point (8 + 8 without
colour); the depth, colour and alpha gathers are neighbouring pixels for neighbouring points and are left out.  integrate_many makes
ceil(n / 8) passes, n single calls make n; the effective rate is passes x 40 B x points / time, quoted as a fraction of 6.3 TB/s.
--only-hip runs the hip legs alone, for `rocprofv3 --kernel-trace --stats -- python tools/mesh_bench.py --only-hip`."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, mesh  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402

PEAK = 6.3e12


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def sphere_view(cam, W, H, dev, gen):
    """dict of integrate's arguments: the unit sphere's z-depth at the pixel centres (0 where the ray misses), a random image."""
    vm = cam.world_view_transform.double()
    c = (torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64) @ vm)[:3].to(dev)
    tx, ty = mesh.tanfov(cam)
    rx = ((2 * torch.arange(W, dtype=torch.float64, device=dev) + 1) / W - 1) * tx
    ry = ((2 * torch.arange(H, dtype=torch.float64, device=dev) + 1) / H - 1) * ty
    d = torch.stack([rx[None, :].expand(H, W), ry[:, None].expand(H, W), torch.ones(H, W, dtype=torch.float64, device=dev)], dim=-1)
    a, b, cc = (d * d).sum(-1), -2 * (d @ c), float(c @ c) - 1.0
    disc = b * b - 4 * a * cc
    s = (-b - disc.clamp_min(0).sqrt()) / (2 * a)
    depth = torch.where((disc > 0) & (s > 0), s, torch.zeros_like(s)).float().contiguous()
    return dict(depth=depth, camera=cam.to(dev), color=torch.rand(3, H, W, generator=gen).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--only-hip", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench.py measures on a GPU; there is none")
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    gen = torch.Generator().manual_seed(0)
    distinct = [sphere_view(syn.orbit_camera(k, 16, W, H, radius=4.0, height_y=-1.5 if k % 2 == 0 else 0.8), W, H, dev, gen) for k in range(16)]
    views = {n: [distinct[k % 16] for k in range(n)] for n in args.views}
    print(f"library build {_lib.build_id()}, {W} x {H} maps, sizes {args.sizes}, views {args.views}, {args.blocks} blocks of >= {args.seconds} s per leg")

    def volume(size, backend="hip"):
        voxel = 3.0 / (size - 1)
        return mesh.TSDFVolume((-1.5 + 0.0123, -1.5 - 0.0071, -1.5 + 0.0049), (size, size, size), voxel, device=dev, backend=backend)

    legs, passes = {}, {}
    for size in args.sizes:
        vol = volume(size)
        for n in args.views:
            legs[(f"integrate {size}^3 n={n}", "hip batched")] = (lambda vol=vol, n=n: vol.integrate_many(views[n]))
            legs[(f"integrate {size}^3 n={n}", "hip single")] = (lambda vol=vol, n=n: [vol.integrate(**v) for v in views[n]])
            passes[(f"integrate {size}^3 n={n}", "hip batched")] = ((n + mesh.BATCH - 1) // mesh.BATCH, size)
            passes[(f"integrate {size}^3 n={n}", "hip single")] = (n, size)
    first = args.sizes[0]
    fused = volume(first)
    fused.integrate_many(distinct)
    legs[(f"extract {first}^3", "hip")] = lambda: fused.extract_mesh(drop_unreferenced=False)
    if not args.only_hip:
        tvol = volume(first, backend="torch")
        n0 = args.views[0]
        legs[(f"integrate {first}^3 n={n0}", "torch")] = lambda: tvol.integrate_many(views[n0])
        tfused = volume(first, backend="torch")
        tfused.tsdf.copy_(fused.tsdf); tfused.weight.copy_(fused.weight); tfused.color.copy_(fused.color)
        legs[(f"extract {first}^3", "torch")] = lambda: tfused.extract_mesh(drop_unreferenced=False)
    reps = {}
    for key, fn in legs.items():                     # warm-up, and the number of calls that fill a block
        timed(fn, 1)
        reps[key] = max(1, int(math.ceil(args.seconds * 1e3 / max(timed(fn, 1), 1e-3))))
    torch.cuda.synchronize()
    times = {key: [] for key in legs}
    for _ in range(args.blocks):
        for key, fn in legs.items():
            times[key].append(timed(fn, reps[key]))
    v, f, _c = fused.extract_mesh(drop_unreferenced=False)
    print(f"  the fused {first}^3 volume: {v.shape[0]} vertices, {f.shape[0]} faces")
    out = {}
    for key, t in times.items():
        med = statistics.median(t)
        line = f"  {key[0]:26s} {key[1]:12s} {med:10.4f} ms ({min(t):.4f}..{max(t):.4f}), {reps[key]} calls per block"
        if key in passes:
            p, size = passes[key]
            nbytes = p * 40 * size ** 3
            line += f"   {p} passes, {nbytes / 1e9:.2f} GB by the byte model: {nbytes / med / 1e9:.2f} TB/s = {100 * nbytes / (med * 1e-3) / PEAK:.0f} % of 6.3 TB/s"
        print(line)
        out[f"{key[0]} {key[1]}"] = [round(x, 4) for x in t]
    print(json.dumps({"mesh_bench": {"W": W, "H": H, "sizes": args.sizes, "views": args.views, "blocks": args.blocks, "build": _lib.build_id(),
                                     "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "ms": out}}))


if __name__ == "__main__":
    main()
