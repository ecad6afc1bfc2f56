#!/usr/bin/env python3
"""A triangle mesh from a Gaussian model through the block-sparse TSDF volume, at a voxel size whose box would not fit densely:

    fuse      mesh.fuse_views over an orbit into a blocks.BlockTSDFVolume: per batch of 8 views the blocks their depth maps touch are
              allocated (lg_blocks_touch, lg_blocks_merge, lg_blocks_regrid), then integrated (lg_blocks_integrate)
    extract   BlockTSDFVolume.extract_mesh: marching tetrahedra across block borders (lg_blocks_mesh_count, lg_blocks_mesh_emit)

    python examples/mesh_extract_sparse.py [--n-gaussians 60000] [--views 24] [--voxel 0.004] [--extent 60] [--out mesh.ply]

The scene is examples/mesh_extract.py's shell of flat Gaussians about the unit sphere, taken as a small object in a capture `--extent`
units wide.  At --voxel 0.004 a dense volume over that box would hold 15000^3 points (3.4e12, against the 2^29 a TSDFVolume may hold);
the shell needs some tens of thousands of blocks of 512 points.  Printed: the blocks, their bytes and what the dense box would
take, the vertex and face counts, the surface area (the sphere: 4 pi = 12.57) and the mean distance of the vertices from the sphere in
voxels.  The PLY file (binary little-endian, with vertex colours) opens in MeshLab or Blender."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import blocks, mesh  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402

from mesh_extract import sphere_shell, surface  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=60_000)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--extent", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    model = sphere_shell(args.n_gaussians).to(dev)
    cameras = [syn.orbit_camera(k, args.views, args.width, args.height, radius=4.0, height_y=(-1.5, 0.8, 2.5)[k % 3]).to(dev) for k in range(args.views)]
    side = int(math.ceil(args.extent / args.voxel))
    print(f"a dense volume over {args.extent} units at voxel {args.voxel}: {side}^3 = {side ** 3:.2e} points, {20 * side ** 3 / 2 ** 40:.0f} TiB "
          f"(mesh.TSDFVolume holds fewer than 2^29 = {2 ** 29:.2e})")
    # the lattice is unbounded: the origin only fixes where lattice point (0, 0, 0) lies, here a corner of the capture
    vol = blocks.BlockTSDFVolume(args.voxel, origin=(-0.5 * args.extent,) * 3, device=dev)
    mesh.fuse_views(cameras, model, pipe, vol)
    v, f, c = vol.extract_mesh()
    off = float(((v.norm(dim=1) - 1).abs() / args.voxel).mean()) if len(v) else float("nan")
    lo, hi = vol.coords().min(dim=0).values.tolist(), vol.coords().max(dim=0).values.tolist()
    print(f"  {vol.n_blocks} blocks ({vol.nbytes() / 2 ** 20:.0f} MiB), block coordinates {lo} .. {hi}")
    print(f"  {len(v)} vertices, {len(f)} faces, area {surface(v, f):.3f} (sphere: {4 * math.pi:.3f}), vertices {off:.2f} voxel from the sphere on average")
    if args.out:
        mesh.save_ply(args.out, v, f, c)
        print(f"  wrote {args.out}")


if __name__ == "__main__":
    main()
