#!/usr/bin/env python3
"""A triangle mesh from a Gaussian model, before and after a prune, on a synthetic scene:

    fuse      mesh.fuse_views over an orbit: render_geometry per camera (median depth, colour, alpha), 8 views per pass over a TSDF volume
              (lg_tsdf_integrate)
    extract   TSDFVolume.extract_mesh: marching tetrahedra with indexed vertices (lg_mesh_count, lg_mesh_emit), normals toward free space
    prune     count_render over the views -> significance score -> prune mask -> prune_points (66 % by default), then the same again:
              through the holes a prune tears the rays reach the far side of the shell, and the fused surface turns ragged: its area
              and its distance from the sphere rise

    python examples/mesh_extract.py [--n-gaussians 60000] [--views 24] [--grid 160] [--out mesh.ply]

The scene is a shell of flat Gaussians about the unit sphere, so the surface is known: the area is 4 pi = 12.57.  Printed per model: the
vertex and face counts, the surface area, and the mean distance of the vertices from the sphere in voxels.  The PLY files (binary
little-endian, with vertex colours) open in MeshLab or Blender."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import mesh  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.prune import prune_epilogue, prune_list_sharded, prune_points  # noqa: E402

from distortion_finetune import with_optimizer  # noqa: E402


def sphere_shell(n, seed=0):
    """n flat Gaussians on the unit sphere, their thin axis along the normal."""
    g = syn.make_gaussians(n, seed=seed, log_scale_mean=math.log(0.012), log_scale_std=0.2, opacity_mean=3.0)
    gen = torch.Generator().manual_seed(seed)
    p = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=1)
    g._xyz = p.clone()
    # the rotation that takes z to the normal p: axis z x p, angle acos(p.z)
    axis = torch.nn.functional.normalize(torch.stack([-p[:, 1], p[:, 0], torch.zeros(n)], dim=1) + 1e-12, dim=1)
    half = 0.5 * torch.acos(p[:, 2].clamp(-1, 1))
    g._rotation = torch.cat([torch.cos(half)[:, None], axis * torch.sin(half)[:, None]], dim=1)
    g._scaling[:, 2] = math.log(0.003)
    return g


def surface(vertices, faces):
    a, b, c = (vertices[faces[:, k].long()] for k in range(3))
    return float(torch.linalg.cross(b - a, c - a).norm(dim=1).sum() / 2)


def fuse_and_extract(model, cameras, pipe, origin, dims, voxel, path):
    vol = mesh.TSDFVolume(origin, dims, voxel, device=model.get_xyz.device)
    mesh.fuse_views(cameras, model, pipe, vol)
    v, f, c = vol.extract_mesh()
    off = float(((v.norm(dim=1) - 1).abs() / voxel).mean()) if len(v) else float("nan")
    print(f"  {model.num} Gaussians: {len(v)} vertices, {len(f)} faces, area {surface(v, f):.3f} (sphere: {4 * math.pi:.3f}), "
          f"vertices {off:.2f} voxel from the sphere on average, {100 * float((vol.weight > 0).float().mean()):.0f} % of the points observed")
    if path:
        mesh.save_ply(path, v, f, c)
        print(f"  wrote {path}")
    return surface(v, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=60_000)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--grid", type=int, default=160)
    ap.add_argument("--prune-percent", type=float, default=0.66)
    ap.add_argument("--v-pow", type=float, default=0.1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    model = with_optimizer(sphere_shell(args.n_gaussians).to(dev))
    cameras = [syn.orbit_camera(k, args.views, args.width, args.height, radius=4.0, height_y=(-1.5, 0.8, 2.5)[k % 3]).to(dev) for k in range(args.views)]
    voxel = 3.0 / (args.grid - 1)
    origin, dims = (-1.5, -1.5, -1.5), (args.grid,) * 3
    print(f"proposed by bounds_from_cameras at this voxel size: {mesh.bounds_from_cameras(cameras, voxel, scale=0.4)}; used: {origin}, {dims}")
    stem, ext = os.path.splitext(args.out)
    before = fuse_and_extract(model, cameras, pipe, origin, dims, voxel, args.out)
    with torch.no_grad():
        _counts, imp_list = prune_list_sharded(model, cameras, pipe, bg)
        _v, mask, _thr = prune_epilogue(model, imp_list, args.v_pow, args.prune_percent)
        prune_points(model, mask)
    after = fuse_and_extract(model, cameras, pipe, origin, dims, voxel, f"{stem}_pruned{ext}" if args.out else "")
    print(f"surface area {before:.3f} -> {after:.3f} after pruning {100.0 * float(mask.float().mean()):.0f} %")


if __name__ == "__main__":
    main()
