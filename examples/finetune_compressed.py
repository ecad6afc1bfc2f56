#!/usr/bin/env python3
"""Fine-tune a VecTree-compressed model in its compressed form and write it back as an extreme_saving directory.

    python examples/finetune_compressed.py [--load DIR] [--save DIR] [--steps 200] [--codebook 256] [--n 50000] [--hip-adam]

Without --load a synthetic scene is quantised here (vectree.quantize_model); the training targets are renders of the
unquantised scene.  With --load the directory is read (vectree.CompressedGaussians.load) and the targets are renders of the
model as loaded, seen from the same orbit: a stand-in for the training views of a real scene.  Adam runs on the float32 master
of the row table only -- the codebook rows are shared by their Gaussians, the gradient reaches them through lg_vq_colors_bwd
as a fixed-order segmented sum -- and the forward always sees the float16 values, so the saved file renders exactly as trained."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn, vectree  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--load", help="extreme_saving directory to fine-tune (default: quantise a synthetic scene)")
ap.add_argument("--save", help="directory to write the fine-tuned model to")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--lr", type=float, default=2e-3)
ap.add_argument("--n", type=int, default=50000, help="Gaussians of the synthetic scene")
ap.add_argument("--codebook", type=int, default=256)
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--hip-adam", action="store_true", help="step with lightgaussian_amd.optim.HipAdam (one lg_adam_step launch) instead of torch.optim.Adam")
args = ap.parse_args()

dev = torch.device("cuda:0")
pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
cams = [syn.orbit_camera(k, args.views, 640, 360).to(dev) for k in range(args.views)]
if args.load:
    cg = vectree.CompressedGaussians.load(args.load, dev)
    teacher = cg
else:
    g = syn.make_gaussians(args.n, sh_degree=3, log_scale_mean=math.log(0.02)).to(dev)
    feats = torch.cat([g._xyz, torch.zeros_like(g._xyz), g._features_dc.transpose(1, 2).reshape(g.num, 3),
                       g._features_rest.transpose(1, 2).reshape(g.num, -1), g._opacity, g._scaling, g._rotation], dim=1).contiguous()
    importance = torch.rand(g.num, device=dev)
    cg = vectree.CompressedGaussians.from_packed(
        vectree.quantize_model(feats, importance, vq_ratio=0.6, codebook_size=args.codebook, iterations=50, chunk=20000), dev)
    teacher = g
with torch.no_grad():
    targets = [render(cam, teacher, pipe, bg)["render"].clone() for cam in cams]

tc = cg.trainable(("rows",))
if args.hip_adam:
    from lightgaussian_amd import optim
    opt = optim.HipAdam(tc.parameters(), lr=args.lr)
else:
    opt = torch.optim.Adam(tc.parameters(), lr=args.lr)


def mean_l1():
    with torch.no_grad():
        return sum((render(c, tc, pipe, bg)["render"] - t).abs().mean().item() for c, t in zip(cams, targets)) / len(cams)


print(f"{tc.num} Gaussians, {tc.codebook_size} codes + {tc._rows.shape[0] - tc.codebook_size} rows of their own; mean L1 before: {mean_l1():.6f}")
for step in range(args.steps):
    cam, target = cams[step % len(cams)], targets[step % len(cams)]
    opt.zero_grad(set_to_none=True)
    (render(cam, tc, pipe, bg)["render"] - target).abs().mean().backward()
    opt.step()
    tc.sync_rows()                       # the forward reads the float16 table: refresh it from the master
print(f"mean L1 after {args.steps} steps of {type(opt).__name__}: {mean_l1():.6f}")
if args.save:
    vectree.save(args.save, tc.repack())
    print(f"wrote {args.save}: {sum(os.path.getsize(os.path.join(args.save, f)) for f in os.listdir(args.save)) / 1e6:.2f} MB")
