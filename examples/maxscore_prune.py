#!/usr/bin/env python3
"""Two pruning criteria on one synthetic model, side by side:

    sum + percentile (LightGaussian):  score_j = sum over views and hits of alpha_j T_j, times the volume factor; the lowest
                                       --prune-percent of the scores go
    max + threshold  (RadSplat):       score_j = max over views and pixels of alpha_j T_j, the largest share Gaussian j ever has of a
                                       pixel; everything below --threshold goes (0.01; 0.25 for the light models)

A sum rewards splats that are big and seen often; a maximum keeps a small splat that dominates one pixel of one view and removes a
large one that is everywhere and never matters.  Both passes run the same significance-only kernels (prune_list_sharded, weight policy
"alpha_t"); the second one with score_reduce="max".  Printed: how many Gaussians each rule keeps and the PSNR of the pruned models'
renders against the unpruned ones.

    python examples/maxscore_prune.py [--n-gaussians 200000 --views 24 --width 640 --height 360]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402
from lightgaussian_amd.prune import calculate_v_imp_score, prune_list_sharded, prune_mask, prune_mask_threshold  # noqa: E402


def subset(g, keep):
    """The rows of a SyntheticGaussians that `keep` selects (a model without an optimizer: prune.prune_below does this to a GaussianModel)."""
    return syn.SyntheticGaussians(g._xyz[keep], g._features_dc[keep], g._features_rest[keep], g._scaling[keep], g._rotation[keep],
                                  g._opacity[keep], active_sh_degree=g.active_sh_degree, max_sh_degree=g.max_sh_degree)


def psnr(a, b):
    return -10.0 * math.log10(max(float(((a - b) ** 2).mean()), 1e-12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=200_000)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--prune-percent", type=float, default=0.66)
    ap.add_argument("--v-pow", type=float, default=0.1)
    ap.add_argument("--threshold", type=float, default=0.01)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = syn.make_gaussians(args.n_gaussians, log_scale_mean=math.log(0.02)).to(dev)
    cams = [syn.orbit_camera(k, args.views, args.width, args.height).to(dev) for k in range(args.views)]
    bg, pipe = torch.zeros(3, device=dev), syn.PipelineParams()
    with torch.no_grad():
        _, s_sum = prune_list_sharded(g, cams, pipe, bg, weight_policy="alpha_t")
        _, s_max = prune_list_sharded(g, cams, pipe, bg, weight_policy="alpha_t", score_reduce="max")
        rules = {f"sum, lowest {100 * args.prune_percent:.0f} %": prune_mask(args.prune_percent, calculate_v_imp_score(g, s_sum, args.v_pow)),
                 f"max, below {args.threshold}": prune_mask_threshold(s_max, args.threshold)}
        full = [render(c, g, pipe, bg, options={"fast_exp": False})["render"] for c in cams]
        print(f"{args.n_gaussians} Gaussians, {args.views} views of {args.width} x {args.height}; largest share of a pixel: "
              f"median {float(s_max.median()):.4f}, never hit {int((s_max == 0).sum())}")
        for name, mask in rules.items():
            kept = subset(g, ~mask)
            quality = [psnr(render(c, kept, pipe, bg, options={"fast_exp": False})["render"], ref) for c, ref in zip(cams, full)]
            print(f"{name:>22}: keeps {int((~mask).sum()):8d} of {args.n_gaussians}, PSNR against the unpruned renders "
                  f"{sum(quality) / len(quality):.2f} dB (worst view {min(quality):.2f})")


if __name__ == "__main__":
    main()
