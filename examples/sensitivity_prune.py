#!/usr/bin/env python3
"""Two pruning criteria on one synthetic model, pruned to the same percentage:

    significance (LightGaussian):  score_j = sum over views and hits of alpha_j T_j, times the volume factor
    sensitivity  (PUP 3D-GS):      score_j = log det of Gaussian j's 6 x 6 block, over (mean, log-scale), of the Gauss-Newton Hessian of the
                                   L2 reconstruction error summed over the views (lightgaussian_amd.sensitivity)

A blending-weight sum rewards what is seen often; the sensitivity asks how much the images move when the Gaussian moves or changes size,
and ranks a Gaussian that fewer than two views constrain (-inf) first.  Printed: how many Gaussians each rule keeps and the PSNR of the
pruned models' renders against the unpruned ones.

    python examples/sensitivity_prune.py [--n-gaussians 200000 --views 24 --width 640 --height 360 --prune-percent 0.8]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import sensitivity  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402
from lightgaussian_amd.prune import calculate_v_imp_score, prune_list, prune_mask  # noqa: E402


def subset(g, keep):
    """The rows of a SyntheticGaussians that `keep` selects (a model without an optimizer: prune.prune_gaussians does this to a GaussianModel)."""
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
    ap.add_argument("--prune-percent", type=float, default=0.8)
    ap.add_argument("--v-pow", type=float, default=0.1)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = syn.make_gaussians(args.n_gaussians, log_scale_mean=math.log(0.02)).to(dev)
    cams = [syn.orbit_camera(k, args.views, args.width, args.height).to(dev) for k in range(args.views)]
    bg, pipe = torch.zeros(3, device=dev), syn.PipelineParams()
    with torch.no_grad():
        _, s_sum = prune_list(g, cams, pipe, bg)
        H = sensitivity.sensitivity_list(g, cams, pipe, bg)
        s_sens = sensitivity.score(H, g, scale_space="log")
        rules = {"significance": prune_mask(args.prune_percent, calculate_v_imp_score(g, s_sum, args.v_pow)),
                 "sensitivity": prune_mask(args.prune_percent, s_sens)}
        full = [render(c, g, pipe, bg, options={"fast_exp": False})["render"] for c in cams]
        finite = torch.isfinite(s_sens)
        print(f"{args.n_gaussians} Gaussians, {args.views} views of {args.width} x {args.height}, pruning {100 * args.prune_percent:.0f} %; "
              f"sensitivity: {int((~finite).sum())} Gaussians score -inf, the others {float(s_sens[finite].min()):.1f} .. {float(s_sens[finite].max()):.1f}")
        for name, mask in rules.items():
            kept = subset(g, ~mask)
            quality = [psnr(render(c, kept, pipe, bg, options={"fast_exp": False})["render"], ref) for c, ref in zip(cams, full)]
            print(f"{name:>14}: keeps {int((~mask).sum()):8d} of {args.n_gaussians}, PSNR against the unpruned renders "
                  f"{sum(quality) / len(quality):.2f} dB (worst view {min(quality):.2f})")


if __name__ == "__main__":
    main()
