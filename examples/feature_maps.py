#!/usr/bin/env python3
"""Accumulated-opacity and expected-depth maps of a model before and after LightGaussian's prune, on a synthetic scene:

    count_render over the views  ->  significance score  ->  prune mask  ->  prune_points
    render_features(cam, model, pipe, "depth") before and after: alpha [H, W] and depth [1, H, W] of the same views

    python examples/feature_maps.py [--n-gaussians 300000] [--prune-percent 0.66]

render_features runs ONE ordinary forward per view and blends the extra channel over the tile lists that forward left
(lg_blend_features) -- no second K1 / binning chain, as a render(..., override_color=...) per three channels would need.
Printed per view: the share of pixels whose alpha dropped by more than --hole (holes the prune opened), and the mean absolute
change of the expected depth over the pixels both models cover."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render_features  # noqa: E402
from lightgaussian_amd.prune import prune_epilogue, prune_list_sharded, prune_points  # noqa: E402


def with_optimizer(model):
    """What GaussianModel.training_setup leaves: one named Adam group per parameter and the densification bookkeeping."""
    n, dev = model.num, model.get_xyz.device
    names = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
    for attr in names.values():
        setattr(model, attr, torch.nn.Parameter(getattr(model, attr)))
    model.optimizer = torch.optim.Adam([{"params": [getattr(model, a)], "lr": 1e-3, "name": k} for k, a in names.items()], lr=0.0, eps=1e-15)
    model.xyz_gradient_accum = torch.zeros(n, 1, device=dev)
    model.denom = torch.zeros(n, 1, device=dev)
    model.max_radii2D = torch.zeros(n, device=dev)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=300_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--prune-percent", type=float, default=0.66)
    ap.add_argument("--v-pow", type=float, default=0.1)
    ap.add_argument("--hole", type=float, default=0.1, help="an alpha drop beyond this counts as a hole")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    model = with_optimizer(syn.make_gaussians(args.n_gaussians, log_scale_mean=-4.0).to(dev))
    cameras = [syn.orbit_camera(k, args.views, args.width, args.height).to(dev) for k in range(args.views)]
    with torch.no_grad():
        before = [render_features(cam, model, pipe, "depth") for cam in cameras]
        _counts, imp_list = prune_list_sharded(model, cameras, pipe, torch.zeros(3, device=dev))
        _v, mask, _thr = prune_epilogue(model, imp_list, args.v_pow, args.prune_percent)
        prune_points(model, mask)
        after = [render_features(cam, model, pipe, "depth") for cam in cameras]
    print(f"{args.n_gaussians} Gaussians -> {model.num} after pruning {100.0 * mask.float().mean():.1f} %")
    for k, (b, a) in enumerate(zip(before, after)):
        dropped = (b["alpha"] - a["alpha"]) > args.hole
        both = (b["alpha"] > 0.5) & (a["alpha"] > 0.5)
        ddepth = (b["depth"][0] - a["depth"][0]).abs()[both].mean().item() if bool(both.any()) else float("nan")
        print(f"view {k}: covered (alpha > 0.5) {100.0 * (b['alpha'] > 0.5).float().mean():5.1f} % -> {100.0 * (a['alpha'] > 0.5).float().mean():5.1f} %, "
              f"alpha dropped by > {args.hole} on {100.0 * dropped.float().mean():.2f} % of the pixels, mean |depth change| {ddepth:.4f}")


if __name__ == "__main__":
    main()
