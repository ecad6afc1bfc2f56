#!/usr/bin/env python3
"""Fine-tune a pruned model against the unpruned model's colour, expected depth and accumulated opacity, on a synthetic scene:

    teacher maps  render_features(cam, model, pipe, "depth") of the unpruned model: render, depth, alpha per view
    prune         count_render over the views -> significance score -> prune mask -> prune_points (66 % by default)
    fine-tune     per step ONE render_features(cam, model, pipe, "depth", geometry_grad=True): the colour image, the depth map and the
                  alpha map of one forward enter one loss, and one backward (lg_backward_features: K7 for the colour term, one more
                  walk of the tile lists for depth and alpha, K9 once) moves _xyz, _opacity, _scaling, _rotation and the colours;
                  the step is lightgaussian_amd.optim.HipAdam (one fused launch)

    python examples/depth_finetune.py [--n-gaussians 100000] [--steps 48]

Printed per pass over the views: the mean of the three loss terms.  A depth or an opacity loss cannot be expressed through render():
it has neither map, and the holes a prune opens (examples/feature_maps.py) are exactly what those two terms see."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render_features  # noqa: E402
from lightgaussian_amd.optim import HipAdam  # noqa: E402
from lightgaussian_amd.prune import prune_epilogue, prune_list_sharded, prune_points  # noqa: E402

PARAMS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
LR = dict(xyz=2e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=2e-2, scaling=5e-3, rotation=1e-3)


def with_optimizer(model):
    """What GaussianModel.training_setup leaves: one named Adam group per parameter and the densification bookkeeping (prune_points
    edits both)."""
    n, dev = model.num, model.get_xyz.device
    for attr in PARAMS.values():
        setattr(model, attr, torch.nn.Parameter(getattr(model, attr)))
    model.optimizer = torch.optim.Adam([{"params": [getattr(model, a)], "lr": LR[k], "name": k} for k, a in PARAMS.items()], lr=0.0, eps=1e-15)
    model.xyz_gradient_accum = torch.zeros(n, 1, device=dev)
    model.denom = torch.zeros(n, 1, device=dev)
    model.max_radii2D = torch.zeros(n, device=dev)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--prune-percent", type=float, default=0.66)
    ap.add_argument("--v-pow", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--w-depth", type=float, default=0.1)
    ap.add_argument("--w-alpha", type=float, default=0.5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    model = with_optimizer(syn.make_gaussians(args.n_gaussians, log_scale_mean=-4.0).to(dev))
    cameras = [syn.orbit_camera(k, args.views, args.width, args.height).to(dev) for k in range(args.views)]
    with torch.no_grad():
        teacher = [render_features(cam, model, pipe, "depth", bg_color=bg) for cam in cameras]
        _counts, imp_list = prune_list_sharded(model, cameras, pipe, bg)
        _v, mask, _thr = prune_epilogue(model, imp_list, args.v_pow, args.prune_percent)
        prune_points(model, mask)
    print(f"{args.n_gaussians} Gaussians -> {model.num} after pruning {100.0 * mask.float().mean():.1f} %")
    for attr in PARAMS.values():
        setattr(model, attr, torch.nn.Parameter(getattr(model, attr).detach().clone()))
    optimizer = HipAdam([{"params": [getattr(model, a)], "lr": LR[k], "name": k} for k, a in PARAMS.items()], lr=0.0, eps=1e-15)
    terms = torch.zeros(3, device=dev)
    for it in range(args.steps):
        k = it % args.views
        t = teacher[k]
        pkg = render_features(cameras[k], model, pipe, "depth", geometry_grad=True, bg_color=bg)
        seen = (t["alpha"] > 0.5).float()                   # depth is supervised where the teacher sees a surface
        l_color = (pkg["render"] - t["render"]).abs().mean()
        l_depth = ((pkg["depth"][0] - t["depth"][0]).abs() * seen).sum() / seen.sum().clamp_min(1.0)
        l_alpha = (pkg["alpha"] - t["alpha"]).abs().mean()
        (l_color + args.w_depth * l_depth + args.w_alpha * l_alpha).backward()
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        terms += torch.stack([l_color.detach(), l_depth.detach(), l_alpha.detach()])
        if k == args.views - 1 or it == args.steps - 1:
            n = k + 1
            c, d, a = (terms / n).tolist()
            print(f"steps {it + 1 - n:4d}..{it:4d}: colour L1 {c:.5f}   depth L1 {d:.5f}   alpha L1 {a:.5f}")
            terms.zero_()


if __name__ == "__main__":
    main()
