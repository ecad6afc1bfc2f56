#!/usr/bin/env python3
"""Fine-tune a pruned model with a photometric loss plus the depth-normal consistency term, on a synthetic scene:

    teacher images  render() of the unpruned model, one per view
    prune           count_render over the views -> significance score -> prune mask -> prune_points (66 % by default)
    fine-tune       per step ONE render_geometry(cam, model, pipe): colour, blended normals, expected depth and alpha from one forward;
                    the loss is L1(colour) + lambda * normals.normal_consistency_loss(normal, depth, alpha, cam) -- the normals of the
                    Gaussians against the normals of the depth surface they render, no ground-truth depth needed -- and one backward
                    moves _xyz, _opacity, _scaling, _rotation and the colours; the step is lightgaussian_amd.optim.HipAdam

    python examples/normal_consistency.py [--n-gaussians 100000] [--steps 48] [--lambda-normal 0.05]

Printed before and after the fine-tune, as means over the views: the consistency term and the angle between the rendered normal and
depth_to_normal(depth) over the pixels the model covers (alpha > 0.5)."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render, render_geometry  # noqa: E402
from lightgaussian_amd.normals import depth_to_normal, normal_consistency_loss  # noqa: E402
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


def consistency(model, cameras, pipe, bg):
    """(mean consistency term, mean angle in degrees between normal and depth_to_normal(depth) where alpha > 0.5) over the views."""
    term = angle = 0.0
    with torch.no_grad():
        for cam in cameras:
            pkg = render_geometry(cam, model, pipe, bg, geometry_grad=False)
            term += float(normal_consistency_loss(pkg["normal"], pkg["depth"], pkg["alpha"], cam))
            n_d = depth_to_normal(pkg["depth"], cam)
            n_r = torch.nn.functional.normalize(pkg["normal"], dim=0)
            seen = (pkg["alpha"] > 0.5) & (n_d.abs().sum(dim=0) > 0)
            cos = (n_r * n_d).sum(dim=0).clamp(-1.0, 1.0)[seen]
            angle += float(torch.rad2deg(torch.acos(cos)).mean()) if cos.numel() else 0.0
    return term / len(cameras), angle / len(cameras)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gaussians", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--prune-percent", type=float, default=0.66)
    ap.add_argument("--v-pow", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--lambda-normal", type=float, default=0.05)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    model = with_optimizer(syn.make_gaussians(args.n_gaussians, log_scale_mean=-4.0).to(dev))
    cameras = [syn.orbit_camera(k, args.views, args.width, args.height).to(dev) for k in range(args.views)]
    with torch.no_grad():
        teacher = [render(cam, model, pipe, bg)["render"] for cam in cameras]
        _counts, imp_list = prune_list_sharded(model, cameras, pipe, bg)
        _v, mask, _thr = prune_epilogue(model, imp_list, args.v_pow, args.prune_percent)
        prune_points(model, mask)
    print(f"{args.n_gaussians} Gaussians -> {model.num} after pruning {100.0 * mask.float().mean():.1f} %")
    for attr in PARAMS.values():
        setattr(model, attr, torch.nn.Parameter(getattr(model, attr).detach().clone()))
    optimizer = HipAdam([{"params": [getattr(model, a)], "lr": LR[k], "name": k} for k, a in PARAMS.items()], lr=0.0, eps=1e-15)
    term, angle = consistency(model, cameras, pipe, bg)
    print(f"before: normal-consistency term {term:.5f}   mean angle {angle:.2f} deg")
    terms = torch.zeros(2, device=dev)
    for it in range(args.steps):
        k = it % args.views
        pkg = render_geometry(cameras[k], model, pipe, bg)
        l_color = (pkg["render"] - teacher[k]).abs().mean()
        l_normal = normal_consistency_loss(pkg["normal"], pkg["depth"], pkg["alpha"], cameras[k])
        (l_color + args.lambda_normal * l_normal).backward()
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        terms += torch.stack([l_color.detach(), l_normal.detach()])
        if k == args.views - 1 or it == args.steps - 1:
            n = k + 1
            c, nn = (terms / n).tolist()
            print(f"steps {it + 1 - n:4d}..{it:4d}: colour L1 {c:.5f}   normal consistency {nn:.5f}")
            terms.zero_()
    term2, angle2 = consistency(model, cameras, pipe, bg)
    print(f"after:  normal-consistency term {term2:.5f}   mean angle {angle2:.2f} deg")
    assert math.isfinite(term2)


if __name__ == "__main__":
    main()
