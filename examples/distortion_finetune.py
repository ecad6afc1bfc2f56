#!/usr/bin/env python3
"""Fine-tune a pruned model with a photometric loss plus the two geometry terms of 2DGS, on a synthetic scene:

    teacher images  render() of the unpruned model, one per view
    prune           count_render over the views -> significance score -> prune mask -> prune_points (66 % by default)
    fine-tune       per step ONE render_geometry(cam, model, pipe, distortion=True): colour, blended normals, expected depth, alpha, the
                    depth distortion map sum_{i<j} w_i w_j (z_i - z_j)^2 and the median depth from one forward; the loss is
                    L1(colour) + lambda_normal * normals.normal_consistency_loss(normal, depth, alpha, cam) + lambda_dist * distortion.mean()
                    -- the distortion term pulls the weights along a ray together: what a prune loosens first is thin structure and
                    floaters -- and ONE backward (lg_backward_distortion) moves _xyz, _opacity, _scaling, _rotation and the colours;
                    the step is lightgaussian_amd.optim.HipAdam

    python examples/distortion_finetune.py [--n-gaussians 100000] [--steps 48] [--lambda-dist 0.05] [--lambda-normal 0.05]

Printed before and after the fine-tune, as means over the views: the distortion term, the consistency term, and the mean absolute
difference between the median and the expected depth over the pixels the model covers (alpha > 0.5): a ray whose weights sit together has
both depths at the same place.  For unbounded scenes blend distortion.ndc_depth(z, near, far) as a further feature column and name it as
m_column of distortion.blend_geometry (2DGS measures the term in NDC depth there)."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render, render_geometry  # noqa: E402
from lightgaussian_amd.normals import normal_consistency_loss  # noqa: E402
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


def geometry_terms(model, cameras, pipe, bg):
    """(mean distortion term, mean consistency term, mean |median depth - expected depth| where alpha > 0.5) over the views."""
    dist = term = spread = 0.0
    with torch.no_grad():
        for cam in cameras:
            pkg = render_geometry(cam, model, pipe, bg, geometry_grad=False, distortion=True)
            dist += float(pkg["distortion"].mean())
            term += float(normal_consistency_loss(pkg["normal"], pkg["depth"], pkg["alpha"], cam))
            seen = pkg["alpha"] > 0.5
            gap = (pkg["median_depth"] - pkg["depth"]).abs()[seen]
            spread += float(gap.mean()) if gap.numel() else 0.0
    return dist / len(cameras), term / len(cameras), spread / len(cameras)


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
    ap.add_argument("--lambda-dist", type=float, default=0.05)
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
    dist, term, spread = geometry_terms(model, cameras, pipe, bg)
    print(f"before: distortion term {dist:.6f}   normal-consistency term {term:.5f}   mean |median - expected depth| {spread:.4f}")
    terms = torch.zeros(3, device=dev)
    for it in range(args.steps):
        k = it % args.views
        pkg = render_geometry(cameras[k], model, pipe, bg, distortion=True)
        l_color = (pkg["render"] - teacher[k]).abs().mean()
        l_normal = normal_consistency_loss(pkg["normal"], pkg["depth"], pkg["alpha"], cameras[k])
        l_dist = pkg["distortion"].mean()
        (l_color + args.lambda_normal * l_normal + args.lambda_dist * l_dist).backward()
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        terms += torch.stack([l_color.detach(), l_normal.detach(), l_dist.detach()])
        if k == args.views - 1 or it == args.steps - 1:
            n = k + 1
            c, nn, dd = (terms / n).tolist()
            print(f"steps {it + 1 - n:4d}..{it:4d}: colour L1 {c:.5f}   normal consistency {nn:.5f}   distortion {dd:.6f}")
            terms.zero_()
    dist2, term2, spread2 = geometry_terms(model, cameras, pipe, bg)
    print(f"after:  distortion term {dist2:.6f}   normal-consistency term {term2:.5f}   mean |median - expected depth| {spread2:.4f}")
    assert math.isfinite(dist2) and math.isfinite(term2)


if __name__ == "__main__":
    main()
