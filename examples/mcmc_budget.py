#!/usr/bin/env python3
"""Training to a Gaussian budget with 3DGS-MCMC (lightgaussian_amd.mcmc), beside the adaptive clone / split of densify_and_prune.

    python examples/mcmc_budget.py [--start 3000] [--cap 12000] [--iterations 600] [--every 15] [--width 160] [--height 120]

A synthetic scene -- target images rendered from a fixed set of Gaussians over an orbit of cameras -- is fitted twice from the same
few thousand starting Gaussians, on the same schedule:
    mcmc      loss + mcmc.regularizers, HipAdam.step, mcmc.after_step: dead Gaussians relocated, the model grown 5 % at a time up to the
              cap, position noise every iteration.  The final count is the cap.
    densify   loss, HipAdam.step, densify.accumulate_stats and, on the same iterations, densify.densify_and_prune: the final count is
              whatever the thresholds leave.
N and the PSNR over the training views are printed as the runs go; nothing is asserted about either."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import densify, mcmc, optim  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render  # noqa: E402

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)
DEGREE = 1


class Model:
    """The attribute surface mcmc and densify touch: the reference GaussianModel's."""

    def __init__(self, g, dev):
        for n in NAMES:
            setattr(self, ATTRS[n], torch.nn.Parameter(getattr(g, ATTRS[n]).to(dev).clone()))
        self.optimizer = optim.HipAdam([{"params": [getattr(self, ATTRS[n])], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=1e-15)
        self.percent_dense = 0.01
        self.reset_stats()

    def reset_stats(self):
        n, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum, self.denom = torch.zeros(n, 1, device=dev), torch.zeros(n, 1, device=dev)
        self.max_radii2D = torch.zeros(n, device=dev)

    def view(self):
        return syn.SyntheticGaussians(self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity, DEGREE, DEGREE)


def psnr(model, cams, targets, bg):
    with torch.no_grad():
        mse = sum(float(((render(c, model.view(), syn.PipelineParams(), bg)["render"] - t) ** 2).mean()) for c, t in zip(cams, targets)) / len(cams)
    return -10.0 * math.log10(max(mse, 1e-12))


def fit(method, start, args, cams, targets, bg, dev):
    model = Model(start, dev)
    torch.manual_seed(0)
    for it in range(1, args.iterations + 1):
        k = it % len(cams)
        pkg = render(cams[k], model.view(), syn.PipelineParams(), bg)
        loss = (pkg["render"] - targets[k]).abs().mean()
        if method == "mcmc":
            loss = loss + mcmc.regularizers(model)
        model.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if method == "densify":
            densify.accumulate_stats(model, pkg["viewspace_points"], pkg["visibility_filter"], radii=pkg["radii"])
        model.optimizer.step()
        if method == "mcmc":
            mcmc.after_step(model, it, LRS["xyz"], args.cap, start=args.every - 1, stop=args.iterations, every=args.every)
        elif args.every - 1 < it < args.iterations and it % args.every == 0:
            densify.densify_and_prune(model, 0.0002, 0.005, 4.0, None)
        if it % (2 * args.every) == 0 or it == args.iterations:
            print(f"  {method:8s} iteration {it:5d}: N = {model._xyz.shape[0]:6d}, PSNR {psnr(model, cams, targets, bg):5.2f} dB")
    return model._xyz.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--start", type=int, default=3000)
    ap.add_argument("--cap", type=int, default=12000)
    ap.add_argument("--truth", type=int, default=20000, help="Gaussians of the scene the targets are rendered from")
    ap.add_argument("--iterations", type=int, default=600)
    ap.add_argument("--every", type=int, default=15)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--height", type=int, default=120)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    bg = torch.zeros(3, device=dev)
    cams = [syn.orbit_camera(k, args.views, W, H).to(dev) for k in range(args.views)]
    truth = syn.make_gaussians(args.truth, sh_degree=DEGREE, seed=3, extent=(2.0, 1.2, 2.0), log_scale_mean=math.log(0.03), opacity_mean=1.0).to(dev)
    with torch.no_grad():
        targets = [render(c, truth, syn.PipelineParams(), bg)["render"].clone() for c in cams]
    start = syn.make_gaussians(args.start, sh_degree=DEGREE, seed=4, extent=(2.0, 1.2, 2.0), log_scale_mean=math.log(0.06), opacity_mean=-1.0)
    print(f"{args.truth} Gaussians in the scene, {args.views} views of {W} x {H}; from {args.start} Gaussians, {args.iterations} iterations, "
          f"growth every {args.every}; budget {args.cap}")
    final = {method: fit(method, start, args, cams, targets, bg, dev) for method in ("mcmc", "densify")}
    print(f"final N: mcmc {final['mcmc']} (the budget: {args.cap}), densify_and_prune {final['densify']}")


if __name__ == "__main__":
    main()
