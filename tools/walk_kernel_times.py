#!/usr/bin/env python3
"""Per-kernel times of the list walks of lg_features.h and lg_distortion.h (LG_FLAG_PROFILE: device events around each launch), for A/B
runs of two builds of the library:

    LIGHTGAUSSIAN_HIP_LIB=variants/lib_a.so python tools/walk_kernel_times.py a1        (then b1, a2, b2, ... alternately)

bench.py's frozen scene (make_gaussians(N, log_scale_mean = log 0.004), orbit camera 0 of 200).  Per channel count C of --channels:
render_features(geometry_grad=True) forward + backward to every raw parameter and to the features (features_fwd, features_bwd_geom,
features_bwd, features_gather, beside K1 / K6 / K7 / K9 of the same calls); then render_geometry(distortion=True) forward + backward
(distortion_fwd, distortion_bwd, distortion_gather).  Two unprofiled calls, then the mean over --reps profiled calls, ms per launch.
Prints one line `KERNEL_TIMES {json}` carrying the label and the library's build id.  tools/features_bench.py times whole legs and
tools/distortion_bench.py profiles one call of one leg; this is the per-kernel view of both, cheap enough to alternate many times."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, normals  # noqa: E402
from lightgaussian_amd import synthetic as syn  # noqa: E402
from lightgaussian_amd.gaussian_renderer import render_features, render_geometry  # noqa: E402

RAW = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")
SCOPES = ("features_", "distortion_", "blend_", "preprocess")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("label")
    ap.add_argument("--n-gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("walk_kernel_times.py measures on a GPU; there is none")
    dev = torch.device("cuda", 0)
    N, W, H = args.n_gaussians, args.width, args.height
    model = syn.make_gaussians(N, log_scale_mean=math.log(0.004)).to(dev)
    cam = syn.orbit_camera(0, 200, W, H).to(dev)
    pipe = syn.PipelineParams()
    for n in RAW:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    params = [getattr(model, n) for n in RAW]
    gen = torch.Generator(device=dev).manual_seed(1)
    out = {"label": args.label, "build": _lib.build_id(), "N": N, "reps": args.reps}

    def profiled(fn):
        for _ in range(2):
            fn(None)
        torch.cuda.synchronize()
        _lib.profile_reset()
        for _ in range(args.reps):
            fn({"profile": True})
        torch.cuda.synchronize()
        return {k: round(ms / n, 4) for k, (ms, n) in _lib.profile_read().items() if k.startswith(SCOPES)}

    for Cn in args.channels:
        F = torch.randn(N, Cn, device=dev, generator=gen).requires_grad_(True)
        G = torch.randn(Cn, H, W, device=dev, generator=gen)

        def geom(options):
            p = render_features(cam, model, pipe, F, geometry_grad=True, options=options)
            torch.autograd.grad((p["features"] * G).sum() + p["render"].mean(), params + [F], allow_unused=True)

        out[f"features C={Cn}"] = profiled(geom)
        del F, G

    def dist(options):
        p = render_geometry(cam, model, pipe, distortion=True, options=options)
        loss = normals.normal_consistency_loss(p["normal"], p["depth"], p["alpha"], cam) + p["distortion"].mean() + p["render"].mean()
        torch.autograd.grad(loss, params, allow_unused=True)

    out["render_geometry(distortion)"] = profiled(dist)
    print("KERNEL_TIMES " + json.dumps(out))


if __name__ == "__main__":
    main()
