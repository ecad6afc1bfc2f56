#!/usr/bin/env python3
"""Nearest-code search at the reference's shapes (vectree/vectree.py: 8192-entry codebook, 27 / 48 feature dimensions, 8192-row
chunks over all Gaussians): lg_vq_nearest (f32 MFMA, fused argmin) next to the reference's torch formulation
(-torch.cdist(x, embed).argmax(-1), vectree/vq.py:265-266) on the same GPU.  Also times the compaction after a prune
(prune.compact_tensors vs 21 boolean-index kernels).

--leg train: one TRAINING iteration of the codebook at the reference's shapes (vectree.py:196-204: n = 80 000 sampled rows,
K = 8192, d = 27 / 48), device-resident inputs, warm, alternating blocks of
  (a) the parent path: the reference's formulation with only the search fused -- nearest_code, then one_hot (n x K), the two
      reductions against it and the two EMAs in torch, written here from the formulas in lightgaussian_amd/vq.py ema_update;
  (b) vq.ema_update (lg_vq_ema_step).
Prints ms / iteration of both and their ratio, and checks (b)'s post-state against (a)'s: indices equal, both compared with a
float64 evaluation from those indices under the parity rule of tests/test_gpu_vq_train.py (4 x (a)'s own deviation, floor
2^-22).  --fused-only skips (a): the form to run under `rocprofv3 --kernel-trace --stats` for the per-kernel split of (b).

--leg render (not part of "all"): a VecTree-compressed model (vq_ratio 0.6, K = 8192, SH degree 2 and 3, N = 1 M and 3 M, the
synthetic scene and its orbit cameras at 1080p) rendered forward-only, per view and warm, in alternating repeats of
  (a) render() of cg.to_dense() under no_grad -- the dequantised float32 model, the only way to show it without lg_vq_colors;
  (b) render_compressed(cg): lg_vq_colors + the forward on colors_precomp.
Prints the median and the min..max over the repeats of both, lg_vq_colors alone under an event bracket with
GB/s by its byte model, 12 + 4 + 6 (D + 1)^2 read and 12 written per Gaussian, and cg.nbytes() against the dense model's bytes.

--leg finetune (not part of "all"): forward + backward of an L1 loss per view on the same models and cameras, warm, in
alternating repeats of
  (a) render(cg.to_dense()) with the getters fused;
  (b) the same with fuse_getters off -- the like-for-like comparand: the compressed path feeds the unfused forward;
  (c) render(cg.trainable(all five tensors)): the compressed model trained in place, lg_vq_colors_bwd in the backward.
Every tensor of either model takes gradients (SH rows, xyz, opacity, scaling, rotation).
Prints median (min..max) of the three, and the peak allocated memory of one step of (a) and (c), gradient buffers included.
--only-compressed runs (c) alone: the form to run under `rocprofv3 --kernel-trace --stats` for the new kernels' own times."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import vq, prune

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("all", "search", "compact", "train", "render", "finetune"), default="all")
ap.add_argument("--iters", type=int, default=200, help="training iterations per timing (train leg)")
ap.add_argument("--fused-only", action="store_true")
ap.add_argument("--only-compressed", action="store_true", help="finetune leg: leg (c) alone")
ap.add_argument("--degrees", type=int, nargs="+", default=[2, 3], help="SH degrees (finetune leg)")
ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 3_000_000], help="Gaussians (render leg)")
ap.add_argument("--repeats", type=int, default=7, help="timed repeats over all views (render leg, at least 5)")
ap.add_argument("--views", type=int, default=8, help="orbit cameras (render leg)")
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


for d in (27, 48) if args.leg in ("all", "search") else ():
    n, K = 1_200_000, 8192
    g = torch.Generator().manual_seed(d)
    embed = (torch.randn(K, d, generator=g) * 0.3).to(dev)
    x = (embed[torch.randint(0, K, (n,), generator=g).to(dev)] + 0.1 * torch.randn(n, d, generator=g).to(dev))
    ms_hip, ind = timed(lambda: vq.nearest_code(x, embed))

    def ref():
        out = []
        for i in range(0, n, 8192):                     # the reference's chunking (vectree.py:93-96)
            out.append((-torch.cdist(x[i:i + 8192].unsqueeze(0), embed.unsqueeze(0), p=2)).argmax(-1)[0])
        return torch.cat(out)
    ms_ref, ind_ref = timed(ref, reps=2)
    agree = float((ind == ind_ref).float().mean())
    flops = 2.0 * n * K * (d + 1)
    print(f"vq d={d}: n={n} K={K}  lg_vq_nearest {ms_hip:.2f} ms ({flops / ms_hip / 1e9:.1f} TFLOP/s f32)  torch cdist+argmax {ms_ref:.2f} ms  "
          f"index agreement {agree:.6f}")

def compact_leg():
    N = 3_000_000
    g = torch.Generator().manual_seed(1)
    shapes = [(N, 3), (N, 1, 3), (N, 15, 3), (N, 1), (N, 3), (N, 4)]
    ts = []
    for s in shapes:
        for _ in range(3):                                    # parameter + two Adam moments
            ts.append(torch.randn(*s, generator=g).to(dev))
    ts += [torch.rand(N, 1, generator=g).to(dev), torch.rand(N, 1, generator=g).to(dev), torch.rand(N, generator=g).to(dev)]
    keep = (torch.rand(N, generator=g) > 0.66).to(dev)
    ms_hip, outs = timed(lambda: prune.compact_tensors(ts, keep))
    ms_ref, refs = timed(lambda: [t[keep] for t in ts])
    print(f"compaction of 21 tensors at N={N} (keep {int(keep.sum())}): compact_tensors {ms_hip:.2f} ms  torch boolean indexing {ms_ref:.2f} ms  "
          f"equal {all(torch.equal(a, b) for a, b in zip(outs, refs))}")


def parent_step(x, w, embed, cluster_size, decay=0.8, eps=1e-5):
    """The training step as the reference formulates it, with the search already fused (what this package ran before ema_update)."""
    n, K = x.shape[0], embed.shape[0]
    wn = (w * n / w.sum()).unsqueeze(1)
    ind = vq.nearest_code(x, embed)
    onehot = torch.nn.functional.one_hot(ind, K).to(x.dtype)
    cluster_size.mul_(decay).add_((onehot * wn).sum(0), alpha=1 - decay)
    rows_sum = torch.einsum("nd,nc->cd", x * wn, onehot)
    total = cluster_size.sum()
    smoothed = (cluster_size + eps) / (total + K * eps) * total
    embed.mul_(decay).add_(rows_sum / smoothed.unsqueeze(1), alpha=1 - decay)
    return ind


def train_leg(iters, fused_only):
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import vq_train_common as vc                                    # the float64 restatement and the parity rule of the tests
    for d in (27, 48):
        n, K = 80_000, 8192
        g = torch.Generator(device=dev).manual_seed(d)
        embed0 = torch.randn(K, d, device=dev, generator=g) * 0.3
        x = embed0[torch.randint(0, K, (n,), device=dev, generator=g)] + 0.1 * torch.randn(n, d, device=dev, generator=g)
        w = torch.exp(1.5 * torch.randn(n, device=dev, generator=g))          # heavy-tailed importance
        cs0 = torch.rand(K, device=dev, generator=g) * 10

        def block(step, reps):
            e, c = embed0.clone(), cs0.clone()
            step(x, w, e, c); step(x, w, e, c)                                 # warm
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                step(x, w, e, c)
            t1.record(); t1.synchronize()
            return t0.elapsed_time(t1)

        fused = lambda x_, w_, e_, c_: vq.ema_update(x_, e_, c_, weight=w_)    # noqa: E731
        rounds = 4
        reps = (iters + rounds - 1) // rounds
        ms_a = ms_b = 0.0
        for _ in range(rounds):                                                # alternate, so that both see the same clocks
            if not fused_only:
                ms_a += block(parent_step, reps)
            ms_b += block(fused, reps)
        ms_a, ms_b = ms_a / (rounds * reps), ms_b / (rounds * reps)
        if fused_only:
            print(f"vq train d={d}: n={n} K={K}  ema_update {ms_b:.3f} ms / iteration ({rounds * reps} iterations)")
            continue
        ea, ca, eb, cb = embed0.clone(), cs0.clone(), embed0.clone(), cs0.clone()
        ia, ib = parent_step(x, w, ea, ca), vq.ema_update(x, eb, cb, weight=w)
        same_ind = bool(torch.equal(ia, ib))
        e64, c64, _, _ = vc.ema_step_f64(x.cpu().numpy(), w.cpu().numpy(), embed0.cpu().numpy(), cs0.cpu().numpy(), ib.cpu().numpy())
        dev_a = (vc.row_error(ea.cpu().numpy(), e64), vc.row_error(ca.cpu().numpy(), c64))
        dev_b = (vc.row_error(eb.cpu().numpy(), e64), vc.row_error(cb.cpu().numpy(), c64))
        ok = same_ind and dev_b[0] <= vc.bound(dev_a[0]) and dev_b[1] <= vc.bound(dev_a[1])
        print(f"vq train d={d}: n={n} K={K}  parent path (nearest_code + one_hot + einsum + EMA) {ms_a:.3f} ms  ema_update {ms_b:.3f} ms  "
              f"ratio {ms_a / ms_b:.2f}x  ({rounds * reps} iterations each)  indices equal {same_ind}  deviation from float64 embed / cluster_size: "
              f"parent {dev_a[0]:.3g} / {dev_a[1]:.3g}, ema_update {dev_b[0]:.3g} / {dev_b[1]:.3g}  within the parity rule {ok}")
        if not (ok and ms_b < ms_a):
            raise SystemExit("vq train leg: ema_update must agree with the parent path and be faster")


def render_leg(sizes, repeats, n_views):
    import statistics
    from lightgaussian_amd import synthetic as syn, vectree
    from lightgaussian_amd.gaussian_renderer import render, render_compressed
    repeats = max(repeats, 5)
    W, H, K = 1920, 1080, 8192
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    cams = [syn.orbit_camera(k, n_views, W, H).to(dev) for k in range(n_views)]

    def spread(ms):
        return f"{statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"

    def per_view(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for cam in cams:
            fn(cam)
        t1.record(); t1.synchronize()
        return t0.elapsed_time(t1) / len(cams)

    for N in sizes:
        for deg in (2, 3):
            d = 3 * (deg + 1) ** 2
            g = syn.make_gaussians(N, sh_degree=deg)
            gen = torch.Generator().manual_seed(N + deg)
            feats = torch.cat([g._xyz, torch.zeros(N, 3), g._features_dc.transpose(1, 2).reshape(N, 3),
                               g._features_rest.transpose(1, 2).reshape(N, -1), g._opacity, g._scaling, g._rotation], dim=1)
            codebook = feats[torch.randint(0, N, (K,), generator=gen), 6:6 + d]
            mask = torch.zeros(N, dtype=torch.bool)
            mask[torch.topk(torch.rand(N, generator=gen), k=int(N * (1 - 0.6))).indices] = True
            ind = vq.nearest_code(feats[:, 6:6 + d].to(dev), codebook.to(dev)).cpu()
            cg = vectree.CompressedGaussians.from_packed(vectree.pack(feats, mask, codebook, ind), dev)
            del feats, g
            dense = cg.to_dense()
            dense_bytes = sum(t.numel() * 4 for t in (dense._xyz, dense._features_dc, dense._features_rest, dense._opacity, dense._scaling, dense._rotation))
            with torch.no_grad():
                fa = lambda cam: render(cam, dense, pipe, bg)                       # noqa: E731
                fb = lambda cam: render_compressed(cam, cg, pipe, bg)              # noqa: E731
                for _ in range(2):
                    per_view(fa); per_view(fb)
                ms_a, ms_b = [], []
                for _ in range(repeats):                                           # alternate, so that both see the same clocks
                    ms_a.append(per_view(fa)); ms_b.append(per_view(fb))
                ia, ib = fa(cams[1])["render"], fb(cams[1])["render"]
                err = float((ia - ib).abs().max() / ia.abs().max())
            out = torch.empty(N, 3, device=dev)
            model = N * (12 + 4 + 6 * (deg + 1) ** 2 + 12)
            ms_c = []
            for _ in range(2 + repeats):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for cam in cams:
                    cg.colors(cam.camera_center, out=out)
                t1.record(); t1.synchronize()
                ms_c.append(t0.elapsed_time(t1) / len(cams))
            ms_c = ms_c[2:]
            a, b = statistics.median(ms_a), statistics.median(ms_b)
            verdict = "faster" if b < min(ms_a) else "slower" if b > max(ms_a) else "within the spread of (a)"
            print(f"vq render N={N} degree={deg} {W}x{H} {n_views} views x {repeats} repeats, per view:  (a) render(to_dense()) {spread(ms_a)}  "
                  f"(b) render_compressed {spread(ms_b)}  (b)/(a) {b / a:.3f} ({verdict})  image agreement {err:.2e}")
            print(f"    lg_vq_colors alone, back to back (its working set stays in the 256 MB Infinity Cache): {spread(ms_c)}  "
                  f"{model / statistics.median(ms_c) / 1e6:.0f} GB/s by the byte model ({model // N} B / Gaussian)")
            print(f"    resident bytes: compressed {cg.nbytes() / 1e6:.1f} MB, dense {dense_bytes / 1e6:.1f} MB, ratio {dense_bytes / cg.nbytes():.2f}x")
            del cg, dense, out
            torch.cuda.empty_cache()


def finetune_leg(sizes, degrees, repeats, n_views, only_compressed):
    import statistics
    from lightgaussian_amd import synthetic as syn, vectree
    from lightgaussian_amd.gaussian_renderer import render
    repeats = max(repeats, 5)
    W, H, K = 1920, 1080, 8192
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=dev)
    cams = [syn.orbit_camera(k, n_views, W, H).to(dev) for k in range(n_views)]
    target = torch.full((3, H, W), 0.25, device=dev)

    def spread(ms):
        return f"{statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"

    def step(model, leaves, cam, options):
        for t in leaves:
            t.grad = None
        (render(cam, model, pipe, bg, options=options)["render"] - target).abs().mean().backward()

    def per_view(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for cam in cams:
            fn(cam)
        t1.record(); t1.synchronize()
        return t0.elapsed_time(t1) / len(cams)

    def peak_of(fn):
        fn(cams[0]); torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(cams[0]); torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(), base

    for N in sizes:
        for deg in degrees:
            d = 3 * (deg + 1) ** 2
            g = syn.make_gaussians(N, sh_degree=deg)
            gen = torch.Generator().manual_seed(N + deg)
            feats = torch.cat([g._xyz, torch.zeros(N, 3), g._features_dc.transpose(1, 2).reshape(N, 3),
                               g._features_rest.transpose(1, 2).reshape(N, -1), g._opacity, g._scaling, g._rotation], dim=1)
            codebook = feats[torch.randint(0, N, (K,), generator=gen), 6:6 + d]
            mask = torch.zeros(N, dtype=torch.bool)
            mask[torch.topk(torch.rand(N, generator=gen), k=int(N * (1 - 0.6))).indices] = True
            ind = vq.nearest_code(feats[:, 6:6 + d].to(dev), codebook.to(dev)).cpu()
            cg = vectree.CompressedGaussians.from_packed(vectree.pack(feats, mask, codebook, ind), dev)
            del feats, g
            tc = cg.trainable(vectree.TrainableCompressed.PARAMS)
            fc = lambda cam: step(tc, tc.parameters(), cam, None)                  # noqa: E731
            if only_compressed:
                for _ in range(2):
                    per_view(fc)
                ms_c = [per_view(fc) for _ in range(repeats)]
                print(f"vq finetune N={N} degree={deg} {W}x{H} {n_views} views x {repeats} repeats, fwd+bwd per view:  (c) trainable compressed {spread(ms_c)}")
                del cg, tc
                torch.cuda.empty_cache()
                continue
            dense = cg.to_dense()
            dense.requires_grad_(True)
            sh_leaves = [dense._xyz, dense._features_dc, dense._features_rest, dense._opacity, dense._scaling, dense._rotation]
            fa = lambda cam: step(dense, sh_leaves, cam, None)                     # noqa: E731
            fb = lambda cam: step(dense, sh_leaves, cam, {"fuse_getters": False})  # noqa: E731
            for _ in range(2):
                per_view(fa); per_view(fb); per_view(fc)
            ms_a, ms_b, ms_c = [], [], []
            for _ in range(repeats):                                               # alternate, so that all see the same clocks
                ms_a.append(per_view(fa)); ms_b.append(per_view(fb)); ms_c.append(per_view(fc))
            b, c = statistics.median(ms_b), statistics.median(ms_c)
            verdict = "faster" if c < min(ms_b) else "slower" if c > max(ms_b) else "within the spread of (b)"
            print(f"vq finetune N={N} degree={deg} {W}x{H} {n_views} views x {repeats} repeats, fwd+bwd per view:  (a) dense, fused getters {spread(ms_a)}  "
                  f"(b) dense, unfused {spread(ms_b)}  (c) trainable compressed {spread(ms_c)}  (c)/(b) {c / b:.3f} ({verdict})  "
                  f"(c)/(a) {c / statistics.median(ms_a):.3f}")
            for t in sh_leaves + tc.parameters():
                t.grad = None
            pa, ba = peak_of(fa)
            for t in sh_leaves:
                t.grad = None
            pc, bc = peak_of(fc)
            print(f"    peak allocated during one step, gradients included (both models resident: {bc / 1e6:.0f} MB before the step): "
                  f"(a) {pa / 1e6:.1f} MB  (c) {pc / 1e6:.1f} MB;  step-local (a) {(pa - ba) / 1e6:.1f} MB  (c) {(pc - bc) / 1e6:.1f} MB;  "
                  f"resident model bytes: trainable compressed {tc.nbytes() / 1e6:.1f} MB, dense "
                  f"{sum(t.numel() * 4 for t in (dense._xyz, dense._features_dc, dense._features_rest, dense._opacity, dense._scaling, dense._rotation)) / 1e6:.1f} MB")
            del cg, tc, dense, sh_leaves
            torch.cuda.empty_cache()


if args.leg == "finetune":
    finetune_leg(args.sizes, args.degrees, args.repeats, args.views, args.only_compressed)
if args.leg == "render":
    render_leg(args.sizes, args.repeats, args.views)
if args.leg in ("all", "compact"):
    compact_leg()
if args.leg in ("all", "train"):
    train_leg(args.iters, args.fused_only)
