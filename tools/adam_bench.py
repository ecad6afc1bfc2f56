#!/usr/bin/env python3
"""The optimizer step alone, on the model's six tensors (SH degree 3: 59 floats per Gaussian), three legs on one GPU in one run:

    torch     torch.optim.AdamW as the reference builds it (lr=0.0, eps=1e-15, six groups): torch's default multi-tensor step
    fused     the same with fused=True  (what `run.py --fused-adam` switches on)
    hip       lightgaussian_amd.optim.HipAdamW: one lg_adam_step launch  (what `run.py --hip-adam` switches on)

    python tools/adam_bench.py [--n 1000000 3000000] [--steps 200] [--blocks 7] [--only-hip]
    python tools/adam_bench.py --visible-frac 1.0 0.7 0.5 0.25 0.1 [--visible-pattern random|blocks]

--visible-frac F [F ...]: the legs are `hip` (the dense lg_adam_step) and, per fraction, `rows F`: HipAdamW.step(visible=mask), one
lg_adam_step_rows launch, with F of the rows visible -- `random` rows, or contiguous `blocks` of 4096 rows (a view's Morton-ordered
neighbourhoods).  All legs alternate in the same run; GB/s of a masked leg is the DENSE byte model over its time (what the dense
step would have needed), so the figure to read is the time.

Gradients: one third of the rows exactly zero (Gaussians outside the view), the rest normal.  Every leg steps its own copy of the
parameters with the same gradients.  Per size: `--blocks` alternating blocks of `--steps` steps per leg after a warm-up, each block
between two hipEvents; printed as median (min..max) of the per-step time over the blocks, and GB/s by the byte model (16 B read +
12 B written per element).  --only-hip runs the hip leg alone, for `rocprofv3 --kernel-trace --stats -- python tools/adam_bench.py
--only-hip` (the kernel's own time)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, optim  # noqa: E402

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)
BYTES_PER_ELEMENT = 28


def shapes(N, degree):
    return dict(xyz=(N, 3), f_dc=(N, 1, 3), f_rest=(N, (degree + 1) ** 2 - 1, 3), opacity=(N, 1), scaling=(N, 3), rotation=(N, 4))


def make_leg(kind, params0, grads):
    ps = {n: torch.nn.Parameter(t.clone()) for n, t in params0.items()}
    groups = [{"params": [ps[n]], "lr": LRS[n], "name": n} for n in NAMES]
    if kind == "hip":
        opt = optim.HipAdamW(groups, lr=0.0, eps=1e-15)
    else:
        opt = torch.optim.AdamW(groups, lr=0.0, eps=1e-15, **({"fused": True} if kind == "fused" else {}))
    for n in NAMES:
        ps[n].grad = grads[n]
    return opt


def make_mask(N, frac, pattern, dev):
    gen = torch.Generator(device=dev).manual_seed(int(frac * 1000) + 17)
    if frac >= 1.0:
        return torch.ones(N, dtype=torch.bool, device=dev)
    if pattern == "random":
        return torch.rand(N, device=dev, generator=gen) < frac
    nb = (N + 4095) // 4096
    return (torch.rand(nb, device=dev, generator=gen) < frac).repeat_interleave(4096)[:N].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--visible-frac", type=float, nargs="+", default=[])
    ap.add_argument("--visible-pattern", choices=("random", "blocks"), default="random")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    kinds = ("hip",) if (args.only_hip or args.visible_frac) else ("torch", "fused", "hip")
    rows_kinds = {f"rows {f:g}": f for f in args.visible_frac}
    if args.only_hip and rows_kinds:
        kinds = ()
    kinds = kinds + tuple(rows_kinds)
    print(f"library build {_lib.build_id()}, span {optim.SPAN}, {args.blocks} blocks of {args.steps} steps per leg")
    for N in args.n:
        gen = torch.Generator(device=dev).manual_seed(N)
        params0, grads = {}, {}
        for name, shape in shapes(N, args.degree).items():
            params0[name] = torch.randn(shape, device=dev, generator=gen)
            g = torch.randn(shape, device=dev, generator=gen)
            g[0::3] = 0.0
            grads[name] = g
        numel = sum(t.numel() for t in params0.values())
        legs = {k: make_leg("hip" if k in rows_kinds else k, params0, grads) for k in kinds}
        masks = {k: make_mask(N, f, args.visible_pattern, dev) for k, f in rows_kinds.items()}
        for k, m in masks.items():
            print(f"  {k}: {args.visible_pattern}, {float(m.float().mean()):.4f} of {N} rows visible")
            legs[k].step = (lambda o, m: lambda: type(o).step(o, visible=m))(legs[k], m)
        for opt in legs.values():
            for _ in range(args.warmup):
                opt.step()
        torch.cuda.synchronize()
        times = {k: [] for k in kinds}
        for _ in range(args.blocks):
            for k in kinds:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    legs[k].step()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) / args.steps)
        gb = numel * BYTES_PER_ELEMENT / 1e9
        print(f"N = {N}: {numel} elements, {gb:.3f} GB per step by the byte model")
        for k in kinds:
            t = times[k]
            med = statistics.median(t)
            print(f"  {k:9s} {med:.3f} ms ({min(t):.3f}..{max(t):.3f})   {gb / med * 1e3:7.1f} GB/s ({gb / max(t) * 1e3:.1f}..{gb / min(t) * 1e3:.1f})")
        print(json.dumps({"adam_bench": {"N": N, "numel": numel, "steps": args.steps, "blocks": args.blocks, "build": _lib.build_id(), "visible_pattern": args.visible_pattern if rows_kinds else None,
                                         "ms_per_step": {k: [round(x, 4) for x in times[k]] for k in kinds}}}))
        del legs, params0, grads
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
