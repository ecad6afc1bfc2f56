#!/usr/bin/env python3
"""Densification alone, on the model's six tensors with their Adam moments (SH degree 3: 59 floats per Gaussian), on one GPU in one run:

    densify_and_prune    torch   lightgaussian_amd.densify backend="torch": the reference's op sequence restated (masks, nonzero, gathers,
                                 cat of every tensor and moment) -- the comparand
                         hip     backend="hip": lg_densify_plan + one lg_densify_rows launch, one 32-byte read-back
    view statistics      torch   the reference's four boolean-mask statements (add_densification_stats + the trainer's max_radii2D line)
                         hip     densify.accumulate_stats: one lg_densify_stats launch, no host read

    python tools/densify_bench.py [--n 1000000 3000000] [--reps 5] [--stat-steps 50] [--blocks 7] [--only-hip]

A few percent of the rows are above the gradient threshold (most of them small: cloned; the rest split), well under one percent is
pruned -- the trainer's regime.  Every call starts from a fresh copy of the same state (building it is outside the timed region).
Per size: `--blocks` alternating blocks per leg after a warm-up, each block between two hipEvents; printed as median (min..max) of the
per-call time over the blocks.

Byte model, stated before the run (f = 59 floats per row, v = visible fraction, N' = output rows):
    lg_densify_stats    N (1 + v 40) B: the filter byte; per visible row 12 B of gradient, accum / denom / max_radii2D read and written, radii read
    lg_densify_plan     N (24 + 1 + 1) + 8 N' B: scaling, opacity, accum, denom once; the flag byte written and read; the map written
    lg_densify_rows     N' (8 + 3 f 4) + N_keep 3 f 4 + N' 12 B: the map, every parameter and moment word written, the words of kept rows
                        read (parameters of new rows too), the three bookkeeping tensors zeroed
--only-hip runs the hip legs alone, for `rocprofv3 --kernel-trace --stats -- python tools/densify_bench.py --only-hip`."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, densify  # noqa: E402

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
ARGS = dict(max_grad=0.0002, min_opacity=0.005, extent=5.0, max_screen_size=20)


def shapes(N, degree):
    return dict(xyz=(N, 3), f_dc=(N, 1, 3), f_rest=(N, (degree + 1) ** 2 - 1, 3), opacity=(N, 1), scaling=(N, 3), rotation=(N, 4))


class Model:
    def __init__(self, state):
        for n in NAMES:
            setattr(self, ATTRS[n], torch.nn.Parameter(state[n].clone()))
        self.optimizer = torch.optim.AdamW([{"params": [getattr(self, ATTRS[n])], "lr": 1e-3, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
        for n in NAMES:
            self.optimizer.state[getattr(self, ATTRS[n])] = {"step": torch.tensor(1.0), "exp_avg": state["m_" + n].clone(),
                                                             "exp_avg_sq": state["v_" + n].clone()}
        self.percent_dense = 0.01
        self.xyz_gradient_accum, self.denom, self.max_radii2D = state["accum"].clone(), state["denom"].clone(), state["radii"].clone()


def make_state(N, degree, dev):
    gen = torch.Generator(device=dev).manual_seed(N)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)      # noqa: E731
    state = {}
    for n, s in shapes(N, degree).items():
        state[n], state["m_" + n], state["v_" + n] = rnd(s), 0.1 * rnd(s), 0.01 * rnd(s).abs()
    state["scaling"] = 0.7 * rnd(N, 3) + math.log(0.012)
    state["opacity"] = 2.0 * rnd(N, 1)
    hot = torch.rand(N, 1, device=dev, generator=gen) < 0.05
    state["denom"] = torch.randint(1, 9, (N, 1), device=dev, generator=gen).float()
    state["accum"] = torch.where(hot, 4.0, 0.2) * 0.0002 * state["denom"]
    state["radii"] = torch.zeros(N, device=dev)
    return state


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = 0.0
    for _ in range(reps):
        arg = fn.prepare()
        a.record()
        fn(arg)
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
    return total / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stat-steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--only-hip", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    kinds = ("hip",) if args.only_hip else ("torch", "hip")
    print(f"library build {_lib.build_id()}, {args.blocks} blocks of {args.reps} calls / {args.stat_steps} statistics steps per leg")
    for N in args.n:
        state = make_state(N, args.degree, dev)
        f = sum(math.prod(s[1:]) for s in shapes(N, args.degree).values())
        record = {}

        def densify_leg(kind):
            def call(model):
                record[kind] = densify.densify_and_prune(model, backend=kind, **ARGS)
            call.prepare = lambda: Model(state)
            return call

        gen = torch.Generator(device=dev).manual_seed(7)
        grad = torch.randn(N, 3, device=dev, generator=gen) * 1e-4
        visible = torch.rand(N, device=dev, generator=gen) < 0.6
        radii = torch.randint(0, 40, (N,), device=dev, generator=gen, dtype=torch.int32)
        vp = torch.zeros(N, 3, device=dev)
        vp.grad = grad
        stat_models = {k: Model({k2: (v if k2 in ("accum", "denom", "radii") else v[:1]) for k2, v in state.items()}) for k in kinds}

        def stats_leg(kind):
            m = stat_models[kind]

            def call(_):
                for _ in range(args.stat_steps):
                    if kind == "hip":
                        densify.accumulate_stats(m, vp, visible, radii=radii)
                    else:
                        m.max_radii2D[visible] = torch.max(m.max_radii2D[visible], radii[visible])
                        m.xyz_gradient_accum[visible] += torch.norm(vp.grad[visible, :2], dim=-1, keepdim=True)
                        m.denom[visible] += 1
            call.prepare = lambda: None
            return call

        legs = {("densify", k): densify_leg(k) for k in kinds}
        legs.update({("stats", k): stats_leg(k) for k in kinds})
        for fn in legs.values():
            timed(fn, 1)
        torch.cuda.synchronize()
        times = {key: [] for key in legs}
        for _ in range(args.blocks):
            for key, fn in legs.items():
                t = timed(fn, args.reps if key[0] == "densify" else 1)
                times[key].append(t if key[0] == "densify" else t / args.stat_steps)
        rec = record["hip"]
        v = float(visible.float().mean())
        model_bytes = {"stats": N * (1 + v * 40), "plan": N * 26 + 8 * rec["N_out"],
                       "rows": rec["N_out"] * (8 + 3 * f * 4 + 12) + rec["n_keep"] * 3 * f * 4 + (rec["N_out"] - rec["n_keep"]) * f * 4}
        print(f"N = {N}: {rec}")
        print("  byte model: " + ", ".join(f"{k} {b / 1e6:.1f} MB" for k, b in model_bytes.items()))
        for key in legs:
            t = times[key]
            print(f"  {key[0]:8s} {key[1]:6s} {statistics.median(t):9.4f} ms ({min(t):.4f}..{max(t):.4f})")
        print(json.dumps({"densify_bench": {"N": N, "record": rec, "reps": args.reps, "stat_steps": args.stat_steps, "blocks": args.blocks,
                                            "build": _lib.build_id(), "model_bytes": {k: int(b) for k, b in model_bytes.items()},
                                            "ms": {f"{a}_{b}": [round(x, 4) for x in t] for (a, b), t in times.items()}}}))
        del legs, state, stat_models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
