#!/usr/bin/env python3
"""3DGS-MCMC's three per-Gaussian steps alone, on the model's six tensors with their Adam moments (SH degree 3: 59 floats per Gaussian),
on one GPU in one run:

    add_noise    torch   lightgaussian_amd.mcmc backend="torch": the published op sequence (build_rotation, L @ L^T, the gated noise, bmm,
                         add_) -- what a user runs without the library, the comparand
                 hip     backend="hip": one lg_mcmc_noise launch in place
    relocate     torch   5 % of the rows dead: bincount, the float32 double loop over the binomial table, indexed copies
                 hip     lg_mcmc_plan + one lg_mcmc_rows launch in place, one host read (the dead count)
    grow         torch   5 % new rows: the same formulas, every tensor and moment re-allocated with torch.cat
                 hip     lg_mcmc_plan + one lg_mcmc_rows launch into new tensors

    python tools/mcmc_bench.py [--n 1000000 3000000] [--reps 5] [--noise-steps 20] [--blocks 7] [--only-hip]

The noise tensor and the draws are made outside the timed region (both backends would draw them alike); relocate and grow start from a
fresh copy of the same state for every call (building it is outside the timed region too).  Per size: `--blocks` alternating blocks per
leg after a warm-up, each block between two hipEvents; printed as median (min..max) of the per-call time over the blocks.

The noise legs run their steps back to back on the same tensors (50 times as many for hip, whose step is far shorter): at 3 M the
204 MB working set fits the 256 MiB Infinity Cache, so the effective bytes/s printed is not an HBM figure.
Byte model of lg_mcmc_noise, stated before the run: 68 B per row -- xyz read and written (24), scaling (12), rotation (16), opacity (4),
noise (12).  Rows whose gate is exactly 0 read their opacity alone, so the model is an upper bound on the traffic; the opacities here are
2 N(0, 1) logits, of which the part above sigmoid^-1(0.888), where the gate vanishes, is printed.
--only-hip runs the hip legs alone, for `rocprofv3 --kernel-trace --stats -- python tools/mcmc_bench.py --only-hip`."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib, mcmc  # noqa: E402

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
NOISE_BYTES_PER_ROW = 68


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


def make_state(N, degree, dev, dead):
    gen = torch.Generator(device=dev).manual_seed(N)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)      # noqa: E731
    state = {}
    for n, s in shapes(N, degree).items():
        state[n], state["m_" + n], state["v_" + n] = rnd(s), 0.1 * rnd(s), 0.01 * rnd(s).abs()
    state["scaling"] = 0.7 * rnd(N, 3) + math.log(0.012)
    state["opacity"] = 2.0 * rnd(N, 1)
    is_dead = torch.rand(N, 1, device=dev, generator=gen) < dead
    state["opacity"] = torch.where(is_dead, torch.full_like(state["opacity"], -7.0), state["opacity"].clamp(min=-4.0))
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
    ap.add_argument("--noise-steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dead", type=float, default=0.05)
    ap.add_argument("--only-hip", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    kinds = ("hip",) if args.only_hip else ("torch", "hip")
    print(f"library build {_lib.build_id()}, {args.blocks} blocks of {args.reps} calls / {args.noise_steps} (torch), {50 * args.noise_steps} (hip) noise steps per leg")
    for N in args.n:
        state = make_state(N, args.degree, dev, args.dead)
        gen = torch.Generator(device=dev).manual_seed(7)
        noise = torch.randn(N, 3, device=dev, generator=gen)
        sigma = torch.sigmoid(state["opacity"]).reshape(-1)
        dead = sigma <= 0.005
        alive = torch.nonzero(~dead).reshape(-1)
        n_dead = int(dead.sum())
        reloc_draws = alive[torch.multinomial(sigma[alive], n_dead, replacement=True, generator=gen)]
        n_new = int(1.05 * N) - N
        grow_draws = torch.multinomial(sigma, n_new, replacement=True, generator=gen)
        record = {}
        noise_steps = {"torch": args.noise_steps, "hip": 50 * args.noise_steps}      # windows of comparable length: the hip step is far shorter
        noise_models = {k: Model({k2: (v if k2 in ("xyz", "scaling", "rotation", "opacity") else v[:1]) for k2, v in state.items()}) for k in kinds}

        def noise_leg(kind):
            m = noise_models[kind]

            def call(_):
                for _ in range(noise_steps[kind]):
                    mcmc.add_noise(m, 1.6e-6, noise=noise, backend=kind)       # (c = 0.8: the positions stay finite over the whole run)
            call.prepare = lambda: None
            return call

        def relocate_leg(kind):
            def call(model):
                record["relocate", kind] = mcmc.relocate(model, draws=reloc_draws, backend=kind)
            call.prepare = lambda: Model(state)
            return call

        def grow_leg(kind):
            def call(model):
                record["grow", kind] = mcmc.grow(model, 10 ** 9, draws=grow_draws, backend=kind)
            call.prepare = lambda: Model(state)
            return call

        legs = {}
        for what, make in (("add_noise", noise_leg), ("relocate", relocate_leg), ("grow", grow_leg)):
            legs.update({(what, k): make(k) for k in kinds})
        for fn in legs.values():
            timed(fn, 1)
        torch.cuda.synchronize()
        times = {key: [] for key in legs}
        for _ in range(args.blocks):
            for key, fn in legs.items():
                t = timed(fn, 1 if key[0] == "add_noise" else args.reps)
                times[key].append(t / noise_steps[key[1]] if key[0] == "add_noise" else t)
        for key, rec in record.items():
            assert rec["backend"] == key[1], (key, rec)
        noise_bytes = N * NOISE_BYTES_PER_ROW
        gated = float((sigma > 0.888).float().mean())
        print(f"N = {N}: {n_dead} dead rows relocated, {n_new} rows grown, {int(record['relocate', 'hip']['n_sources'])} / "
              f"{int(record['grow', 'hip']['n_sources'])} distinct sources; gate exactly 0 on about {gated:.3f} of the rows")
        for key in legs:
            t = times[key]
            line = f"  {key[0]:9s} {key[1]:6s} {statistics.median(t):9.4f} ms ({min(t):.4f}..{max(t):.4f})"
            if key == ("add_noise", "hip"):
                line += f"   {noise_bytes / 1e6:.0f} MB by the 68 B/row model: {noise_bytes / statistics.median(t) / 1e6:.0f} GB/s effective"
            print(line)
        print(json.dumps({"mcmc_bench": {"N": N, "n_dead": n_dead, "n_new": n_new, "reps": args.reps, "noise_steps": args.noise_steps,
                                         "blocks": args.blocks, "build": _lib.build_id(), "noise_model_bytes": noise_bytes,
                                         "ms": {f"{a}_{b}": [round(x, 4) for x in t] for (a, b), t in times.items()}}}))
        del legs, state, noise_models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
