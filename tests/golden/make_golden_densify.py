"""Golden states for densification, produced by the REFERENCE's own code on the CPU: scene/gaussian_model.py's
GaussianModel.training_setup, one real optimizer (AdamW) step so that the moments are non-zero, add_densification_stats, and
densify_and_prune -- the unmodified methods, loaded through tests/dropin_common.load().

The reference asks for device="cuda" everywhere and draws its noise inside densify_and_split.  The name `torch` inside
scene.gaussian_model and utils.general_utils is therefore bound, for the duration of this script, to a proxy that
  * drops device="cuda" from the tensor factories,
  * evaluates normal(mean, std) as mean + std * z and records the unit-normal z (ATen's own evaluation: normal_(0, 1) * std + mean),
  * turns cuda.empty_cache() into a no-op.
Everything else is torch's own.

Stored per case (tests/densify_common.py reads them): the input state, the arguments, the noise, the full output state (parameters,
moments; the bookkeeping tensors are asserted zero here), the counts {N_out, n_keep, n_clone, n_s, n_child, step}, and R64: the two
child formulas evaluated in float64 on the float32 inputs.  The counts come from the contract as DESIGN section 10.2 words it,
evaluated here in float32 torch ops, and the reference's output is asserted to be exactly the rows that contract names, in its
order -- the generator fails if the contract and the reference ever disagree.

Margins.  Apart from the exact-tie row of case "tie" (g == thr_g, which must be selected), no max scale m, no m / 1.6 and no
sigmoid(opacity) lies within relative 1e-4 of the threshold it is compared with (asserted): a last-bit difference between the CPU's
and the GPU's exp cannot flip a decision.
Run:  python tests/golden/make_golden_densify.py   (needs the reference tree; the committed .npz travels, < 1 MiB)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import densify_common as dc  # noqa: E402
import dropin_common  # noqa: E402

_, gm, _ = dropin_common.load()
gu = importlib.import_module("utils.general_utils")


class TorchProxy:
    def __init__(self):
        self.noise = []
        self.cuda = types.SimpleNamespace(empty_cache=lambda: None)

    def __getattr__(self, name):
        attr = getattr(torch, name)
        if name in ("zeros", "ones", "empty", "full", "tensor", "zeros_like", "arange"):
            def factory(*a, **kw):
                if kw.get("device") == "cuda":
                    del kw["device"]
                return attr(*a, **kw)
            return factory
        return attr

    def normal(self, mean, std):
        z = torch.normal(torch.zeros_like(mean), torch.ones_like(std))
        self.noise.append(z)
        return mean + std * z


def training_args(percent_dense):
    return types.SimpleNamespace(percent_dense=percent_dense, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                                 position_lr_max_steps=30000, feature_lr=2.5e-3, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)


def log_uniform(gen, n, lo, hi):
    return torch.exp(torch.rand(n, generator=gen) * (np.log(hi) - np.log(lo)) + np.log(lo))


def away_from(values, thresholds, what):
    for thr in thresholds:
        rel = ((values.double() - thr).abs() / abs(thr)).min().item() if values.numel() else 1.0
        assert rel > 1e-4, f"{what} within {rel:.2e} of {thr}"


# name: N, degree, (scale range), max_grad, min_opacity, extent, max_screen_size, fraction of rows with g above max_grad
PERCENT_DENSE = 0.01
CASE_SPECS = {
    "mixed": dict(n=300, deg=1, scale=(0.004, 1.2), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=20, hot=0.75),
    "no_screen": dict(n=64, deg=1, scale=(0.004, 1.2), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=None, hot=0.7),
    "none_selected": dict(n=64, deg=1, scale=(0.004, 1.2), max_grad=1000.0, min_opacity=0.005, extent=5.0, screen=20, hot=0.7, level=0.0002),
    "all_clone": dict(n=64, deg=1, scale=(0.004, 0.045), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=20, hot=1.0),
    "all_split": dict(n=64, deg=1, scale=(0.06, 1.2), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=20, hot=1.0, floor=0.06),
    "all_pruned": dict(n=64, deg=1, scale=(0.004, 1.2), max_grad=0.0002, min_opacity=2.0, extent=5.0, screen=20, hot=0.7),
    "denom0": dict(n=64, deg=1, scale=(0.004, 1.2), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=20, hot=0.7, denom0=0.5),
    "tie": dict(n=64, deg=1, scale=(0.004, 1.2), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=20, hot=0.5, tie=17),
    "deg0": dict(n=64, deg=0, scale=(0.004, 1.2), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=20, hot=0.7),
    "deg3": dict(n=60, deg=3, scale=(0.004, 1.2), max_grad=0.0002, min_opacity=0.005, extent=5.0, screen=20, hot=0.7),
}
assert tuple(CASE_SPECS) == dc.CASES

proxy = TorchProxy()
gm.torch = gu.torch = proxy
out = {}
try:
    for ci, (name, spec) in enumerate(CASE_SPECS.items()):
        gen = torch.Generator().manual_seed(20261018 + ci)
        torch.manual_seed(777 + ci)                       # the reference's noise comes from the global generator
        n, deg = spec["n"], spec["deg"]
        f32 = lambda v: float(np.float32(v))              # noqa: E731
        thr_g, thr_d, thr_w = f32(spec["max_grad"]), f32(PERCENT_DENSE * spec["extent"]), f32(0.1 * spec["extent"])
        shp = dc.shapes(n, deg)
        params = {k: torch.randn(s, generator=gen) for k, s in shp.items()}
        sc = log_uniform(gen, n * 3, *spec["scale"]).reshape(n, 3)
        if "floor" in spec:                               # every row's largest scale above thr_d
            sc[:, 0] = sc[:, 0].clamp_min(spec["floor"])
        params["scaling"] = torch.log(sc)
        params["opacity"] = 3.0 * torch.randn(n, 1, generator=gen)
        params["rotation"] = torch.randn(n, 4, generator=gen) * log_uniform(gen, n, 0.2, 5.0)[:, None]

        model = gm.GaussianModel(deg)
        model.spatial_lr_scale = 1.0
        for k in dc.NAMES:
            setattr(model, dc.ATTRS[k], torch.nn.Parameter(params[k].clone()))
        model.max_radii2D = torch.zeros(n)
        model.training_setup(training_args(PERCENT_DENSE))
        assert isinstance(model.optimizer, torch.optim.AdamW)
        for k in dc.NAMES:
            getattr(model, dc.ATTRS[k]).grad = torch.randn(shp[k], generator=gen) * 0.1
        model.optimizer.step()
        model.optimizer.zero_grad(set_to_none=True)
        step = 1

        # statistics through the reference's own add_densification_stats: `views` views, each with its own visibility
        views = 4
        hot = torch.rand(n, generator=gen) < spec["hot"]
        level = torch.where(hot, log_uniform(gen, n, 3.0, 40.0), log_uniform(gen, n, 0.02, 0.5)) * spec.get("level", spec["max_grad"])
        stats_in = []
        for v in range(views):
            vis = torch.rand(n, generator=gen) < (1.0 - spec.get("denom0", 0.0)) * 0.8
            if v == 0 and "denom0" not in spec:
                vis[:] = True
            d = torch.randn(n, 2, generator=gen)
            d = d / d.norm(dim=1, keepdim=True) * (level * (0.5 + torch.rand(n, generator=gen)))[:, None]
            vp = torch.zeros(n, 3)
            vp.grad = torch.cat([d, torch.randn(n, 1, generator=gen)], dim=1)
            if name == "mixed":
                stats_in.append((vp.grad.clone(), vis.clone()))
            model.add_densification_stats(vp, vis)
        if name == "mixed":
            out["stats/grad"] = torch.stack([g for g, _ in stats_in]).numpy()
            out["stats/filter"] = torch.stack([f for _, f in stats_in]).numpy()
            out["stats/accum"] = model.xyz_gradient_accum.numpy().copy()
            out["stats/denom"] = model.denom.numpy().copy()
        if "denom0" in spec:                               # a few rows with a sum but no count: g = inf, selected
            never = torch.nonzero(model.denom.reshape(-1) == 0).reshape(-1)
            assert never.numel() >= 8
            model.xyz_gradient_accum[never[:3]] = 1.0
        if "tie" in spec:
            model.xyz_gradient_accum[spec["tie"]] = thr_g
            model.denom[spec["tie"]] = 1.0
        model.max_radii2D = torch.rand(n, generator=gen) * 40.0

        inputs = {k: getattr(model, dc.ATTRS[k]).detach().clone() for k in dc.NAMES}
        moments = {k: (model.optimizer.state[getattr(model, dc.ATTRS[k])]["exp_avg"].clone(),
                       model.optimizer.state[getattr(model, dc.ATTRS[k])]["exp_avg_sq"].clone()) for k in dc.NAMES}
        accum, denom, radii = model.xyz_gradient_accum.clone(), model.denom.clone(), model.max_radii2D.clone()

        # the contract, in float32 torch ops, and the margins
        s = torch.exp(inputs["scaling"]); m = s.max(dim=1).values
        sigma = torch.sigmoid(inputs["opacity"]).reshape(-1)
        g = (accum / denom).reshape(-1); g[g.isnan()] = 0.0
        away_from(m, (thr_d,) + ((thr_w,) if spec["screen"] else ()), f"{name}: max scale")
        away_from(m / np.float32(1.6), (thr_w,) if spec["screen"] else (), f"{name}: child max scale")
        away_from(sigma, (f32(spec["min_opacity"]),), f"{name}: opacity")
        gg = g.clone()
        if "tie" in spec:
            assert gg[spec["tie"]].item() == thr_g
            gg[spec["tie"]] = 1.0
        away_from(gg[torch.isfinite(gg)], (thr_g,), f"{name}: gradient")
        pruned = lambda sg, mu: (sg < f32(spec["min_opacity"])) | ((mu > thr_w) if spec["screen"] else torch.zeros_like(sg, dtype=torch.bool))   # noqa: E731
        hot_rows = g >= thr_g
        split, clone = hot_rows & (m > thr_d), hot_rows & (m <= thr_d)
        keep_rows = torch.nonzero(~split & ~pruned(sigma, m)).reshape(-1)
        clone_rows = torch.nonzero(clone & ~pruned(sigma, m)).reshape(-1)
        split_rows = torch.nonzero(split).reshape(-1)
        child_ok = ~pruned(sigma, m / np.float32(1.6))[split_rows]
        parents, rank = split_rows[child_ok], torch.arange(split_rows.numel())[child_ok]
        n_keep, n_clone, n_s, n_child = keep_rows.numel(), clone_rows.numel(), split_rows.numel(), parents.numel()
        n_out = n_keep + n_clone + 2 * n_child

        proxy.noise.clear()
        model.densify_and_prune(spec["max_grad"], spec["min_opacity"], spec["extent"], spec["screen"])
        assert len(proxy.noise) == 1 and tuple(proxy.noise[0].shape) == (2 * n_s, 3)
        noise = proxy.noise[0].clone()

        # the reference's output is what the contract names, in its order
        gather = torch.cat([keep_rows, clone_rows, parents, parents])
        assert model._xyz.shape[0] == n_out, (name, model._xyz.shape[0], n_out)
        for k in dc.NAMES:
            p = getattr(model, dc.ATTRS[k])
            st = model.optimizer.state[p]
            assert p.shape[0] == n_out and float(st["step"]) == step
            rows = slice(0, n_keep + n_clone) if k in ("xyz", "scaling") else slice(0, n_out)
            assert dc.same_bits(p[rows], inputs[k][gather][rows]), (name, k)
            for key, old in zip(("exp_avg", "exp_avg_sq"), moments[k]):
                assert dc.same_bits(st[key][:n_keep], old[keep_rows]) and not st[key][n_keep:].any(), (name, k, key)
            out[f"{name}/out_{k}"] = p.detach().numpy().copy()
            out[f"{name}/out_m_{k}"] = st["exp_avg"].numpy().copy()
            out[f"{name}/out_v_{k}"] = st["exp_avg_sq"].numpy().copy()
        assert tuple(model.xyz_gradient_accum.shape) == (n_out, 1) and tuple(model.denom.shape) == (n_out, 1) and tuple(model.max_radii2D.shape) == (n_out,)
        assert not model.xyz_gradient_accum.any() and not model.denom.any() and not model.max_radii2D.any()
        if "tie" in spec:
            assert spec["tie"] in clone_rows.tolist() + split_rows.tolist()
        noise_rows = torch.cat([rank, n_s + rank]).numpy()
        two = lambda k: np.concatenate([inputs[k].numpy()[parents.numpy()]] * 2, axis=0)          # noqa: E731
        r64_xyz, r64_scaling = dc.child_r64(two("xyz"), two("scaling"), two("rotation"), noise.numpy()[noise_rows])
        first = n_keep + n_clone
        for label, got, ref in (("xyz", model._xyz, r64_xyz), ("scaling", model._scaling, r64_scaling)):
            err = np.abs(got.detach().numpy()[first:].astype(np.float64) - ref).max() if n_child else 0.0
            assert err <= 1e-5 * max(1.0, np.abs(ref).max() if n_child else 1.0), (name, label, err)     # R64 is the formula the reference evaluates
        out[f"{name}/r64_xyz"], out[f"{name}/r64_scaling"] = r64_xyz, r64_scaling
        for k in dc.NAMES:
            out[f"{name}/in_{k}"] = inputs[k].numpy()
            out[f"{name}/in_m_{k}"], out[f"{name}/in_v_{k}"] = moments[k][0].numpy(), moments[k][1].numpy()
        out[f"{name}/in_accum"], out[f"{name}/in_denom"], out[f"{name}/in_max_radii2D"] = accum.numpy(), denom.numpy(), radii.numpy()
        out[f"{name}/noise"] = noise.numpy()
        out[f"{name}/args"] = np.array([spec["max_grad"], spec["min_opacity"], spec["extent"], np.nan if spec["screen"] is None else spec["screen"],
                                        PERCENT_DENSE], dtype=np.float64)
        out[f"{name}/counts"] = np.array([n_out, n_keep, n_clone, n_s, n_child, step, spec.get("tie", -1)], dtype=np.int64)
        print(f"{name}: N {n} -> {n_out}  keep {n_keep} clone {n_clone} split-selected {n_s} (children kept of {n_child})")
finally:
    gm.torch = gu.torch = torch

c = out["mixed/counts"]
assert c[1] > 0 and c[2] > 0 and c[4] > 0 and c[3] > c[4] and c[1] + c[3] < 300, "the mixed case exercises every kind of row"
assert out["all_pruned/counts"][0] == 0 and out["none_selected/counts"][2] == 0 and out["none_selected/counts"][3] == 0
assert out["all_clone/counts"][3] == 0 and out["all_clone/counts"][2] > 0 and out["all_split/counts"][3] == 64 and out["all_split/counts"][1] == 0
path = os.path.join(HERE, "reference_densify.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1 << 20
