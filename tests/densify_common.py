"""Shared by tests/golden/make_golden_densify.py, tests/test_densify_host.py and tests/test_gpu_densify.py (test infrastructure).

The goldens (tests/golden/reference_densify.npz) hold, per case, the state of a reference GaussianModel after one real AdamW step
(parameters, moments, statistics), the arguments of densify_and_prune, the unit-normal noise the reference drew, the reference's
own output state, and a float64 evaluation (R64) of the two child formulas on the same float32 inputs.

Parity rule for the computed child rows (the project's rule, tests/test_gpu_adam.py):
    max|ours - R64| <= 4 max|golden32 - R64| + 2^-23 max|R64|
Everything else -- row counts, row order, every copied row, every moment -- is compared bit for bit."""
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reference_densify.npz")
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
CASES = ("mixed", "no_screen", "none_selected", "all_clone", "all_split", "all_pruned", "denom0", "tie", "deg0", "deg3")
# training_setup's learning rates (arguments/__init__.py defaults, spatial_lr_scale 1)
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)
SHRINK32 = float(np.float32(0.8 * 2))


def shapes(n, deg):
    return dict(xyz=(n, 3), f_dc=(n, 1, 3), f_rest=(n, (deg + 1) ** 2 - 1, 3), opacity=(n, 1), scaling=(n, 3), rotation=(n, 4))


def bits(t):       # (not common.bits: an int32 torch view on the CPU, for torch.equal)
    return t.detach().contiguous().cpu().view(torch.int32)


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and torch.equal(bits(a), bits(b))


class Model:
    """The attribute surface densify.densify_and_prune / prune.prune_points touch: the reference GaussianModel's."""

    def __init__(self, params, moments, step, percent_dense, accum, denom, max_radii2D, device="cpu", cls=torch.optim.AdamW, dtype=torch.float32):
        mk = lambda a: torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype).clone()      # noqa: E731
        for n in NAMES:
            setattr(self, ATTRS[n], torch.nn.Parameter(mk(params[n])))
        self.optimizer = cls([{"params": [getattr(self, ATTRS[n])], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=1e-15)
        if moments is not None:
            for n in NAMES:
                self.optimizer.state[getattr(self, ATTRS[n])] = {"step": torch.tensor(float(step)), "exp_avg": mk(moments[n][0]),
                                                                 "exp_avg_sq": mk(moments[n][1])}
        self.percent_dense = percent_dense
        self.xyz_gradient_accum, self.denom, self.max_radii2D = mk(accum), mk(denom), mk(max_radii2D)

    @property
    def get_xyz(self):
        return self._xyz

    def param(self, n):
        return getattr(self, ATTRS[n])


_FILE = {}


def golden():
    if "z" not in _FILE:
        _FILE["z"] = dict(np.load(GOLDEN))
    return _FILE["z"]


def case(name):
    z = golden()
    c = {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + "/")}
    a = c["args"]
    c["kwargs"] = dict(max_grad=float(a[0]), min_opacity=float(a[1]), extent=float(a[2]), max_screen_size=None if math.isnan(a[3]) else float(a[3]))
    c["percent_dense"] = float(a[4])
    return c


def model_of(c, device="cpu", cls=torch.optim.AdamW):
    return Model({n: c[f"in_{n}"] for n in NAMES}, {n: (c[f"in_m_{n}"], c[f"in_v_{n}"]) for n in NAMES}, int(c["counts"][5]), c["percent_dense"],
                 c["in_accum"], c["in_denom"], c["in_max_radii2D"], device=device, cls=cls)


def child_r64(xyz, scaling, rotation, noise):
    """The two child formulas in float64 on float32 inputs (numpy [n, .] arrays of the PARENTS, one noise row each)."""
    xyz, scaling, q, z = (np.asarray(a, np.float64) for a in (xyz, scaling, rotation, noise))
    s = np.exp(scaling)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    r, x, y, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + w * w), 2 * (x * y - r * w), 2 * (x * w + r * y),
                  2 * (x * y + r * w), 1 - 2 * (x * x + w * w), 2 * (y * w - r * x),
                  2 * (x * w - r * y), 2 * (y * w + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    return np.einsum("nij,nj->ni", R, z * s) + xyz, np.log(s / SHRINK32)


def rule(label, ours, gold32, r64):
    ours, gold32, r64 = (np.asarray(a, np.float64) for a in (ours, gold32, r64))
    assert ours.shape == r64.shape, (label, ours.shape, r64.shape)
    if r64.size == 0:
        return
    eo, eg = np.abs(ours - r64).max(), np.abs(gold32 - r64).max()
    bound = 4.0 * eg + 2.0 ** -23 * np.abs(r64).max()
    print(f"{label}: |ours - R64| {eo:.3e}  |golden32 - R64| {eg:.3e}  bound {bound:.3e}")
    assert np.isfinite(eo) and eo <= bound, f"{label}: |ours - R64| {eo:.3e} > bound {bound:.3e} (golden32 {eg:.3e})"


def check_against(model, out, counts, r64_xyz, r64_scaling, label, step=None):
    """`model` after densify_and_prune against an expected output state `out` = {name: array, "m_" + name, "v_" + name}:
    counts = (N_out, n_keep, n_clone, n_s, n_child).  Copied rows and moments bit for bit, child xyz / scaling by the rule."""
    n_out, n_keep, n_clone, n_s, n_child = (int(v) for v in counts[:5])
    first_child = n_keep + n_clone
    assert n_out == first_child + 2 * n_child
    opt = model.optimizer
    assert len(opt.param_groups) == len(NAMES)
    for group, n in zip(opt.param_groups, NAMES):
        p = group["params"][0]
        assert group["name"] == n and p is model.param(n) and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        want = torch.as_tensor(np.asarray(out[n]))
        assert tuple(p.shape) == tuple(want.shape) and p.shape[0] == n_out, (label, n, tuple(p.shape), tuple(want.shape))
        rows = slice(0, first_child) if n in ("xyz", "scaling") else slice(0, n_out)
        assert same_bits(p[rows], want[rows]), f"{label}: copied rows of {n} differ"
        st = opt.state[p]
        assert set(opt.state.keys()) == {g["params"][0] for g in opt.param_groups}
        for key, tag in (("exp_avg", "m_"), ("exp_avg_sq", "v_")):
            assert same_bits(st[key], torch.as_tensor(np.asarray(out[tag + n]))), f"{label}: {key} of {n} differs"
            assert not st[key][n_keep:].any()
        if step is not None:
            assert float(st["step"]) == float(step)
    rule(f"{label} child xyz", model._xyz.detach().cpu().numpy()[first_child:], np.asarray(out["xyz"])[first_child:], r64_xyz)
    rule(f"{label} child scaling", model._scaling.detach().cpu().numpy()[first_child:], np.asarray(out["scaling"])[first_child:], r64_scaling)
    assert tuple(model.xyz_gradient_accum.shape) == (n_out, 1) and tuple(model.denom.shape) == (n_out, 1) and tuple(model.max_radii2D.shape) == (n_out,)
    assert not model.xyz_gradient_accum.any() and not model.denom.any() and not model.max_radii2D.any()


def check_golden(model, c, label):
    out = {k[4:]: v for k, v in c.items() if k.startswith("out_")}
    check_against(model, out, c["counts"], c["r64_xyz"], c["r64_scaling"], label, step=int(c["counts"][5]))


def can_step(model):
    """The re-keyed optimizer takes a step on the new parameters."""
    gen = torch.Generator().manual_seed(5)
    before = [model.param(n).detach().clone() for n in NAMES]
    for n in NAMES:
        p = model.param(n)
        p.grad = torch.randn(p.shape, generator=gen).to(p.device)
    steps = [float(model.optimizer.state[model.param(n)]["step"]) for n in NAMES]
    model.optimizer.step()
    for n, b, s in zip(NAMES, before, steps):
        p = model.param(n)
        assert float(model.optimizer.state[p]["step"]) == s + 1
        assert p.numel() == 0 or not torch.equal(p.detach(), b), n


def harness():
    """The product's lg_math.h child formulas compiled for the CPU (without -mfma: fmaf() is the library's)."""
    import ctypes as C
    import common
    return common.build_harness("densify", headers=(common.LG_MATH_H,), flags=common.STRICT_FP, signatures={
        "h_densify_children": (None, [C.c_int] + [C.c_void_p] * 6)})


def random_case(n, deg=1, seed=0, hot=0.6, scale=(0.004, 1.2)):
    """A model state in the goldens' layout (numpy), for comparisons of the two backends on one device."""
    gen = torch.Generator().manual_seed(seed)
    lu = lambda k, lo, hi: torch.exp(torch.rand(k, generator=gen) * (math.log(hi) - math.log(lo)) + math.log(lo))      # noqa: E731
    c = {}
    for k, s in shapes(n, deg).items():
        c[f"in_{k}"] = torch.randn(s, generator=gen).numpy()
        c[f"in_m_{k}"] = (0.1 * torch.randn(s, generator=gen)).numpy()
        c[f"in_v_{k}"] = (0.01 * torch.rand(s, generator=gen)).numpy()
    c["in_scaling"] = torch.log(lu(n * 3, *scale)).reshape(n, 3).numpy()
    c["in_opacity"] = (3.0 * torch.randn(n, 1, generator=gen)).numpy()
    c["in_rotation"] = (torch.randn(n, 4, generator=gen) * lu(n, 0.2, 5.0)[:, None]).numpy()
    denom = torch.randint(0, 5, (n, 1), generator=gen).float()
    level = torch.where(torch.rand(n, 1, generator=gen) < hot, lu(n, 3.0, 40.0)[:, None], lu(n, 0.02, 0.5)[:, None]) * 0.0002
    c["in_accum"], c["in_denom"] = (level * denom).numpy(), denom.numpy()
    c["in_max_radii2D"] = (torch.rand(n, generator=gen) * 40.0).numpy()
    c["kwargs"] = dict(max_grad=0.0002, min_opacity=0.005, extent=5.0, max_screen_size=20)
    c["percent_dense"] = 0.01
    c["counts"] = np.array([0, 0, 0, 0, 0, 3, -1])
    return c


def contract_rows(model, th):
    """The contract's decisions, restated in torch ops on the model's own device (before densify_and_prune):
    (keep rows, clone rows, split-selected rows, parents whose children stay, their ranks among the split-selected rows)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=model._xyz.device)      # noqa: E731
    with torch.no_grad():
        m = torch.exp(model._scaling).max(dim=1).values
        sigma = torch.sigmoid(model._opacity).reshape(-1)
        g = (model.xyz_gradient_accum / model.denom).reshape(-1)
        g[g.isnan()] = 0.0
        gone = lambda mu: (sigma < f(th["min_opacity"])) | ((mu > f(th["thr_w"])) if th["use_extent"] else torch.zeros_like(sigma, dtype=torch.bool))   # noqa: E731
        split = (g >= f(th["thr_g"])) & (m > f(th["thr_d"]))
        clone = (g >= f(th["thr_g"])) & (m <= f(th["thr_d"]))
        keep_rows = torch.nonzero(~split & ~gone(m)).reshape(-1)
        clone_rows = torch.nonzero(clone & ~gone(m)).reshape(-1)
        split_rows = torch.nonzero(split).reshape(-1)
        ok = ~gone(m / f(SHRINK32))[split_rows]
        return keep_rows.cpu(), clone_rows.cpu(), split_rows.cpu(), split_rows[ok].cpu(), torch.arange(split_rows.numel())[ok.cpu()]


def expected_r64(c, parents, rank, n_s, noise):
    parents, rows = parents.numpy(), torch.cat([rank, n_s + rank]).numpy()
    two = lambda k: np.concatenate([c[k][parents]] * 2, axis=0)      # noqa: E731
    return child_r64(two("in_xyz"), two("in_scaling"), two("in_rotation"), np.asarray(noise)[rows])
