"""Shared by tests/test_mcmc_host.py and tests/test_gpu_mcmc.py (test infrastructure).

A float64 numpy twin of the three contracts of lightgaussian_amd.mcmc, stated the long way round -- D by the
published double loop with its binomial table, the noise as the dense Sigma v -- so that the product's closed form and factorised
update are tested against something they do not share; a seeded case builder on densify_common.Model; and the expected state after a
row movement.

Bounds.  The recomputed opacity and scaling of the HIP path and of the lg_math.h functions: |got - r64| <= 2^-23 |r64| per element --
one rounding to float32 (2^-24 relative) of a double result good to under 2^-40, with the factor two of room the rounding of the
scaling sum's float32 input leaves.  The torch backend evaluates the same formulas in float32 with pow; its own error is up to 2e-4
relative in o / D (measured against float64 over o in [0.005, 1 - 2^-20], M <= 51), so its rows are held to five times that:
|got - r64| <= 1e-3 max(1, |r64|).  Everything else -- row order, copied rows, moments -- is compared bit for bit."""
import math

import numpy as np
import torch

import densify_common as dc

MAX_COPIES = 51
EXACT = 2.0 ** -23
TORCH_TOL = 1e-3
OPACITY_HI = 1.0 - 2.0 ** -23


# ---- the twin ---------------------------------------------------------------------------------------------------------------------

def double_loop_D(x, M):
    """D = sum_{i=1..M} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1) in float64, term by term as published."""
    total = 0.0
    for i in range(1, M + 1):
        for k in range(i):
            total += math.comb(i - 1, k) * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1)
    return total


def x_of(o, M):
    return 1.0 - (1.0 - o) ** (1.0 / M)


def relocation_r64(opacity_raw, scaling_raw, cnt, min_opacity):
    """opacity' [n] and scaling' [n, 3] in float64 of rows with float32 raw opacity [n], raw scaling [n, 3], drawn cnt [n] >= 1 times."""
    op = np.asarray(opacity_raw, np.float64).reshape(-1)
    sc = np.asarray(scaling_raw, np.float64).reshape(-1, 3)
    lo = float(np.float32(min_opacity))
    out_op, out_sc = np.empty_like(op), np.empty_like(sc)
    for r, (raw, c) in enumerate(zip(op, np.asarray(cnt).reshape(-1))):
        M = min(int(c) + 1, MAX_COPIES)
        o = 1.0 / (1.0 + math.exp(-raw))
        x = x_of(o, M)
        xc = min(max(x, lo), OPACITY_HI)
        out_op[r] = math.log(xc / (1.0 - xc))
        out_sc[r] = sc[r] + math.log(o / double_loop_D(x, M))
    return out_op, out_sc


def noise_r64(xyz, scaling, rotation, opacity, noise, c, k, x0):
    """xyz + Sigma (noise g c) in float64 on float32 inputs, Sigma = (R diag(s)) (R diag(s))^T stored densely; c, k, x0 as float32 values."""
    xyz, scaling, q, z = (np.asarray(a, np.float64) for a in (xyz, scaling, rotation, noise))
    c, k, x0 = (float(np.float32(v)) for v in (c, k, x0))
    s = np.exp(scaling)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    r, x, y, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + w * w), 2 * (x * y - r * w), 2 * (x * w + r * y),
                  2 * (x * y + r * w), 1 - 2 * (x * x + w * w), 2 * (y * w - r * x),
                  2 * (x * w - r * y), 2 * (y * w + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    cov = np.einsum("nij,nkj->nik", L, L)
    sigma = 1.0 / (1.0 + np.exp(-np.asarray(opacity, np.float64).reshape(-1, 1)))
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(-k * ((1.0 - sigma) - x0)))
    return xyz + np.einsum("nij,nj->ni", cov, z * g * c)


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def case(n, deg=1, seed=0, dead=0.05):
    """A model state in densify_common's layout; about `dead` of the rows have sigmoid(opacity) <= 0.005, the rest lie well above."""
    c = dc.random_case(n, deg=deg, seed=seed)
    gen = torch.Generator().manual_seed(seed + 7)
    sigma = 0.02 + 0.97 * torch.rand(n, 1, generator=gen)
    is_dead = torch.rand(n, 1, generator=gen) < dead
    sigma = torch.where(is_dead, 0.004 * torch.rand(n, 1, generator=gen) + 0.0005, sigma)
    c["in_opacity"] = torch.log(sigma / (1 - sigma)).numpy()
    return c


def noise_case(n, seed=0):
    """Opacities spread over sigma in [0.001, 0.9], every eighth row at 0.9 itself: the gate runs from about 0.6 down to exactly 0 in
    float32 (at sigma = 0.9 the exponent is 89.5, above float32's overflow at 88.73)."""
    c = dc.random_case(n, deg=1, seed=seed)
    gen = torch.Generator().manual_seed(seed + 3)
    sigma = torch.exp(torch.rand(n, 1, generator=gen) * (math.log(0.9) - math.log(0.001)) + math.log(0.001))
    sigma[7::8] = 0.9
    c["in_opacity"] = torch.log(sigma / (1 - sigma)).numpy()
    c["noise"] = torch.randn(n, 3, generator=gen).numpy()
    return c


def hand_draws(sources, n):
    """Source rows for n draws: sources[0] once, [1] twice, [2] 50 times, [3] 51 times, [4] 200 times as far as n allows, the rest of
    the draws spread over the remaining sources, shuffled by a fixed permutation."""
    sources = [int(s) for s in sources]
    out = []
    for s, times in zip(sources, (1, 2, 50, 51, 200)):
        out += [s] * min(times, n - len(out))
    rest = sources[5:] or sources
    out += [rest[j % len(rest)] for j in range(n - len(out))]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).tolist()
    return torch.tensor([out[j] for j in perm], dtype=torch.int64)


def dead_rows(c, min_opacity=0.005):
    sigma = torch.sigmoid(torch.from_numpy(c["in_opacity"])).reshape(-1)
    return sigma <= torch.tensor(min_opacity, dtype=torch.float32)


# ---- the expected state of a row movement -----------------------------------------------------------------------------------------

def expected_state(c, dst, src, n_out, min_opacity):
    """{name: [n_out, ...] float32 rows, "m_" + name, "v_" + name} after moving rows src -> dst of case c, with "r64_opacity" /
    "r64_scaling" (float64, whole tensors) holding the twin's values at the touched rows, and "touched" (bool [n_out])."""
    dst, src = np.asarray(dst, np.int64), np.asarray(src, np.int64)
    n = c["in_xyz"].shape[0]
    cnt = np.bincount(src, minlength=n)
    rows = np.nonzero(cnt)[0]
    new_op, new_sc = relocation_r64(c["in_opacity"][rows], c["in_scaling"][rows], cnt[rows], min_opacity)
    grown = lambda a: np.concatenate([a, np.zeros((n_out - n,) + a.shape[1:], a.dtype)], axis=0)      # noqa: E731
    out = {}
    for name in dc.NAMES:
        value = grown(np.asarray(c[f"in_{name}"], np.float32))
        value[dst] = value[src]
        out[name] = value
        for tag in ("m_", "v_"):
            moment = grown(np.asarray(c[f"in_{tag}{name}"], np.float32))
            moment[rows] = 0
            moment[dst] = 0
            out[tag + name] = moment
    r64_op, r64_sc = out["opacity"].astype(np.float64), out["scaling"].astype(np.float64)
    r64_op[rows, 0], r64_sc[rows] = new_op, new_sc
    r64_op[dst], r64_sc[dst] = r64_op[src], r64_sc[src]
    touched = np.zeros(n_out, bool)
    touched[rows] = True
    touched[dst] = True
    out.update(r64_opacity=r64_op, r64_scaling=r64_sc, touched=touched, sources=rows)
    return out


def check_state(model, exp, dst, src, label, exact, step=3):
    """`model` after the movement against expected_state: everything bit for bit but opacity / scaling at the touched rows, which are
    held to the twin (exact: the 2^-23 bound, otherwise the torch backend's) and, at dst, are the bits of their source row."""
    n_out = exp["touched"].shape[0]
    opt = model.optimizer
    assert set(opt.state.keys()) == {g["params"][0] for g in opt.param_groups}
    touched = torch.from_numpy(exp["touched"])
    for group, name in zip(opt.param_groups, dc.NAMES):
        p = group["params"][0]
        assert group["name"] == name and p is model.param(name) and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        want = torch.from_numpy(exp[name])
        assert tuple(p.shape) == tuple(want.shape) and p.shape[0] == n_out, (label, name, tuple(p.shape))
        got = p.detach().cpu()
        if name in ("opacity", "scaling"):
            assert dc.same_bits(got[~touched], want[~touched]), f"{label}: untouched rows of {name} differ"
            assert dc.same_bits(got[dst], got[src]), f"{label}: copies of {name} are not their sources' bits"
            r64 = exp["r64_" + name][exp["touched"]]
            err = np.abs(got[touched].double().numpy() - r64)
            bound = EXACT * np.abs(r64) if exact else TORCH_TOL * np.maximum(1.0, np.abs(r64))
            worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
            print(f"{label} {name}: max |got - r64| {err.max() if err.size else 0.0:.3e}, worst error / bound {worst:.3f}")
            assert np.isfinite(got.numpy()).all() and worst <= 1.0, f"{label}: {name} off by {worst:.2f}x its bound"
        else:
            assert dc.same_bits(got, want), f"{label}: rows of {name} differ"
        st = opt.state[p]
        for key, tag in (("exp_avg", "m_"), ("exp_avg_sq", "v_")):
            assert dc.same_bits(st[key], torch.from_numpy(exp[tag + name])), f"{label}: {key} of {name} differs"
            assert not st[key].cpu()[touched].any()
        assert float(st["step"]) == float(step)


def harness():
    """The product's lg_math.h MCMC functions compiled for the CPU (without -mfma: fmaf() is the library's)."""
    import ctypes as C
    import common
    P = C.c_void_p
    return common.build_harness("mcmc", headers=(common.LG_MATH_H,), flags=common.STRICT_FP, signatures={
        "h_mcmc_binomial_sum": (C.c_double, [C.c_double, C.c_int]),
        "h_mcmc_relocate": (None, [C.c_int, P, P, P, C.c_float, P, P]),
        "h_mcmc_noise": (None, [C.c_int, P, P, P, P, P, C.c_float, C.c_float, C.c_float, P, P])})
