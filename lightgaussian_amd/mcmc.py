"""3DGS-MCMC (Kheradmand et al., NeurIPS 2024; gsplat's MCMCStrategy) on the device: training to a Gaussian budget.

    add_noise(model, xyz_lr, noise_lr=5e5, noise=None, k=100.0, x0=0.995, backend="hip")
        the covariance-shaped position noise after every optimizer step: ONE lg_mcmc_noise launch in place on _xyz, no host read.
    relocate(model, min_opacity=0.005, draws=None, backend="hip")
        dead rows (sigmoid(_opacity) <= min_opacity) become copies of live rows drawn in proportion to their opacity; the opacity and
        scaling of every drawn row are corrected so that the image is unchanged.  In place: lg_mcmc_plan + one lg_mcmc_rows launch.
    grow(model, cap_max, factor=1.05, draws=None, backend="hip")
        the model grows to min(cap_max, int(factor N)) rows, the new ones copies of drawn rows, by the same row movement into new tensors.
    regularizers(model, opacity_reg=0.01, scale_reg=0.01)      the paper's two mean-absolute terms, a differentiable torch scalar.
    after_step(model, iteration, xyz_lr, cap_max, ...)         the published schedule in one call.

The contract (include/lightgaussian_mcmc.h).  Noise, per row in float32:

    sigma = sigmoid(_opacity)    s = exp(_scaling)    R = R(q / |q|)    g = 1 / (1 + exp(-k ((1 - sigma) - x0)))
    xyz += R (s^2 o (R^T (noise g c)))        c = float32(noise_lr * xyz_lr), the product evaluated in double and rounded once

noise is unit normal [N, 3]; the default draw is torch.randn_like(model._xyz), so a seeded run keeps torch's stream.  A row whose
g c is exactly 0 keeps its value.  Row movement, for n pairs (dst[j], src[j]) with cnt[i] = the number of j with src[j] == i: every row
with cnt > 0 takes, with M = min(cnt + 1, 51), o = sigmoid(opacity), x = 1 - (1 - o)^(1/M),

    D = sum_{i=1..M} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)
    opacity' = logit(clamp(x, min_opacity, 1 - 2^-23))        scaling' = scaling + log(o / D)

every other parameter stays; row dst[j] of every parameter is row src[j] after that update, bit for bit; exp_avg and exp_avg_sq
are zero at every source and destination row; the optimizer's `step` is untouched.  The HIP path evaluates D in double in its
closed form; backend="torch" is the published float32 op sequence (L @ L^T and bmm for the noise, the double loop with a binomial
table for D), CPU tensors too: the fallback and the comparand.  backend="hip" falls back to it, with one warning per reason, for
parameters that are not contiguous float32 on the GPU, more than one parameter per group, N >= 2^30.
relocate keeps the nn.Parameter objects and the optimizer's state keys; grow swaps the Parameters and re-keys the state exactly as
densify.densify_and_prune does (model_rows.install; an optimizer state without Adam's moments is refused by model_rows.entries), and
xyz_gradient_accum, denom and max_radii2D, where the model has them, keep their first N rows and get zero rows behind them.  "n_sources" in the returned records is a 0-dim int64 tensor on the model's device (the number of
distinct drawn rows): reading it is the caller's choice, the calls themselves make one host read (relocate: the dead count) or none.
set_profile(True) records the launches under "mcmc_noise", "mcmc_count", "mcmc_plan", "mcmc_rows" (_lib.profile_read)."""
import ctypes as C
import math

import torch

from . import _lib, model_rows
from .model_rows import check_backend, f32 as to_f32, moments, plain_f32, rotation_matrices, warn_once      # (f32 here: ctypes c_float)

MCMC_COPY, MCMC_MOMENT, MCMC_OPACITY, MCMC_SCALING = 0, 1, 2, 3      # lg_densify_tensor.role of lg_mcmc_rows (LG_MCMC_*)
MCMC_MAX_COPIES = 51                                                 # LG_MCMC_MAX_COPIES: M = min(cnt + 1, 51)
MAX_ROWS = 1 << 30
MULTINOMIAL_MAX = 1 << 24                                            # torch.multinomial refuses more categories

# The C ABI of include/lightgaussian_mcmc.h, in header order: name -> (restype, argtypes).  tests/test_mcmc_host.py holds every
# entry against the header.
i32, i64, u32, f32, sz, vp = C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_size_t, C.c_void_p
PROTOTYPES = {
    "lg_mcmc_scratch_bytes": (sz, (i32,)),
    "lg_mcmc_noise": (C.c_int, (i32, vp, vp, vp, vp, vp, f32, f32, f32, u32, vp)),
    "lg_mcmc_plan": (C.c_int, (i32, i32, vp, vp, vp, f32, vp, u32, vp)),
    "lg_mcmc_rows": (C.c_int, (i32, i64, i32, vp, vp, vp, i32, C.POINTER(_lib.lg_densify_tensor), u32, vp)),
}

set_profile, _flags = model_rows.profile_switch()
def load():
    """The library object of _lib.load() with the prototypes of include/lightgaussian_mcmc.h set on it."""
    return _lib.bind(_lib.load(), PROTOTYPES)


# ---- position noise ---------------------------------------------------------------------------------------------------------------

def _noise_torch(model, noise, c, k, x0):
    """The published statement: build_scaling_rotation, L @ L^T, the gated noise, bmm, add_."""
    xyz = model._xyz.detach()
    L = rotation_matrices(model._rotation.detach()) * torch.exp(model._scaling.detach())[:, None, :]       # R diag(s)
    cov = L @ L.transpose(1, 2)
    sigma = torch.sigmoid(model._opacity.detach()).reshape(-1, 1)
    g = 1 / (1 + torch.exp(-k * ((1 - sigma) - x0)))
    v = noise * g * c
    xyz.add_(torch.bmm(cov, v.unsqueeze(-1)).squeeze(-1))


def _noise_ineligible(model):
    n = model._xyz.shape[0]
    if not all(plain_f32(t, True) for t in (model._xyz, model._scaling, model._rotation, model._opacity)):
        return "a parameter that is not contiguous float32 on the GPU"
    if n >= MAX_ROWS:
        return "N >= 2^30"
    return None


def add_noise(model, xyz_lr, noise_lr=5e5, noise=None, k=100.0, x0=0.995, backend="hip"):
    """_xyz += Sigma (noise g c) in place by the contract in the module docstring; xyz_lr is the current learning rate of the positions.
    noise: unit-normal float32 [N, 3] on the model's device, or None for torch.randn_like(model._xyz).  No host read."""
    check_backend(backend, "add_noise")
    xyz = model._xyz
    n = xyz.shape[0]
    if noise is None:
        noise = torch.randn_like(xyz.detach())
    elif not (torch.is_tensor(noise) and tuple(noise.shape) == (n, 3) and noise.dtype == xyz.dtype and noise.device == xyz.device):
        raise ValueError(f"add_noise: noise must be a {xyz.dtype} [{n}, 3] tensor on {xyz.device}")
    c, k, x0 = to_f32(float(noise_lr) * float(xyz_lr)), to_f32(k), to_f32(x0)
    if backend == "hip":
        why = _noise_ineligible(model)
        if why is not None:
            warn_once(model, "mcmc", "add_noise", why)
            backend = "torch"
    with torch.no_grad():
        if backend == "torch":
            _noise_torch(model, noise, c, k, x0)
            return
        if n == 0:
            return
        dev = xyz.device
        noise = noise.contiguous()
        with torch.cuda.device(dev):
            _lib.check(load().lg_mcmc_noise(n, _lib.ptr(xyz), _lib.ptr(model._scaling), _lib.ptr(model._rotation), _lib.ptr(model._opacity),
                                            _lib.ptr(noise), c, k, x0, _flags(), _lib.stream(dev)))
        torch.autograd.graph.increment_version(xyz)


# ---- row movement: relocation and growth ------------------------------------------------------------------------------------------

def _role(model, p):
    return MCMC_OPACITY if p is model._opacity else (MCMC_SCALING if p is model._scaling else MCMC_COPY)


def _rows_ineligible(model, entries, n_out):
    if any(len(g["params"]) != 1 for g in model.optimizer.param_groups):
        return "more than one parameter per group"
    if not all(plain_f32(t, True) for _, _, p, st in entries for t in [p] + moments(st)):
        return "a tensor that is not contiguous float32 on the GPU"
    if model._xyz.shape[0] >= MAX_ROWS or n_out >= (1 << 31):
        return "N >= 2^30"
    return None


_TABLE = {}


def _binomials(dev):
    """binoms[n, k] = C(n, k) for n, k < 51 in float32 (the published table)."""
    if dev not in _TABLE:
        _TABLE[dev] = torch.tensor([[float(math.comb(n, k)) for k in range(MCMC_MAX_COPIES)] for n in range(MCMC_MAX_COPIES)],
                                   dtype=torch.float32, device=dev)
    return _TABLE[dev]


def _relocation_torch(opacity_raw, scaling_raw, cnt, min_opacity):
    """opacity' and scaling' of rows drawn cnt times: the published float32 statement -- pow, the double loop over i = 1..M and
    k < i with the binomial table (the inner loop as one row operation) -- on the raw rows."""
    dev, dt = opacity_raw.device, opacity_raw.dtype
    m = torch.clamp(cnt + 1, max=MCMC_MAX_COPIES)
    o = torch.sigmoid(opacity_raw.reshape(-1))
    x = 1 - torch.pow(1 - o, 1 / m.to(dt))
    ks = torch.arange(MCMC_MAX_COPIES, device=dev)
    sign_over_root = torch.where(ks % 2 == 0, 1.0, -1.0).to(dt) / torch.sqrt((ks + 1).to(dt))
    binoms = _binomials(dev).to(dt)
    denom = torch.zeros_like(o)
    for i in range(1, (int(m.max()) if m.numel() else 0) + 1):
        live = m >= i
        row = (binoms[i - 1, :i] * sign_over_root[:i])[None, :] * torch.pow(x[:, None], (ks[:i] + 1).to(dt)[None, :])
        denom = denom + torch.where(live, row.sum(dim=1), torch.zeros_like(o))
    lo, hi = torch.tensor(min_opacity, dtype=dt, device=dev), torch.tensor(1.0 - 2.0 ** -23, dtype=dt, device=dev)
    xc = torch.minimum(torch.maximum(x, lo), hi)
    return torch.log(xc / (1 - xc)).reshape(opacity_raw.shape), scaling_raw + torch.log(o / denom)[:, None]


def _move_torch(model, entries, dst, src, n_out, min_opacity):
    """The row movement in plain torch ops.  In place when n_out == N (returns None); otherwise [(param, exp_avg, exp_avg_sq)] of n_out
    rows in the order of `entries`.  Second value: the number of distinct sources (0-dim tensor)."""
    n = model._xyz.shape[0]
    dev = model._xyz.device
    cnt = torch.bincount(src, minlength=n)
    rows = torch.nonzero(cnt).reshape(-1)
    new_opacity, new_scaling = _relocation_torch(model._opacity.detach()[rows], model._scaling.detach()[rows], cnt[rows], min_opacity)
    inplace = n_out == n
    out = []
    for _, _, p, st in entries:
        role = _role(model, p)
        tensors = [p.detach()] + moments(st)
        if not inplace:
            tensors = [torch.cat([t, torch.zeros((n_out - n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)], dim=0) for t in tensors]
        value = tensors[0]
        if role == MCMC_OPACITY:
            value[rows] = new_opacity
        elif role == MCMC_SCALING:
            value[rows] = new_scaling
        value[dst] = value[src]
        for moment in tensors[1:]:
            moment[rows] = 0
            moment[dst] = 0
        out.append(tuple(tensors) if st is not None else (value, None, None))
    return (None if inplace else out), (cnt > 0).sum()


def _move_hip(model, entries, dst, src, n_out, min_opacity):
    lib = load()
    dev = model._xyz.device
    n = model._xyz.shape[0]
    inplace = n_out == n
    dst32, src32 = dst.to(torch.int32).contiguous(), src.to(torch.int32).contiguous()
    out, rows = [], []
    with torch.cuda.device(dev):
        stream = _lib.stream(dev)
        scratch = _lib.scratch(lib.lg_mcmc_scratch_bytes(n), dev)
        _lib.check(lib.lg_mcmc_plan(n, src32.numel(), _lib.ptr(src32), _lib.ptr(model._opacity), _lib.ptr(model._scaling),
                                    to_f32(min_opacity), _lib.ptr(scratch), _flags(), stream))
        for _, _, p, st in entries:
            old = [p.detach()] + moments(st)
            new = old if inplace else [torch.empty((n_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in old]
            words = old[0][0].numel()
            roles = [_role(model, p)] + [MCMC_MOMENT] * (len(old) - 1)
            rows += [(a, b, words, role) for a, b, role in zip(old, new, roles)]
            out.append(tuple(new) if st is not None else (new[0], None, None))
        for count, table in model_rows.row_table(rows):
            _lib.check(lib.lg_mcmc_rows(n, n_out, src32.numel(), _lib.ptr(dst32), _lib.ptr(src32), _lib.ptr(scratch), count, table,
                                        _flags(), stream))
        if inplace:
            torch.autograd.graph.increment_version([a for a, _, _, _ in rows])
        n_sources = (scratch[:4 * n].view(torch.int32) > 0).sum()
    return (None if inplace else out), n_sources


def _move(model, entries, dst, src, n_out, min_opacity, backend, what):
    if backend == "hip":
        why = _rows_ineligible(model, entries, n_out)
        if why is not None:
            warn_once(model, "mcmc", what, why)
            backend = "torch"
    with torch.no_grad():
        new, n_sources = (_move_hip if backend == "hip" else _move_torch)(model, entries, dst, src, n_out, min_opacity)
    return new, n_sources, backend


def _draw(weights, n):
    """n draws with replacement in proportion to `weights` (1-D, >= 0): torch.multinomial, and above its 2^24 categories the inverse
    CDF (a float64 cumsum, searchsorted on torch.rand)."""
    if weights.numel() <= MULTINOMIAL_MAX:
        return torch.multinomial(weights, n, replacement=True)
    cdf = torch.cumsum(weights.to(torch.float64), dim=0)
    u = torch.rand(n, dtype=torch.float64, device=weights.device) * cdf[-1]
    return torch.clamp(torch.searchsorted(cdf, u, right=True), max=weights.numel() - 1)


def _check_draws(draws, n, rows, dev, what, live=None):
    if not (torch.is_tensor(draws) and draws.dtype == torch.int64 and tuple(draws.shape) == (n,) and draws.device == dev):
        raise ValueError(f"{what}: draws must be an int64 [{n}] tensor on {dev}")
    if n > 0 and not bool(((draws >= 0) & (draws < rows)).all()):
        raise ValueError(f"{what}: draws outside [0, {rows})")
    if n > 0 and live is not None and not bool(live[draws].all()):
        raise ValueError(f"{what}: every drawn source must be a live row (sigmoid(_opacity) > min_opacity)")
    return draws


def relocate(model, min_opacity=0.005, draws=None, backend="hip"):
    """Dead rows (sigmoid(_opacity) <= min_opacity) become copies of live rows, in place, by the contract in the module docstring.
    draws: int64 [n_dead] of live source rows, one per dead row in ascending order of the dead rows, or None for
    torch.multinomial(sigma[alive], n_dead, replacement=True) mapped back through the alive indices.
    Returns {"n_dead", "n_sources", "backend"}; with no dead or no live row nothing is launched."""
    check_backend(backend, "relocate")
    entries = model_rows.entries(model, "relocate")
    n = model._xyz.shape[0]
    dev = model._xyz.device
    with torch.no_grad():
        sigma = torch.sigmoid(model._opacity.detach()).reshape(-1)
        dead = sigma <= to_f32(min_opacity)                                 # (a Python scalar: no copy to the device)
        order = torch.argsort(dead.to(torch.uint8), stable=True)           # the live rows ascending, then the dead rows ascending
        n_dead = int(dead.sum().item())                                     # the one host read of the call
        alive, dst = order[:n - n_dead], order[n - n_dead:]
        if n_dead == 0 or n_dead == n:
            return dict(n_dead=n_dead, n_sources=torch.zeros((), dtype=torch.int64, device=dev), backend=backend)
        src = alive[_draw(sigma[alive], n_dead)] if draws is None else _check_draws(draws, n_dead, n, dev, "relocate", live=~dead)
    _, n_sources, backend = _move(model, entries, dst, src, n, min_opacity, backend, "relocate")
    return dict(n_dead=n_dead, n_sources=n_sources, backend=backend)


def grow(model, cap_max, factor=1.05, draws=None, backend="hip", *, min_opacity=0.005):
    """The model grows by n = max(0, min(cap_max, int(factor N)) - N) rows, copies of rows drawn in proportion to their opacity, by the
    contract in the module docstring (min_opacity: the floor of the corrected opacities).  draws: int64 [n] of source rows, or None for
    torch.multinomial(sigma, n, replacement=True).  New tensors of N + n rows: Parameters swapped, the optimizer's state re-keyed.
    Returns {"N_out", "n_new", "n_sources", "backend"}."""
    check_backend(backend, "grow")
    entries = model_rows.entries(model, "grow")
    n = model._xyz.shape[0]
    dev = model._xyz.device
    n_new = max(0, min(int(cap_max), int(factor * n)) - n)
    if draws is not None:
        _check_draws(draws, n_new, n, dev, "grow")
    if n_new == 0:
        return dict(N_out=n, n_new=0, n_sources=torch.zeros((), dtype=torch.int64, device=dev), backend=backend)
    with torch.no_grad():
        src = _draw(torch.sigmoid(model._opacity.detach()).reshape(-1), n_new) if draws is None else draws
        dst = torch.arange(n, n + n_new, dtype=torch.int64, device=dev)
    new, n_sources, backend = _move(model, entries, dst, src, n + n_new, min_opacity, backend, "grow")
    book = {name: getattr(model, name, None) for name in model_rows.BOOK}
    book = {name: torch.cat([old, torch.zeros((n_new,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)], dim=0)
            for name, old in book.items() if torch.is_tensor(old) and old.shape[0] == n}
    model_rows.install(model, entries, new, book=book)
    return dict(N_out=n + n_new, n_new=n_new, n_sources=n_sources, backend=backend)


# ---- the rest of the method -------------------------------------------------------------------------------------------------------

def regularizers(model, opacity_reg=0.01, scale_reg=0.01):
    """opacity_reg * mean |sigmoid(_opacity)| + scale_reg * mean |exp(_scaling)|: add it to the loss."""
    return opacity_reg * torch.abs(torch.sigmoid(model._opacity)).mean() + scale_reg * torch.abs(torch.exp(model._scaling)).mean()


def after_step(model, iteration, xyz_lr, cap_max, *, start=500, stop=25_000, every=100, min_opacity=0.005, factor=1.05, noise_lr=5e5,
               k=100.0, x0=0.995, backend="hip"):
    """The published schedule, to be called after optimizer.step(): relocate and grow when start < iteration < stop and
    iteration % every == 0, and always add_noise.  Returns {"relocate": record or None, "grow": record or None}.
    Data-parallel runs (dp.wrap_optimizer) are refused: every rank would need the same draws."""
    if getattr(model.optimizer, "_lg_dp_wrapped", False):
        raise RuntimeError("mcmc.after_step: the optimizer is wrapped for data-parallel training; the ranks would draw differently and diverge")
    done = {"relocate": None, "grow": None}
    if start < iteration < stop and iteration % every == 0:
        done["relocate"] = relocate(model, min_opacity=min_opacity, backend=backend)
        done["grow"] = grow(model, cap_max, factor=factor, min_opacity=min_opacity, backend=backend)
    add_noise(model, xyz_lr, noise_lr=noise_lr, k=k, x0=x0, backend=backend)
    return done
