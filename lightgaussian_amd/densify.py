"""Densification of train_densify_prune.py on the device: the per-iteration view statistics and densify_and_prune.

    accumulate_stats(model, viewspace_points, update_filter, radii=None)
        GaussianModel.add_densification_stats (scene/gaussian_model.py:784-788) and, with `radii`, the trainer's own max_radii2D
        statement (train_densify_prune.py:172-174): ONE lg_densify_stats launch, no compaction, no host read.  The reference runs
        four boolean-mask statements, each with a nonzero() and a host sync.
    densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, noise=None, backend="hip")
        GaussianModel.densify_and_prune (:745-761, with densify_and_clone / densify_and_split / densification_postfix /
        cat_tensors_to_optimizer / prune_points behind it) as ONE pass: lg_densify_plan classifies every row and maps every output
        row to its source, lg_densify_rows writes every tensor of the new model in one launch.  One device-to-host read per call:
        the record {N_out, n_keep, n_clone, n_s, n_child}, which sizes the noise and the outputs.

The contract.  Thresholds are evaluated in double and rounded ONCE to float32: thr_g = max_grad, thr_d =
percent_dense * extent, thr_w = 0.1 * extent, min_opacity; the split divisor is float32(0.8 * 2).  Per row, s = exp(_scaling),
m = max s, sigma = sigmoid(_opacity), g = xyz_gradient_accum / denom with NaN -> 0:

    clone = g >= thr_g and m <= thr_d        split = g >= thr_g and m > thr_d
    pruned(sigma, mu) = sigma < min_opacity or (max_screen_size truthy and mu > thr_w)

The reference's third prune term, max_radii2D > max_screen_size, never fires: densification_postfix has zeroed max_radii2D for
every row by the time it is looked at (:662-664).  We follow the reference: max_screen_size only switches the world-space test on.
Output rows, in this order: (1) originals that are not split and not pruned(sigma, m), with their Adam moments; (2) clones of the
rows with `clone` that are not pruned, raw rows bit for bit, moments zero; (3) first and (4) second children of the split rows
that are not pruned(sigma, m / 1.6) -- each group in the original order.  The k-th split row (k counts ALL of them, n_s in total)
uses noise[k] for its first and noise[n_s + k] for its second child:

    xyz_child = R(q / |q|) (noise * s) + xyz        scaling_child = log(s / 1.6)        everything else copied, moments zero

xyz_gradient_accum, denom and max_radii2D are zero for all output rows; the optimizer's `step` is untouched.  noise is unit normal
[2 n_s, 3]; the default draw is torch.normal(zeros, ones) of that shape on the model's device -- the reference's
torch.normal(mean=zeros, std=stds) is normal_(0, 1) * std + mean, so a seeded trainer keeps its random stream.  The reference's two
torch.cuda.empty_cache() calls are not made.

backend="torch" is the same contract in plain torch ops (CPU tensors too): the fallback and the comparand.  backend="hip" falls
back to it, with one warning per reason, for: thr_g <= 0, parameters that are not float32 on the GPU, more than one parameter per
group, N >= 2^30.  The optimizer surgery is model_rows.install's, as for prune.prune_points and mcmc.grow: new nn.Parameters, the
state objects moved to them; an optimizer state without Adam's moments is refused (model_rows.entries).
set_profile(True) records the launches under "densify_stats", "densify_plan", "densify_rows" (_lib.profile_read)."""
import torch

from . import _lib, model_rows
from .model_rows import f32, plain_f32, warn_once

SHRINK = 0.8 * 2
MAX_ROWS = 1 << 30
set_profile, _flags = model_rows.profile_switch()


def thresholds(model, max_grad, min_opacity, extent, max_screen_size):
    return dict(thr_g=f32(max_grad), thr_d=f32(float(model.percent_dense) * float(extent)), thr_w=f32(0.1 * float(extent)),
                min_opacity=f32(min_opacity), use_extent=bool(max_screen_size))


# ---- view statistics --------------------------------------------------------------------------------------------------------------

def _stats_ineligible(model, grad, update_filter, radii):
    accum, denom = model.xyz_gradient_accum, model.denom
    n = accum.shape[0]
    if not (plain_f32(accum) and plain_f32(denom) and plain_f32(grad)):
        return "a tensor that is not float32 on the GPU"
    if not (accum.is_contiguous() and denom.is_contiguous() and accum.numel() == n and denom.numel() == n):
        return "a non-contiguous statistics tensor"
    if tuple(grad.shape) != (n, 3) or not grad.is_contiguous():
        return "a viewspace gradient that is not a contiguous [N, 3]"
    if not (torch.is_tensor(update_filter) and update_filter.is_cuda and update_filter.dtype in (torch.bool, torch.uint8)
            and update_filter.numel() == n and update_filter.is_contiguous()):
        return "an update filter that is not a contiguous bool / uint8 [N] on the GPU"
    if radii is not None:
        mr = model.max_radii2D
        if not (plain_f32(mr) and mr.is_contiguous() and mr.numel() == n):
            return "a max_radii2D that is not a contiguous float32 [N] on the GPU"
        if not (torch.is_tensor(radii) and radii.is_cuda and radii.dtype == torch.int32 and radii.numel() == n and radii.is_contiguous()):
            return "radii that are not a contiguous int32 [N] on the GPU"
    if n >= MAX_ROWS:
        return "N >= 2^30"
    return None


def accumulate_stats(model, viewspace_points, update_filter, radii=None, absgrad=False):
    """xyz_gradient_accum[f] += |viewspace_points.grad[f, :2]|, denom[f] += 1 and, with radii, max_radii2D[f] = max(max_radii2D[f],
    radii[f]) for f = update_filter, in place.  No host read on either path.
    absgrad=True: the norm is taken of viewspace_points.absgrad instead -- the absolute mean gradients a render with option absgrad
    leaves there (rasterizer.set_option; same [N,3] layout, so the same lg_densify_stats launch) -- ValueError when it is absent."""
    if absgrad:
        grad = getattr(viewspace_points, "absgrad", None)
        if grad is None:
            raise ValueError("accumulate_stats(absgrad=True): viewspace_points carries no .absgrad (render with option absgrad, "
                             "call it after backward())")
    else:
        grad = viewspace_points.grad
        if grad is None:
            raise ValueError("accumulate_stats: viewspace_points carries no gradient (call it after backward())")
    with torch.no_grad():
        why = _stats_ineligible(model, grad, update_filter, radii)
        if why is not None:
            if grad.is_cuda:
                warn_once(model, "densify", "accumulate_stats", why)
            f = update_filter.reshape(-1).bool()
            accum, denom = model.xyz_gradient_accum, model.denom
            length = torch.linalg.vector_norm(grad[:, :2], dim=-1).reshape(accum.shape)
            accum.add_(torch.where(f.reshape(accum.shape), length, torch.zeros_like(length)))
            denom.add_(f.reshape(denom.shape).to(denom.dtype))
            if radii is not None:
                mr = model.max_radii2D
                mr.copy_(torch.where(f, torch.maximum(mr, radii.reshape(-1).to(mr.dtype)), mr))
            return
        n = model.xyz_gradient_accum.shape[0]
        dev = grad.device
        mr = model.max_radii2D if radii is not None else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().lg_densify_stats(n, _lib.ptr(grad), _lib.ptr(update_filter), _lib.ptr(radii), _lib.ptr(mr),
                                                    _lib.ptr(model.xyz_gradient_accum), _lib.ptr(model.denom), _flags(), _lib.stream(dev)))
        torch.autograd.graph.increment_version([model.xyz_gradient_accum, model.denom] + ([mr] if mr is not None else []))


# ---- densify_and_prune ------------------------------------------------------------------------------------------------------------

def _ineligible(model, th, entries):
    if not th["thr_g"] > 0.0:
        return "max_grad <= 0"
    if any(len(g["params"]) != 1 for g in model.optimizer.param_groups):
        return "more than one parameter per group"
    tensors = _bookkeeping(model)
    for _, _, p, st in entries:
        tensors += [p] + model_rows.moments(st)
    if not all(plain_f32(t) for t in tensors):
        return "a tensor that is not float32 on the GPU"
    if model._xyz.shape[0] >= MAX_ROWS:
        return "N >= 2^30"
    return None


def _check_noise(noise, n_s, dev):
    if not (torch.is_tensor(noise) and tuple(noise.shape) == (2 * n_s, 3) and noise.dtype == torch.float32 and noise.device == dev):
        raise ValueError(f"densify_and_prune: noise must be a float32 [{2 * n_s}, 3] tensor on {dev} (2 rows per split-selected Gaussian)")
    return noise.contiguous()


def _draw_noise(n_s, dev):
    # the reference's torch.normal(mean=zeros, std=stds) consumes the generator exactly like this draw of the same shape
    return torch.normal(mean=torch.zeros((2 * n_s, 3), device=dev), std=torch.ones((2 * n_s, 3), device=dev))


def _bookkeeping(model):
    return [getattr(model, name) for name in model_rows.BOOK]


def _role(model, p):
    return _lib.DENSIFY_XYZ if p is model._xyz else (_lib.DENSIFY_SCALING if p is model._scaling else _lib.DENSIFY_COPY)


def _rows_torch(model, th, entries, noise):
    """The contract in plain torch ops.  Returns ([(param, exp_avg, exp_avg_sq)] in the order of `entries`, the counts, the zeroed
    bookkeeping tensors)."""
    dev = model._xyz.device
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)          # noqa: E731 -- 0-dim: does not promote a float32 tensor
    xyz, raw_s, raw_q = model._xyz.detach(), model._scaling.detach(), model._rotation.detach()
    s = torch.exp(raw_s)
    m = s.max(dim=1).values
    sigma = torch.sigmoid(model._opacity.detach()).reshape(-1)
    g = (model.xyz_gradient_accum / model.denom).reshape(-1)
    g = torch.where(g.isnan(), torch.zeros_like(g), g)

    def pruned(sig, mu):
        out = sig < t(th["min_opacity"])
        return (out | (mu > t(th["thr_w"]))) if th["use_extent"] else out

    hot = g >= t(th["thr_g"])
    split = hot & (m > t(th["thr_d"]))
    clone = hot & (m <= t(th["thr_d"]))
    stays = ~pruned(sigma, m)
    keep_rows = torch.nonzero(~split & stays).reshape(-1)
    clone_rows = torch.nonzero(clone & stays).reshape(-1)
    split_rows = torch.nonzero(split).reshape(-1)
    n_s = split_rows.numel()
    child_stays = ~pruned(sigma, m / t(f32(SHRINK)))[split_rows]
    parents = split_rows[child_stays]
    rank = torch.arange(n_s, device=dev)[child_stays]
    noise = _draw_noise(n_s, dev).to(xyz.dtype) if noise is None else _check_noise(noise, n_s, dev)

    rot = model_rows.rotation_matrices(raw_q[parents])
    child_xyz = [torch.bmm(rot, (noise[rows] * s[parents]).unsqueeze(-1)).squeeze(-1) + xyz[parents] for rows in (rank, n_s + rank)]
    child_scaling = torch.log(s[parents] / t(f32(SHRINK)))
    n_new = clone_rows.numel() + 2 * parents.numel()
    out = []
    for _, _, p, st in entries:
        src = p.detach()
        role = _role(model, p)
        kids = child_xyz if role == _lib.DENSIFY_XYZ else ([child_scaling] * 2 if role == _lib.DENSIFY_SCALING else [src[parents]] * 2)
        new_p = torch.cat([src[keep_rows], src[clone_rows]] + kids, dim=0)
        moments = [None, None]
        if st is not None:
            moments = [torch.cat([st[key][keep_rows], torch.zeros((n_new,) + tuple(src.shape[1:]), dtype=st[key].dtype, device=dev)], dim=0)
                       for key in ("exp_avg", "exp_avg_sq")]
        out.append((new_p, moments[0], moments[1]))
    n_out = keep_rows.numel() + n_new
    counts = dict(N_out=n_out, n_keep=keep_rows.numel(), n_clone=clone_rows.numel(), n_s=n_s, n_child=parents.numel())
    return out, counts, [torch.zeros((n_out,) + tuple(old.shape[1:]), dtype=old.dtype, device=dev) for old in _bookkeeping(model)]


def _rows_hip(model, th, entries, noise):
    lib = _lib.load()
    dev = model._xyz.device
    n = model._xyz.shape[0]
    raw_s, raw_q = model._scaling.detach().contiguous(), model._rotation.detach().contiguous()
    opacity = model._opacity.detach().contiguous()
    accum, denom = model.xyz_gradient_accum.contiguous(), model.denom.contiguous()
    with torch.cuda.device(dev):
        stream = _lib.stream(dev)
        table_map = torch.empty((2 * max(n, 1), 2), dtype=torch.int32, device=dev)
        record = torch.empty(8, dtype=torch.int32, device=dev)
        scratch = _lib.scratch(lib.lg_densify_scratch_bytes(n), dev)
        _lib.check(lib.lg_densify_plan(n, _lib.ptr(raw_s), _lib.ptr(opacity), _lib.ptr(accum), _lib.ptr(denom), th["thr_g"], th["thr_d"],
                                       th["thr_w"], th["min_opacity"], int(th["use_extent"]), _lib.ptr(table_map), _lib.ptr(record),
                                       _lib.ptr(scratch), _flags(), stream))
        n_out, n_keep, n_clone, n_s, n_child = record.cpu().tolist()[:5]          # the one host read of the call
        noise = _draw_noise(n_s, dev) if noise is None else _check_noise(noise, n_s, dev)
        out, rows = [], []
        for _, _, p, st in entries:
            src = p.detach().contiguous()
            words = src[0].numel() if n > 0 else 0
            new = [torch.empty((n_out,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)]
            rows.append((src, new[0], words, _role(model, p)))
            for key in ("exp_avg", "exp_avg_sq") if st is not None else ():
                new.append(torch.empty_like(new[0]))
                rows.append((st[key].contiguous(), new[-1], words, _lib.DENSIFY_MOMENT))
            out.append(tuple(new) if st is not None else (new[0], None, None))
        book = [torch.empty((n_out,) + tuple(old.shape[1:]), dtype=old.dtype, device=dev) for old in _bookkeeping(model)]
        if n_out > 0:
            rows += [(None, b, b[0].numel(), _lib.DENSIFY_ZERO) for b in book]
            for count, table in model_rows.row_table(rows):
                _lib.check(lib.lg_densify_rows(n, n_out, _lib.ptr(table_map), _lib.ptr(record), count, table, _lib.ptr(raw_q), _lib.ptr(raw_s),
                                               _lib.ptr(noise) if n_s > 0 else None, 2 * n_s, _flags(), stream))
    return out, dict(N_out=n_out, n_keep=n_keep, n_clone=n_clone, n_s=n_s, n_child=n_child), book


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, noise=None, backend="hip"):
    """GaussianModel.densify_and_prune(max_grad, min_opacity, extent, max_screen_size) on `model` (a reference GaussianModel or anything
    with its attributes: optimizer, _xyz ... _rotation, percent_dense, xyz_gradient_accum, denom, max_radii2D), by the contract in the
    module docstring.  noise: unit-normal float32 [2 n_s, 3] on the model's device, or None for the default draw.
    Returns the record {"N_out", "n_keep", "n_clone", "n_s", "n_child", "backend"}."""
    model_rows.check_backend(backend, "densify_and_prune")
    th = thresholds(model, max_grad, min_opacity, extent, max_screen_size)
    entries = model_rows.entries(model, "densify_and_prune")
    if backend == "hip":
        why = _ineligible(model, th, entries)
        if why is not None:
            warn_once(model, "densify", "densify_and_prune", why)
            backend = "torch"
    with torch.no_grad():
        new, counts, zeros = (_rows_hip if backend == "hip" else _rows_torch)(model, th, entries, noise)
    model_rows.install(model, entries, new, book=dict(zip(model_rows.BOOK, zeros)))
    return dict(counts, backend=backend)
