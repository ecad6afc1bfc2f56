"""Row surgery on a model and its optimizer: the host-side plumbing under every feature that changes the number or the identity of
a model's rows -- prune.prune_points, densify.densify_and_prune, mcmc.relocate / mcmc.grow.

    entries(model, what)                 [(group, j, parameter, state or None)] over every parameter of model.optimizer, checked
    install(model, entries, new, book)   the new tensors become the model's Parameters; the optimizer's state objects move to them
    row_table(rows)                      (count, lg_densify_tensor table) per chunk of at most LG_DENSIFY_MAX_TENSORS tensors

and the small helpers those features share.  No state of its own: profile_switch() hands every module its own switch."""
import warnings

import torch
from torch import nn

from . import _lib

ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
BOOK = ("xyz_gradient_accum", "denom", "max_radii2D")


def profile_switch():
    """(set_profile, flags) of one module: a switch of its own, and LG_FLAG_PROFILE or 0 by it."""
    on = [False]

    def set_profile(value):
        """LG_FLAG_PROFILE on every library call of this module (_lib.profile_read)."""
        on[0] = bool(value)

    return set_profile, lambda: _lib.profile_flag(on[0])


def warn_once(model, module, what, reason):
    """One warning per model, entry point and reason."""
    seen = model.__dict__.setdefault("_lg_rows_warned", set())
    if (module, what, reason) not in seen:
        seen.add((module, what, reason))
        warnings.warn(f"lightgaussian_amd.{module}.{what}: {reason} is outside the HIP path; taking the torch path", stacklevel=3)


def check_backend(backend, what):
    if backend not in ("hip", "torch"):
        raise ValueError(f"{what}: unknown backend {backend!r} (hip | torch)")


def f32(x):
    """A Python / numpy scalar evaluated in double, rounded once to float32 (what a float32 tensor compared with it sees)."""
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32).item()


def plain_f32(t, contiguous=False):
    return (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided
            and (not contiguous or t.is_contiguous()))


def rotation_matrices(raw_q):
    """build_rotation: R(q / |q|), q = (r, x, y, z), [n, 3, 3]."""
    q = raw_q / torch.sqrt(raw_q[:, 0] * raw_q[:, 0] + raw_q[:, 1] * raw_q[:, 1] + raw_q[:, 2] * raw_q[:, 2] + raw_q[:, 3] * raw_q[:, 3])[:, None]
    r, x, y, z = q.unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def moments(state):
    """[exp_avg, exp_avg_sq] of an entry's state, [] for None."""
    return [] if state is None else [state["exp_avg"], state["exp_avg_sq"]]


def entries(model, what, n=None):
    """[(group, index in the group, parameter, its optimizer state or None)] over every parameter of model.optimizer.  A missing or
    empty state is None.  ValueError, before anything is touched, for a parameter that does not have one row per Gaussian (n rows:
    model._xyz's, unless the caller knows them otherwise) and for a state that holds something but not both Adam moments: its rows
    could not follow the parameter's."""
    opt = model.optimizer
    n = model._xyz.shape[0] if n is None else n
    out = []
    for group in opt.param_groups:
        for j, p in enumerate(group["params"]):
            if p.shape[0] != n:
                raise ValueError(f"{what}: every parameter of the optimizer must have one row per Gaussian")
            st = opt.state.get(p, None) or None
            if st is not None and not ("exp_avg" in st and "exp_avg_sq" in st):
                raise ValueError(f"{what}: the optimizer state of group {group.get('name')!r} holds {sorted(st)} without exp_avg / exp_avg_sq; "
                                 "only Adam-family state can follow its rows")
            out.append((group, j, p, st))
    return out


def install(model, entries, new, book=None):
    """`new` = [(parameter tensor, exp_avg, exp_avg_sq)] in the order of `entries` (the moments unused where the entry has no state).
    Every tensor becomes an nn.Parameter in its group's place; the entry's state object -- the same dict, so `step` and whatever else
    it holds stay -- gets the new moments and moves to the new key; the first parameter of a group named in ATTR is bound to the
    model's attribute; `book` = {name: tensor} sets the bookkeeping attributes.  Returns {group name: its first Parameter}."""
    opt = model.optimizer
    named = {}
    for (group, j, p, st), (tensor, exp_avg, exp_avg_sq) in zip(entries, new):
        param = nn.Parameter(tensor.requires_grad_(True))
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = exp_avg, exp_avg_sq
            del opt.state[p]
            opt.state[param] = st
        group["params"][j] = param
        if j == 0 and "name" in group:
            named[group["name"]] = param
            if group["name"] in ATTR:
                setattr(model, ATTR[group["name"]], param)
    for name, tensor in (book or {}).items():
        setattr(model, name, tensor)
    return named


def row_table(rows):
    """rows = [(src tensor or None, dst tensor, words per row, role)].  Yields (count, lg_densify_tensor table) per chunk of at most
    LG_DENSIFY_MAX_TENSORS; rows of zero words ([N, 0, 3]) have nothing to write and are left out."""
    rows = [r for r in rows if r[2] > 0]
    for lo in range(0, len(rows), _lib.DENSIFY_MAX_TENSORS):
        part = rows[lo:lo + _lib.DENSIFY_MAX_TENSORS]
        table = (_lib.lg_densify_tensor * len(part))()
        for row, (src, dst, words, role) in zip(table, part):
            row.src, row.dst, row.row_words, row.role = None if src is None else src.data_ptr(), dst.data_ptr(), words, role
        yield len(part), table
