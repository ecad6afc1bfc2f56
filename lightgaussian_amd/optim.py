"""HipAdam / HipAdamW: torch.optim.Adam / AdamW whose step() is ONE lg_adam_step launch over all parameter tensors.

The reference builds torch.optim.AdamW(l, lr=0.0, eps=1e-15) over six one-tensor groups with an lr each (scene/gaussian_model.py
training_setup), rewrites the xyz group's lr every iteration and reaches the moments by key (exp_avg, exp_avg_sq) from its prune /
densify surgery.  These classes ARE torch's classes (isinstance holds, param_groups / state / state_dict / hooks are torch's own)
with step() replaced:

    state       exactly what torch's default, non-fused Adam keeps: `step` a CPU float32 scalar tensor, exp_avg / exp_avg_sq from
                zeros_like(p, memory_format=preserve_format), created at the first step that sees a gradient -- a state_dict()
                loads into torch's default Adam / AdamW and back
    one step    every parameter with a gradient, its group's lr / betas / eps / weight_decay / decoupled flag as they stand at that
                moment -> one lg_adam_step call per distinct (device, betas, eps, decoupled); a parameter without a gradient is
                skipped as in torch (no state, no bits change, its step does not advance)
    afterwards  torch.autograd.graph.increment_version on every tensor written through its raw pointer (param, exp_avg,
                exp_avg_sq): autograd's in-place check and TrainableCompressed's _rows._version resync keep seeing the update
    ineligible  amsgrad / maximize / capturable / differentiable, a tensor lr, a non-float32, sparse or non-contiguous parameter,
                gradient or moment: torch's own step, unchanged, and one warning per optimizer that names the reason
    CPU         raises: there is no CPU fallback
    visible=    step(visible=mask), opt-in: ONE lg_adam_step_rows launch that steps only the rows a view saw.  `mask` is a contiguous
                bool / uint8 CUDA tensor [N] (render()'s visibility_filter; the union of several views is `a.clone() | b`), read in
                place.  Every parameter with a gradient and shape[0] == N is masked, all others are dense entries of the same launch
                (no parameter with N rows: ValueError).  A row whose byte is non-zero takes exactly the dense arithmetic, bias
                correction by the tensor's own step count, which advances once per call as always; a row whose byte is zero keeps
                the bits of param, exp_avg and exp_avg_sq -- no moment decay, no weight decay in either form, its gradient never
                read.  This is NOT dense Adam, where an unseen row coasts on its momentum.  State, hooks, version counters and
                state_dict are those of the dense step.  An ineligible configuration raises RuntimeError here: torch's dense step
                is never taken silently in place of a masked one.

hip_step_class(cls) / convert(opt) make the HIP-stepping subclass of any Adam subclass (run.hip_adam uses them on the optimizers
the unmodified trainers construct).  set_profile(True) records the launches under "adam" ("adam_rows" for step(visible=);
_lib.profile_read)."""
import warnings

import torch

from . import _lib, model_rows

MAX_TENSORS = _lib.ADAM_MAX_TENSORS
SPAN = _lib.ADAM_SPAN
set_profile, _profile_flag = model_rows.profile_switch()      # one "adam" / "adam_rows" entry per launch in _lib.profile_read()
_CLASSES = {}


def _torch_step(cls):
    """cls.step without Optimizer.profile_hook_step's wrapper (the hooks run once, around OUR step)."""
    f = cls.step
    while getattr(f, "hooked", False) and hasattr(f, "__wrapped__"):
        f = f.__wrapped__
    return f


def _flat_params(opt):
    return [p for g in opt.param_groups for p in g["params"]]


def _refuse_cpu(params):
    for p in params:
        if not p.is_cuda:
            raise RuntimeError("HipAdam / HipAdamW step through lg_adam_step on the MI355X only (no CPU fallback): "
                               f"a parameter lives on {p.device}; use torch.optim.Adam / AdamW for it")


def _ineligible_group(group):
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        if group.get(flag):
            return f"{flag}=True"
    if torch.is_tensor(group["lr"]):
        return "a tensor lr"
    if any(torch.is_tensor(b) for b in group["betas"]):
        return "tensor betas"
    return None


def _ineligible_tensor(t, what):
    if t.is_sparse or t.layout != torch.strided:
        return f"a sparse {what}"
    if t.dtype != torch.float32:
        return f"a {str(t.dtype).replace('torch.', '')} {what}"
    if not t.is_contiguous():
        return f"a non-contiguous {what}"
    return None


def _check_visible(visible):
    """Why `visible` cannot be the row mask of lg_adam_step_rows, or None."""
    if not torch.is_tensor(visible):
        return f"visible must be a tensor, not {type(visible).__name__}"
    if visible.dtype not in (torch.bool, torch.uint8):
        return f"a {str(visible.dtype).replace('torch.', '')} mask (bool or uint8: one byte per row)"
    if visible.dim() != 1:
        return f"a {visible.dim()}-D mask (one byte per row: [N])"
    if not visible.is_cuda:
        return f"a mask on {visible.device}"
    if not visible.is_contiguous():
        return "a non-contiguous mask"
    return None


class _HipStep:
    """Mix-in in front of torch.optim.Adam (or a subclass of it): step() through lg_adam_step; step(visible=) through lg_adam_step_rows."""

    def _lg_fallback(self, reason, closure):
        if not self.__dict__.get("_lg_warned", False):
            self.__dict__["_lg_warned"] = True
            warnings.warn(f"{type(self).__name__}: {reason} is outside lg_adam_step; this optimizer takes torch's own step", stacklevel=3)
        base = next(c for c in type(self).__mro__ if "step" in c.__dict__ and not issubclass(c, _HipStep))
        return _torch_step(base)(self, closure)

    def _lg_ineligible(self, why, closure, visible):
        if visible is not None:
            raise RuntimeError(f"{type(self).__name__}.step(visible=): {why} is outside lg_adam_step_rows, and torch's dense step is not "
                               "taken in place of a masked one")
        return self._lg_fallback(why, closure)

    def step(self, closure=None, *, visible=None):
        _refuse_cpu(_flat_params(self))
        if visible is not None:
            why = _check_visible(visible)
            if why is not None:
                raise RuntimeError(f"{type(self).__name__}.step(visible=): {why}")
            rows = visible.shape[0]
            if not any(p.grad is not None and p.dim() >= 1 and p.shape[0] == rows for p in _flat_params(self)):
                raise ValueError(f"{type(self).__name__}.step(visible=): the mask has {rows} rows and no parameter with a gradient has "
                                 f"{rows} as its leading dimension")
        for group in self.param_groups:
            why = _ineligible_group(group)
            if why is not None:
                return self._lg_ineligible(why, closure, visible)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                why = _ineligible_tensor(p, "parameter") or _ineligible_tensor(p.grad, "gradient")
                if why is None and len(state) != 0:
                    why = _ineligible_tensor(state["exp_avg"], "exp_avg") or _ineligible_tensor(state["exp_avg_sq"], "exp_avg_sq")
                    if why is None and not (state["exp_avg"].device == p.device and state["exp_avg_sq"].device == p.device):
                        why = "a moment on another device"
                if why is None and p.grad.device != p.device:
                    why = "a gradient on another device"
                if why is None and visible is not None and p.dim() >= 1 and p.shape[0] == visible.shape[0] and p.device != visible.device:
                    why = f"a mask on {visible.device} for a parameter on {p.device}"
                if why is not None:
                    self._lg_ineligible(why, None, visible)  # (the closure has run)
                    return loss
                work.append((group, p))
        if not work:
            return loss
        calls = {}
        with torch.no_grad():
            for group, p in work:
                state = self.state[p]
                if len(state) == 0:                          # torch's lazy state of the default path (Adam._init_group)
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                beta1, beta2 = group["betas"]
                decoupled = bool(group.get("decoupled_weight_decay", False))
                key = (p.device.index, float(beta1), float(beta2), float(group["eps"]), decoupled)
                calls.setdefault(key, []).append((p, p.grad, state["exp_avg"], state["exp_avg_sq"], float(group["lr"]),
                                                  float(group["weight_decay"]), int(state["step"].item())))
        lib = _lib.load()
        for (index, beta1, beta2, eps, decoupled), entries in calls.items():
            table = ((_lib.lg_adam_tensor if visible is None else _lib.lg_adam_rows_tensor) * len(entries))()
            for entry, (p, g, m, v, lr, wd, step) in zip(table, entries):
                row = entry if visible is None else entry.t
                row.param, row.grad, row.exp_avg, row.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                row.numel, row.lr, row.weight_decay, row.step = p.numel(), lr, wd, step
                if visible is not None and p.dim() >= 1 and p.shape[0] == visible.shape[0]:     # (else a dense entry of the same launch)
                    entry.row_mask, entry.rows = visible.data_ptr(), visible.shape[0]
            flags = (_lib.ADAM_DECOUPLED_WD if decoupled else 0) | _profile_flag()
            with torch.cuda.device(index):
                call = lib.lg_adam_step if visible is None else lib.lg_adam_step_rows
                _lib.check(call(len(entries), table, beta1, beta2, eps, flags, _lib.stream()))
            torch.autograd.graph.increment_version([t for e in entries for t in e[:1] + e[2:4]])
        return loss


def hip_step_class(cls):
    """The HIP-stepping subclass of `cls` (torch.optim.Adam or a subclass of it), one per class."""
    if issubclass(cls, _HipStep):
        return cls
    if not issubclass(cls, torch.optim.Adam):
        raise TypeError(f"{cls.__name__} is not a torch.optim.Adam")
    if cls not in _CLASSES:
        _CLASSES[cls] = type("Hip" + cls.__name__, (_HipStep, cls), {"__module__": __name__, "__doc__": f"{cls.__name__} stepping through lg_adam_step."})
    return _CLASSES[cls]


def convert(opt):
    """Turn an Adam / AdamW instance into the HIP-stepping subclass of its own class, in place (state and groups untouched)."""
    opt.__class__ = hip_step_class(type(opt))
    opt._patch_step_function()          # the step pre / post hooks wrap the new class's step, once
    return opt


class HipAdam(_HipStep, torch.optim.Adam):
    """torch.optim.Adam (weight decay in its L2 form) stepping through lg_adam_step."""

    def __init__(self, params, *args, **kw):
        super().__init__(params, *args, **kw)
        _refuse_cpu(_flat_params(self))


class HipAdamW(_HipStep, torch.optim.AdamW):
    """torch.optim.AdamW (decoupled weight decay) stepping through lg_adam_step."""

    def __init__(self, params, *args, **kw):
        super().__init__(params, *args, **kw)
        _refuse_cpu(_flat_params(self))


_CLASSES[torch.optim.Adam] = HipAdam
_CLASSES[torch.optim.AdamW] = HipAdamW
