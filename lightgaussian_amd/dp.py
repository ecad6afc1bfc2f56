"""Data-parallel training of the reference's UNMODIFIED trainers (`python -m lightgaussian_amd.run --distributed`).

One process per GPU, Gaussians replicated, every rank draws its cameras from its own shard of the train list, and the gradients
of the step are averaged over the ranks right before `optimizer.step()` -- a global batch of `world` views per optimizer step
where the reference trains on one (prune_finetune.py:144-168,287-289; distill_train.py:124-166; train_densify_prune.py:118-212).
Nothing in the trainers is edited; the glue hangs on four methods of the reference's classes:

    Scene.getTrainCameras                    rank r sees cameras r, r + world, ... of the (identically shuffled, scene/__init__.py:82-88)
                                             list: the trainers' `viewpoint_stack = scene.getTrainCameras().copy()` then walks a
                                             disjoint shard per rank -- an epoch still visits every camera exactly once.  The full
                                             list stays reachable as scene._lg_all_train_cameras() (the significance pass needs it:
                                             every rank must hand prune_list_sharded the same sequence).
    GaussianModel.training_setup             the optimizer it creates (scene/gaussian_model.py:184-217) gets its step() wrapped:
                                             average the gradients of the parameter groups over the ranks, then step.  Round 5: the
                                             SH-coefficient gradients (192 of the 236 gradient bytes per Gaussian at degree 3) are
                                             NOT all-reduced: the patched render() makes the rasterizer's backward leave dL/d(rgb)
                                             per Gaussian (12 B) and all-gathers that plus the camera centre behind K9
                                             (parallel.RankOneSHExchange); every rank rebuilds sum_ranks basis(dir) (x) dRGB locally
                                             (lg_sh_grad_from_rgb: the same bits on every rank).  The other four tensors (44 B per
                                             Gaussian) go through ONE bucketed dense all-reduce (parallel.allreduce_gradients), or --
                                             with one view per step -- in ranges overlapped with K9 (parallel.OverlappedGradAllReduce
                                             over lg_backward_chunked).  The round-4 form (dense SH gradients; only the rows some
                                             rank's camera saw: parallel.allreduce_gradients_visible) stays as the checker
                                             (configure(sh="dense") / configure(dense=True); visibility from note_render).
    GaussianModel.add_densification_stats    (train_densify_prune.py:175) the per-view statistics are summed over the ranks, so
                                             xyz_gradient_accum / denom -- and with them every densification decision -- are the same
                                             on every rank.
    GaussianModel.densify_and_prune          max_radii2D is max-reduced first (the trainer updates it in its own loop,
                                             train_densify_prune.py:172-174, from this rank's view only); afterwards the ranks check
                                             that they still hold the same number of Gaussians.

Consistency rule: every rank must execute the same collectives in the same order with the same N.  The parameters start equal
(same checkpoint / point cloud, same seeds: utils/general_utils.py:147-151), receive the same averaged gradients, and every
pruning / densification decision is a deterministic function of all-reduced data, so they stay equal; `assert_same_count()`
verifies it wherever N can change -- the count AND a 64-bit digest of the positions (one 16-byte all-gather): replicas that drifted
apart in VALUE with N intact (e.g. a rank whose RNG stream is off by one draw in the reference's densify_and_split,
scene/gaussian_model.py:666-700 `torch.normal`) would otherwise train `world` silently different models.  A mismatch raises on every
rank instead of hanging in the next collective.  Output files: ranks other than 0 write under <model_path>/.rank<r> (run.py rewrites their -m argument).
"""
import os
import threading

import torch
import torch.distributed as dist

from . import parallel

_STATE = {"installed": [], "group": None, "visible": {}, "lock": threading.Lock(), "steps": 0, "rows": 0, "dense_steps": 0,
          "adam_visible_steps": 0, "adam_dense_fallbacks": 0, "sinks": {}, "sh_steps": 0, "wire_bytes": 0, "sh_wire_bytes": 0, "mask_prev": None, "overlap": None, "stepped": {}}
# optimizer group name (scene/gaussian_model.py:204-211) -> attribute the fused rasterizer reports its gradient under
_GROUP_OF = {"_xyz": "xyz", "_features_dc": "f_dc", "_features_rest": "f_rest", "_opacity": "opacity", "_scaling": "scaling", "_rotation": "rotation"}


# Switches of the exchange.  They are set by configure() / install(**config) -- never read from the environment on the step's path
# (a stray variable in a user's shell must not change what a training step exchanges).  The launcher (`python -m lightgaussian_amd.run`)
# reads the LG_DP_* variables ONCE, at start-up, through config_from_env().
#   sh         "rank1": SH gradients through parallel.RankOneSHExchange (default); "dense": all-reduced like the rest (the checker)
#   force      exchange at world size 1 too (the RCCL code path on a 1-GPU box; tests)
#   check_set  compare the set of parameters that hold a gradient across the ranks: True every step, False never, None = the schedule of _check_same_set
#   dense      with sh="dense": one dense all-reduce of all six tensors instead of the visible-rows exchange
#   check      verify the visible-rows precondition: True every step, False never, None = every 64th step
#   overlap    install(): all-reduce the non-SH gradients in ranges behind K9 (parallel.OverlappedGradAllReduce)
_DEFAULTS = {"sh": "rank1", "force": False, "check_set": None, "dense": False, "check": None, "overlap": False}
_CONFIG = dict(_DEFAULTS)
_ENV = {"LG_DP_SH": ("sh", lambda v: "dense" if v == "dense" else "rank1"), "LG_DP_FORCE": ("force", lambda v: v == "1"),
        "LG_DP_CHECK_SET": ("check_set", lambda v: True if v == "1" else False if v == "0" else None), "LG_DP_DENSE": ("dense", lambda v: v == "1"),
        "LG_DP_CHECK": ("check", lambda v: True if v == "1" else False if v == "0" else None), "LG_DP_OVERLAP": ("overlap", lambda v: v == "1")}


def configure(**kw):
    """Set switches of the exchange (see _DEFAULTS above); unknown names raise.  Returns the configuration now in force."""
    for k, v in kw.items():
        if k not in _DEFAULTS:
            raise TypeError(f"dp.configure: unknown switch {k!r} (known: {sorted(_DEFAULTS)})")
        if k == "sh" and v not in ("rank1", "dense"):
            raise ValueError("dp.configure: sh must be 'rank1' or 'dense'")
        _CONFIG[k] = v
    return dict(_CONFIG)


def config_from_env(env=None):
    """The launcher's one read of the environment: LG_DP_SH=dense, LG_DP_FORCE=1, LG_DP_CHECK_SET=0|1, LG_DP_DENSE=1, LG_DP_CHECK=0|1,
    LG_DP_OVERLAP=1 become configure() switches.  Called by lightgaussian_amd.run at start-up, nowhere else."""
    env = os.environ if env is None else env
    return configure(**{key: conv(env[name]) for name, (key, conv) in _ENV.items() if name in env})


def sh_mode():
    """"rank1" (default): SH gradients through parallel.RankOneSHExchange; "dense" (configure(sh="dense")): all-reduced like the rest."""
    return _CONFIG["sh"]


def _forced():
    return bool(_CONFIG["force"]) and dist.is_available() and dist.is_initialized()


def active():
    return dist.is_available() and dist.is_initialized() and dist.get_world_size(_STATE["group"]) > 1


def _rank_world():
    if not (dist.is_available() and dist.is_initialized()):
        return 0, 1
    return dist.get_rank(_STATE["group"]), dist.get_world_size(_STATE["group"])


def replica_digest(t):
    """64-bit digest of a replicated tensor's VALUES: the int64 sum of its 32-bit patterns (one reduction kernel, no host copy of the
    tensor).  Equal replicas give equal digests; one differing element changes it unless another difference cancels it exactly."""
    if t is None or t.numel() == 0:
        return torch.zeros((), dtype=torch.int64, device=t.device if t is not None else "cpu")
    return torch.sum(t.detach().contiguous().view(torch.int32), dtype=torch.int64)


def assert_same_count(n, what="Gaussians", values=None):
    """Every rank must hold the same Gaussians before a collective sized by them: the same NUMBER and -- `values` (the model's _xyz)
    given -- the same VALUES (replica_digest).  One all-gather of two int64 per rank; a mismatch raises on every rank."""
    if not active():
        return
    rank, world = _rank_world()
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(_STATE["group"]) == "nccl" else torch.device("cpu")
    mine = torch.zeros(2, dtype=torch.int64, device=dev)
    mine[0] = int(n)
    if values is not None:
        mine[1] = replica_digest(values).to(dev)
    allc = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allc, mine, group=_STATE["group"])
    rows = [t.tolist() for t in allc]
    counts = [int(r[0]) for r in rows]
    if len(set(counts)) != 1:
        raise RuntimeError(f"data-parallel ranks diverged: number of {what} per rank = {counts} (rank {rank}); the next collective would "
                           "mismatch.  Every rank must load the same model and take the same prune / densify decisions.")
    digests = [int(r[1]) for r in rows]
    if len(set(digests)) != 1:
        raise RuntimeError(f"data-parallel ranks diverged in VALUE: the {what} hold different positions on different ranks (digest per rank = "
                           f"{[hex(d & 0xFFFFFFFFFFFFFFFF) for d in digests]}, rank {rank}) although their number agrees.  The replicas no longer "
                           "train one model -- typically a random-number stream that is out of step between the ranks (the reference's "
                           "densify_and_split draws from torch.normal): seed every rank identically and draw nothing rank-dependent.")


# ---- visibility of the step's renders -------------------------------------------------------------------------------------------

def note_render(pc, pkg):
    """Called with the result of every render() of a step: remembers (ORs) which Gaussians this rank's view(s) saw, keyed by the
    model's parameter tensor, for the gradient exchange in front of the next optimizer.step()."""
    if not torch.is_grad_enabled():
        return
    xyz = getattr(pc, "_xyz", None)
    vis = pkg.get("visibility_filter") if isinstance(pkg, dict) else None
    if xyz is None or vis is None or not getattr(xyz, "requires_grad", False):
        return
    with _STATE["lock"]:
        key = id(xyz)
        prev = _STATE["visible"].pop(key, None)
        # (clone: the fused path returns a view into the forward's saved geom buffer)
        _STATE["visible"][key] = (xyz, vis.detach().clone() if prev is None or prev[1].shape != vis.shape else prev[1].logical_or_(vis.detach()))
        while len(_STATE["visible"]) > 8:                 # models that are rendered with grad but never stepped: bounded
            _STATE["visible"].pop(next(iter(_STATE["visible"])))


def wrap_render(render_fn):
    """render() that also records the visibility for the gradient exchange (same signature, same result)."""
    import inspect
    try:
        sig = inspect.signature(render_fn).parameters
        takes_options = "options" in sig or any(q.kind is inspect.Parameter.VAR_KEYWORD for q in sig.values())
    except (TypeError, ValueError):
        takes_options = False

    def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, **kw):
        # (a render without an `options` parameter -- not ours -- cannot be told about the sink: its step takes the dense / visible-rows path)
        sink = _sink_for(pc, override_color, pipe) if (takes_options and torch.is_grad_enabled()) else None
        if sink is not None:
            kw["options"] = dict(kw.get("options") or {}, sh_grad_sink=sink)
        pkg = render_fn(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, **kw)
        note_render(pc, pkg)
        return pkg
    render.__wrapped__ = render_fn
    render.__module__ = getattr(render_fn, "__module__", __name__)
    render.__qualname__ = getattr(render_fn, "__qualname__", "render")
    render.__doc__ = render_fn.__doc__
    return render


def _sink_for(pc, override_color, pipe):
    """The RankOneSHExchange collecting this step's dRGB for the model `pc` (keyed by its _xyz tensor), or None when the render does
    not evaluate SH inside the rasterizer (override_color, convert_SHs_python), the model is not trainable, no exchange will follow,
    or configure(sh="dense")."""
    if sh_mode() != "rank1" or not (active() or _forced()):
        return None
    xyz = getattr(pc, "_xyz", None)
    if xyz is None or not getattr(xyz, "requires_grad", False) or override_color is not None or getattr(pipe, "convert_SHs_python", False):
        return None
    if not isinstance(getattr(pc, "_features_dc", None), torch.Tensor) or not isinstance(getattr(pc, "_features_rest", None), torch.Tensor):
        return None
    with _STATE["lock"]:
        # only models whose optimizer.step is the wrapped one get a sink: anywhere else (an optimizer created before install(), a teacher with
        # requires_grad) nobody would rebuild the SH gradients from it and f_dc / f_rest would silently stop training
        reg = _STATE["stepped"].get(id(xyz))
        if reg is None or reg() is not xyz:
            return None
        ent = _STATE["sinks"].get(id(xyz))
        if ent is None or ent[0] is not xyz:
            ent = _STATE["sinks"][id(xyz)] = (xyz, parallel.RankOneSHExchange(_STATE["group"], average=True, force=_forced()))
            while len(_STATE["sinks"]) > 8:
                _STATE["sinks"].pop(next(iter(_STATE["sinks"])))
        return ent[1]


def _take_sink(params):
    with _STATE["lock"]:
        for key, (xyz, sink) in list(_STATE["sinks"].items()):
            if any(xyz is p for p in params):
                del _STATE["sinks"][key]
                return sink if sink.views else None
    return None


def _check_same_set(mask_bits, force=False):
    """Every rank must exchange the same set of parameters (the flat buffers are sized by it).  The set follows from the trainer's
    iteration logic -- e.g. train_densify_prune.py:194-197 swaps the opacity Parameter in reset_opacity() between backward() and
    step(), leaving that group without a gradient on EVERY rank -- so it is compared, not assumed: one 16-byte MAX all-reduce of
    (mask, ~mask).  When: the comparison reads its result on the host, i.e. it drains the device and costs the step its run-ahead,
    so it is not made every step: on the first 8 steps, on every 64th, and on every step whose set differs from this rank's previous
    one (ranks that change together -- the legitimate case -- all compare; a rank that changes ALONE enters a collective the others do
    not, which fails in the collective itself: no schedule short of every step can turn that into a clean error).
    configure(check_set=True): every step (tests); check_set=False: never."""
    mode = _CONFIG["check_set"]
    n, prev = _STATE["steps"], _STATE.get("mask_prev")
    _STATE["mask_prev"] = mask_bits
    if mode is False or not (mode is True or n <= 8 or n % 64 == 0 or (prev is not None and prev != mask_bits)):
        return
    group = _STATE["group"]
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    t = torch.tensor([mask_bits, (~mask_bits) & 0xFFFFFFFF], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    hi, lo = int(t[0].item()), (~int(t[1].item())) & 0xFFFFFFFF
    if hi != mask_bits or lo != mask_bits:
        raise RuntimeError(f"data-parallel step: the ranks hold gradients for different parameter groups (this rank: mask {mask_bits:#x}, union "
                           f"{hi:#x}, intersection {lo:#x}); every rank must differentiate the same set of parameters")


def _take_visible(params):
    """The recorded visibility whose model owns `params` (by the identity of its _xyz tensor), or None."""
    ids = {id(p) for p in params}
    with _STATE["lock"]:
        hit = None
        for key, (xyz, vis) in list(_STATE["visible"].items()):
            if key in ids and any(xyz is p for p in params):
                hit = vis
                del _STATE["visible"][key]
    return hit


def take_visible_for_step(params, closure=None):
    """run.py --hip-adam=visible: the union of the views rendered with grad since the last step of the optimizer over `params`, for
    HipAdam.step(visible=) -- the same record the visible-rows exchange reads -- or None: nothing was recorded (renders under
    no_grad, a closure that has yet to render, a model without _xyz), or a densify / prune has replaced the tensors since and no
    parameter with a gradient has the mask's row count.  None is the dense step; both outcomes are counted (stats())."""
    vis = _take_visible(params) if closure is None else None
    if vis is not None and vis.dtype not in (torch.bool, torch.uint8):
        vis = vis != 0
    if vis is not None and not any(p.grad is not None and p.dim() >= 1 and p.shape[0] == vis.shape[0] for p in params):
        vis = None
    _STATE["adam_visible_steps" if vis is not None else "adam_dense_fallbacks"] += 1
    return vis


def exchange_gradients(optimizer, check=None, force=None):
    """Average the gradients of the parameter groups of `optimizer` over the ranks (in place), right before its step().

    Which parameters: those that HAVE a gradient on this rank -- single-process Adam skips a group whose .grad is None, and the
    reference's own trainer produces that state (train_densify_prune.py:194-197: reset_opacity() replaces the opacity Parameter
    between backward() and step()) -- plus the two SH groups when this step's renders went through the rank-one exchange
    (their .grad is None by design: the sink holds dRGB instead).  The set is compared across ranks (_check_same_set).
    How: SH groups rebuilt from the all-gathered dRGB (parallel.RankOneSHExchange.finish); the others by one bucketed dense
    all-reduce -- or, under configure(sh="dense") when the step's renders were seen by note_render, the round-4 visible-rows exchange
    of all six (check: verify its precondition -- rows outside this rank's visibility exactly zero -- default: configure(check=...),
    i.e. every 64th step).  force: exchange at world size 1 too (the RCCL code path on a 1-GPU box; default: configure(force=...))."""
    if force is None:
        force = bool(_CONFIG["force"])
    if not (active() or (force and dist.is_available() and dist.is_initialized())):
        return None
    groups = [(g.get("name"), p) for g in optimizer.param_groups for p in g["params"]]
    params = [p for _n, p in groups]
    sink = _take_sink(params)
    by_name = {n: p for n, p in groups if n is not None}
    sh_params = [by_name.get("f_dc"), by_name.get("f_rest")] if sink is not None else []
    if sink is not None and (sh_params[0] is None or sh_params[1] is None or by_name.get("xyz") is None):
        raise RuntimeError("data-parallel step: dRGB was collected for a model whose optimizer has no f_dc / f_rest / xyz groups "
                           "(scene/gaussian_model.py:204-211 names them); use dp.configure(sh='dense')")
    # An SH group that ALREADY holds a gradient next to the sink's dRGB -- another render of the step went through override_color /
    # convert_SHs_python / a render() without `options`, or a regulariser acts on the coefficients: that gradient is all-reduced like the
    # other tensors and the rebuilt one is ADDED to it (it used to be overwritten, and was never reduced).
    have = [p for p in params if p.grad is not None]
    _STATE["steps"] += 1
    mask_bits = sum(1 << i for i, p in enumerate(params[:16]) if p.grad is not None or any(p is q for q in sh_params))
    mask_bits |= sum(1 << (16 + i) for i, p in enumerate(params[:16]) if p.grad is not None and any(p is q for q in sh_params))
    _check_same_set(mask_bits, force)
    vis = _take_visible(params)
    if not have and sink is None:
        return None
    info = {"mode": "dense", "of": int(params[0].shape[0]), "params": len(have) + sum(1 for q in sh_params if q.grad is None)}
    rebuilt = []
    if sink is not None:
        xyz = by_name["xyz"]
        M = 1 + int(sh_params[1].shape[1])
        g_dc, g_rest = sink.finish(xyz, M)
        rebuilt = [(sh_params[0], g_dc.view_as(sh_params[0])), (sh_params[1], g_rest.view_as(sh_params[1]))]
        _STATE["sh_steps"] += 1
        _STATE["wire_bytes"] += sink.bytes_on_wire
        _STATE["sh_wire_bytes"] += sink.bytes_on_wire
        info.update(mode="rank1_sh+dense", sh_bytes_on_wire=sink.bytes_on_wire)

    def _rest(have):
        nonlocal check
        ov = _STATE.get("overlap")
        if ov is not None and ov.grads is not None:
            # install(overlap=True) / run.py --dp-overlap: the step's ONE rasterizer backward ran its per-Gaussian stage in ranges, and each range of the
            # (non-SH) gradient tensors was all-reduced on a side stream while K9 computed the next one (parallel.OverlappedGradAllReduce over
            # lg_backward_chunked).  The reduced tensors replace what autograd put into the leaves; whatever the hook did not see -- the literal
            # getter pattern reports gradients of the ACTIVATED tensors, which are not parameters -- goes through the dense all-reduce below.
            reduced = ov.finish(None)
            ov.grads = None
            done = []
            if all(n in _GROUP_OF for n in reduced):
                for n, g in reduced.items():
                    q = by_name.get(_GROUP_OF[n])
                    if q is not None and q.grad is not None and q.grad.numel() == g.numel():
                        q.grad = g.view_as(q)
                        done.append(q)
            have = [q for q in have if not any(q is d for d in done)]
            info["overlapped"] = len(done)
            _STATE["overlap_steps"] = _STATE.get("overlap_steps", 0) + (1 if done else 0)
        if not have:
            return info
        N = have[0].shape[0]
        rows_ok = sink is None and vis is not None and vis.shape[0] == N and all(p.grad.shape[0] == N for p in have) and len(have) == len(params)
        if rows_ok and not _CONFIG["dense"]:
            if check is None:
                check = _CONFIG["check"] is True or (_CONFIG["check"] is None and _STATE["steps"] % 64 == 1)
            if check:
                hidden = ~vis.reshape(-1).bool()
                for p in have:
                    if bool((p.grad.reshape(N, -1)[hidden] != 0).any()):
                        raise RuntimeError("data-parallel step: a gradient row of a Gaussian no render of this step saw is non-zero; the "
                                           "visible-rows exchange would leave it unreduced (use dp.configure(dense=True))")
            k, _ = parallel.allreduce_gradients_visible(have, vis, group=_STATE["group"], force=force)
            _STATE["rows"] += k
            world = dist.get_world_size(_STATE["group"])
            _STATE["wire_bytes"] += int(2 * (N + k * sum(p.grad[0].numel() * 4 for p in have)) * (world - 1) / max(world, 1))
            info.update(mode="visible", rows=k)
            return info
        _STATE["dense_steps"] += 1
        info["collectives"] = parallel.allreduce_gradients(have, group=_STATE["group"], force=force)
        nb = sum(p.grad.numel() * 4 for p in have)
        world = dist.get_world_size(_STATE["group"])
        _STATE["wire_bytes"] += int(2 * nb * (world - 1) / max(world, 1))
        return info

    info = _rest(have)
    for q, g in rebuilt:                       # (after the all-reduce of whatever autograd had put there)
        q.grad = g if q.grad is None else q.grad.add_(g)
    return info


def wrap_optimizer(optimizer):
    """optimizer.step() := exchange_gradients(optimizer); step().  Idempotent."""
    if getattr(optimizer, "_lg_dp_wrapped", False):
        return optimizer
    inner = optimizer.step

    def step(*a, **kw):
        if kw.get("visible") is not None:
            # (refused before anything is exchanged: every rank would have to step the union of all ranks' views)
            raise RuntimeError("step(visible=) on a data-parallel optimizer (dp.wrap_optimizer): the replicas stay identical only under "
                               "the union of the ranks' visibility, which is not exchanged; take the dense step")
        # (configure(force=True): exchange at world size 1 too -- the RCCL code path of a 1-GPU box, tests/test_gpu_dp_runner.py)
        exchange_gradients(optimizer)
        out = inner(*a, **kw)
        _register(optimizer)
        return out

    optimizer.step = step
    optimizer._lg_dp_wrapped = True
    _register(optimizer)
    return optimizer


def _register(optimizer):
    """Remember which model (by its `xyz` parameter) this wrapped optimizer steps -- only such models are handed an SH-gradient sink -- and
    drop what was recorded for tensors that are no parameter of it any more: a prune / densify between backward() and step() replaces every
    Parameter (train_densify_prune.py), and the sink of the old _xyz would otherwise pin it and the gathered [world, 3 N + 3] buffers for the
    rest of the run (0.3 GB per stale sink at 3 M Gaussians on 8 ranks).  Every stale entry goes, whatever the size of the store;
    outstanding gathers are waited for first."""
    import weakref
    with _STATE["lock"]:
        live = {id(p): p for g in optimizer.param_groups for p in g["params"]}
        mine = getattr(optimizer, "_lg_dp_ids", set())
        for key in [k for k in mine if k not in live]:
            _STATE["stepped"].pop(key, None)
            ent = _STATE["sinks"].pop(key, None)
            if ent is not None:
                ent[1].abandon()
            _STATE["visible"].pop(key, None)
        for key in [k for k, ref in _STATE["stepped"].items() if ref() is None]:
            _STATE["stepped"].pop(key, None)
        for g in optimizer.param_groups:
            if g.get("name") == "xyz":
                for p in g["params"]:
                    _STATE["stepped"][id(p)] = weakref.ref(p)
        optimizer._lg_dp_ids = set(live)


# ---- patches on the reference's classes ------------------------------------------------------------------------------------------

def _set(owner, name, new):
    _STATE["installed"].append((owner, name, owner.__dict__.get(name, None), name in owner.__dict__))
    setattr(owner, name, new)


def shard_cameras(cams, rank, world):
    """Cameras of `rank`: every world-th of the list (an empty shard -- fewer cameras than ranks -- falls back to the whole list)."""
    mine = list(cams)[rank::world]
    return mine if mine else list(cams)


def install(gaussian_model_cls=None, scene_cls=None, group=None, overlap=None, **config):
    """Hang the data-parallel glue on the reference's classes (see the module docstring).  Safe to call at world size 1 (every hook
    degenerates to the original behaviour).  uninstall() restores the classes.
    overlap (default: configure(overlap=...)): all-reduce the non-SH gradients in ranges behind K9 instead of after backward() returns
    (one rasterizer backward per optimizer step, as all three reference trainers have it; a second one before step() raises).
    **config: further configure() switches."""
    _STATE["group"] = group
    if config:
        configure(**config)
    if overlap is None:
        overlap = bool(_CONFIG["overlap"])
    if overlap and (active() or _forced()) and _STATE.get("overlap") is None:
        _STATE["overlap"] = parallel.OverlappedGradAllReduce(group, chunks=4)
        _STATE["overlap"].__enter__()
    if scene_cls is not None and hasattr(scene_cls, "getTrainCameras") and not hasattr(scene_cls, "_lg_all_train_cameras"):
        orig_get = scene_cls.getTrainCameras

        def getTrainCameras(self, scale=1.0):
            rank, world = _rank_world()
            full = orig_get(self, scale)
            return shard_cameras(full, rank, world) if world > 1 else full

        _set(scene_cls, "_lg_all_train_cameras", orig_get)
        _set(scene_cls, "getTrainCameras", getTrainCameras)
    gm = gaussian_model_cls
    if gm is not None and hasattr(gm, "training_setup") and not getattr(gm.training_setup, "_lg_dp", False):
        orig_setup = gm.training_setup

        def training_setup(self, training_args):
            out = orig_setup(self, training_args)
            wrap_optimizer(self.optimizer)
            return out

        training_setup._lg_dp = True
        _set(gm, "training_setup", training_setup)
    if gm is not None and hasattr(gm, "add_densification_stats") and not getattr(gm.add_densification_stats, "_lg_dp", False):
        def add_densification_stats(self, viewspace_point_tensor, update_filter):
            """scene/gaussian_model.py:784-788 with the per-view increments summed over the ranks."""
            if not active():
                self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1, keepdim=True)
                self.denom[update_filter] += 1
                return
            n = self.xyz_gradient_accum.shape[0]
            # one [N, 2] buffer kept across iterations (r4 verdict: it was allocated anew every step); dense on purpose: the ranks'
            # update_filters differ, and 8 B per Gaussian is 3 % of what the gradient exchange of the same step moves
            inc = getattr(self, "_lg_dp_inc", None)
            if inc is None or inc.shape[0] != n or inc.device != self.xyz_gradient_accum.device:
                inc = self._lg_dp_inc = torch.zeros((n, 2), dtype=self.xyz_gradient_accum.dtype, device=self.xyz_gradient_accum.device)
            else:
                inc.zero_()
            inc[update_filter, 0:1] = torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1, keepdim=True)
            inc[update_filter, 1] = 1
            dist.all_reduce(inc, op=dist.ReduceOp.SUM, group=_STATE["group"])
            self.xyz_gradient_accum += inc[:, 0:1]
            self.denom += inc[:, 1:2]

        add_densification_stats._lg_dp = True
        _set(gm, "add_densification_stats", add_densification_stats)
    if gm is not None and hasattr(gm, "densify_and_prune") and not getattr(gm.densify_and_prune, "_lg_dp", False):
        orig_dap = gm.densify_and_prune

        def densify_and_prune(self, *a, **kw):
            if active():
                assert_same_count(self.get_xyz.shape[0], values=self.get_xyz)
                dist.all_reduce(self.max_radii2D, op=dist.ReduceOp.MAX, group=_STATE["group"])
            out = orig_dap(self, *a, **kw)
            if active():
                assert_same_count(self.get_xyz.shape[0], "Gaussians after densify_and_prune", values=self.get_xyz)
            return out

        densify_and_prune._lg_dp = True
        _set(gm, "densify_and_prune", densify_and_prune)


def uninstall():
    while _STATE["installed"]:
        owner, name, old, had = _STATE["installed"].pop()
        if had:
            setattr(owner, name, old)
        else:
            try:
                delattr(owner, name)
            except AttributeError:
                pass
    _STATE["visible"].clear()
    for _k, ent in list(_STATE["sinks"].items()):
        ent[1].abandon()
    _STATE["sinks"].clear()
    _STATE["stepped"].clear()
    if _STATE.get("overlap") is not None:
        _STATE["overlap"].__exit__(None, None, None)
        _STATE["overlap"] = None
    _STATE["group"] = None
    _CONFIG.update(_DEFAULTS)


def stats():
    """Counters of the exchanges so far: steps, rows exchanged (visible mode), steps that fell back to the dense all-reduce; and of
    run.py --hip-adam=visible: optimizer steps masked by the recorded visibility, steps that took the dense step instead."""
    return {"adam_visible_steps": _STATE["adam_visible_steps"], "adam_dense_fallbacks": _STATE["adam_dense_fallbacks"], "steps": _STATE["steps"], "rows_exchanged": _STATE["rows"], "dense_steps": _STATE["dense_steps"],
            "rank1_sh_steps": _STATE["sh_steps"], "overlapped_steps": _STATE.get("overlap_steps", 0), "bytes_on_wire": _STATE["wire_bytes"], "sh_bytes_on_wire": _STATE["sh_wire_bytes"]}
    # (bytes_on_wire: what a ring moves through this rank -- 2 (w - 1) / w of the payload for an all-reduce, payload x w for the
    #  all-gather of dRGB (own block sent once, w - 1 blocks received); an estimate from the tensor sizes, not a counter)
