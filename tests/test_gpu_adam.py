"""-m gpu: lg_adam_step through lightgaussian_amd.optim.HipAdam / HipAdamW against torch's own optimizers.

Parity rule, used throughout.  R64 = torch.optim.AdamW / Adam on float64 CPU copies of the same inputs; T32 = torch's default
(non-fused) optimizer in float32 on the GPU, which is what the HIP step replaces.  For param, exp_avg and exp_avg_sq of every tensor:

    max|ours - R64| <= 4 max|T32 - R64| + 2^-23 max|R64|

(4: the project's margin for float32 state against a float64 reference, as in the VQ training step; the last term only covers a
tensor where T32 happens to be exact).  The observed ratio max|ours - R64| / max|T32 - R64| is printed per tensor."""
import functools
import math
import warnings

import pytest
import torch

from lightgaussian_amd import _lib, optim, run as lg_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAN, MAXT = optim.SPAN, optim.MAX_TENSORS
EPS = 1e-15                                 # training_setup's
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
# training_setup's learning rates (arguments/__init__.py defaults, spatial_lr_scale 1)
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)


def model_shapes(N):
    return dict(xyz=(N, 3), f_dc=(N, 1, 3), f_rest=(N, 15, 3), opacity=(N, 1), scaling=(N, 3), rotation=(N, 4))


def bits(t):       # (not common.bits: an integer torch view of any element size, on the device)
    return t.detach().contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def gradient(shape, gen, never=None):
    """Rows scaled log-normally (sigma 4 in log space), magnitudes no smaller than 1e-12, every third row exactly zero, the row
    `never` always zero."""
    g = torch.randn(shape, generator=gen)
    rows = torch.exp(4.0 * torch.randn((shape[0],) + (1,) * (len(shape) - 1), generator=gen))
    g = g * rows
    g = torch.where(g < 0, -1.0, 1.0) * g.abs().clamp_min(1e-12)
    g[0::3] = 0.0
    if never is not None and never < shape[0]:
        g[never] = 0.0
    return g


def check_rule(label, ours, t32, r64):
    """The parity rule on three lists of {"p", "m", "v"} dicts; returns the largest observed ratio."""
    worst = 0.0
    for k, (o, t, r) in enumerate(zip(ours, t32, r64)):
        for key in ("p", "m", "v"):
            ref = r[key].double().cpu()
            if ref.numel() == 0:
                assert o[key].numel() == 0
                continue
            eo = (o[key].double().cpu() - ref).abs().max().item()
            et = (t[key].double().cpu() - ref).abs().max().item()
            bound = 4.0 * et + 2.0 ** -23 * ref.abs().max().item()
            ratio = eo / et if et > 0 else (0.0 if eo == 0 else math.inf)
            print(f"{label} tensor {k} {key}: ours {eo:.3e} T32 {et:.3e} ratio {ratio:.3f}")
            assert math.isfinite(eo) and eo <= bound, f"{label} tensor {k} {key}: |ours - R64| {eo:.3e} > bound {bound:.3e} (T32 {et:.3e})"
            if et > 0:
                worst = max(worst, ratio)
    return worst


def snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append(dict(p=p.detach().clone(), m=st["exp_avg"].detach().clone() if st else torch.zeros(0),
                        v=st["exp_avg_sq"].detach().clone() if st else torch.zeros(0)))
    return out


def launches():
    torch.cuda.synchronize()
    return _lib.profile_read().get("adam", (0.0, 0))[1]


# ---- 1. model shapes ------------------------------------------------------------------------------------------------------------

STEPS1 = 4


@functools.lru_cache(maxsize=None)
def model_inputs(scale):
    gen = torch.Generator().manual_seed(1234)
    shapes = model_shapes(1025)
    params = {n: scale * torch.randn(s, generator=gen) for n, s in shapes.items()}
    grads = [{n: gradient(s, gen, never=7) for n, s in shapes.items()} for _ in range(STEPS1)]
    xyz_lr = [LRS["xyz"] * 0.5 ** k for k in range(STEPS1)]
    return params, grads, xyz_lr


def run_model(cls, scale, device, dtype, stream=None):
    params0, grads, xyz_lr = model_inputs(scale)
    ps = {n: torch.nn.Parameter(t.to(device=device, dtype=dtype).clone()) for n, t in params0.items()}
    gs = [{n: g.to(device=device, dtype=dtype) for n, g in step.items()} for step in grads]
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(None)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with ctx:
        opt = cls([{"params": [ps[n]], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=EPS)
        for k in range(STEPS1):
            for group in opt.param_groups:
                if group["name"] == "xyz":
                    group["lr"] = xyz_lr[k]
            for n in NAMES:
                ps[n].grad = gs[k][n]
            opt.step()
        out = snapshot(opt, [ps[n] for n in NAMES])
    if stream is not None:
        stream.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def model_references(scale):
    return run_model(torch.optim.AdamW, scale, DEV, torch.float32), run_model(torch.optim.AdamW, scale, "cpu", torch.float64)


@functools.lru_cache(maxsize=None)
def model_ours(scale):
    optim.set_profile(True)
    _lib.profile_reset()
    try:
        out = run_model(optim.HipAdamW, scale, DEV, torch.float32)
        n = launches()
    finally:
        optim.set_profile(False)
    return out, n


@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_model_shapes(scale):
    t32, r64 = model_references(scale)
    ours, n = model_ours(scale)
    assert n == STEPS1, f"{n} launches for {STEPS1} steps of the six-group model (one per step expected)"
    print("largest ratio:", check_rule(f"model scale {scale:g}", ours, t32, r64))
    # the row that never saw a gradient only decayed; its moments are exactly zero
    assert not ours[0]["m"][7].any() and not ours[0]["v"][7].any()


# ---- 2. boundaries --------------------------------------------------------------------------------------------------------------

PAD = 64                                    # floats of sentinel on either side (a multiple of 4: the view keeps the buffer's alignment)
SENTINEL = 0x7FC12345                       # a NaN with a payload: any arithmetic on it, and any stray store, shows
BOUNDARY_NUMELS = [1, 2, 3, 4, 5, 1023, 1024, 1025, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3, 0] + [7, 8, 9, 10, 11, 12, 13]
# (numel, which of param / grad / exp_avg / exp_avg_sq starts one float into its storage)
MISALIGNED = [(2 * SPAN + 5, "p"), (SPAN + 8, "v")]


def guarded(values, shift):
    buf = torch.full((values.numel() + 2 * PAD + 1,), 0.0, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    view = buf[PAD + shift:PAD + shift + values.numel()]
    view.copy_(values.to(DEV))
    return buf, view


def guards_intact(buf, shift, n):
    b = buf.view(torch.int32).cpu()
    return bool((b[:PAD + shift] == SENTINEL).all()) and bool((b[PAD + shift + n:] == SENTINEL).all())


def test_boundaries():
    gen = torch.Generator().manual_seed(77)
    cases = [(n, "") for n in BOUNDARY_NUMELS] + MISALIGNED
    steps = 3
    p0 = [torch.randn(n, generator=gen) for n, _ in cases]
    g0 = [[gradient((n,), gen) if n else torch.zeros(0) for n, _ in cases] for _ in range(steps)]
    lrs = [1e-3 * (1 + k % 5) for k in range(len(cases))]

    def plain(device, dtype):
        ps = [torch.nn.Parameter(t.to(device=device, dtype=dtype).clone()) for t in p0]
        opt = torch.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], lr=0.0, eps=EPS)
        for s in range(steps):
            for p, g in zip(ps, g0[s]):
                p.grad = g.to(device=device, dtype=dtype)
            opt.step()
        return snapshot(opt, ps)

    t32, r64 = plain(DEV, torch.float32), plain("cpu", torch.float64)
    bufs, ps = [], []
    for (n, mis), t in zip(cases, p0):
        entry = {}
        for key in ("p", "g", "m", "v"):
            shift = 1 if key == mis else 0
            entry[key] = guarded(t if key == "p" else torch.zeros(n), shift) + (shift,)
        bufs.append(entry)
        ps.append(entry["p"][1].requires_grad_(True))
    opt = optim.HipAdamW([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], lr=0.0, eps=EPS)
    for p, e in zip(ps, bufs):              # the state torch's default step would have created, inside the guarded buffers
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": e["m"][1], "exp_avg_sq": e["v"][1]}
        p.grad = e["g"][1]
    nonempty = sum(1 for n, _ in cases if n > 0)
    assert nonempty > 2 * MAXT
    optim.set_profile(True)
    _lib.profile_reset()
    try:
        for s in range(steps):
            for e, g in zip(bufs, g0[s]):
                e["g"][1].copy_(g.to(DEV))
            opt.step()
        n_launch = launches()
    finally:
        optim.set_profile(False)
    assert n_launch == steps * math.ceil(nonempty / MAXT), (n_launch, nonempty)
    for (n, _), e in zip(cases, bufs):
        for key in ("p", "g", "m", "v"):
            assert guards_intact(e[key][0], e[key][2], n), f"numel {n}: the sentinel around {key} was overwritten"
    ours = [dict(p=e["p"][1], m=e["m"][1], v=e["v"][1]) for e in bufs]
    print("largest ratio:", check_rule("boundaries", ours, t32, r64))
    assert all(int(opt.state[p]["step"]) == steps for (n, _), p in zip(cases, ps))


# ---- 3. semantics ---------------------------------------------------------------------------------------------------------------

def small_inputs(seed, n=2 * 1025 + 3, steps=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen), [gradient((n,), gen) for _ in range(steps)]


def run_small(cls, device, dtype, p0, grads, **kw):
    p = torch.nn.Parameter(p0.to(device=device, dtype=dtype).clone())
    opt = cls([p], **kw)
    for g in grads:
        p.grad = g.to(device=device, dtype=dtype)
        opt.step()
    return opt, p


def test_group_without_gradient_is_untouched_and_stateless():
    a = torch.nn.Parameter(torch.randn(300, device=DEV))
    b = torch.nn.Parameter(torch.randn(300, device=DEV))
    a0, before = a.detach().clone(), b.detach().clone()
    opt = optim.HipAdamW([{"params": [a], "lr": 0.01}, {"params": [b], "lr": 0.01}], lr=0.0)
    a.grad = torch.randn(300, device=DEV)
    opt.step()
    assert same_bits(b, before) and b not in opt.state and b._version == 0
    assert int(opt.state[a]["step"]) == 1 and not same_bits(a, a0)
    b.grad = torch.randn(300, device=DEV)
    opt.step()
    assert int(opt.state[a]["step"]) == 2 and int(opt.state[b]["step"]) == 1      # b's own first step


def test_zero_lr_keeps_the_parameter_bits_while_the_moments_move():
    p0, grads = small_inputs(5)
    opt, p = run_small(optim.HipAdamW, DEV, torch.float32, p0, grads, lr=0.0, eps=EPS)
    assert same_bits(p, p0)
    assert opt.state[p]["exp_avg"].abs().max() > 0 and opt.state[p]["exp_avg_sq"].abs().max() > 0


@pytest.mark.parametrize("kind, wd", [("Adam", 0.0), ("Adam", 0.1), ("AdamW", 0.0), ("AdamW", 0.01)])
def test_weight_decay_forms(kind, wd):
    p0, grads = small_inputs(11)
    kw = dict(lr=2e-3, eps=1e-8, weight_decay=wd)
    res = []
    for cls, device, dtype in ((getattr(optim, "Hip" + kind), DEV, torch.float32), (getattr(torch.optim, kind), DEV, torch.float32),
                               (getattr(torch.optim, kind), "cpu", torch.float64)):
        opt, p = run_small(cls, device, dtype, p0, grads, **kw)
        res.append(snapshot(opt, [p]))
    print("largest ratio:", check_rule(f"{kind} wd {wd}", *res))


INELIGIBLE = {
    "amsgrad": (dict(amsgrad=True), torch.float32, False),
    "maximize": (dict(maximize=True), torch.float32, False),
    "capturable": (dict(capturable=True), torch.float32, False),
    "differentiable": (dict(differentiable=True), torch.float32, False),
    "tensor lr": (dict(lr=torch.tensor(2e-3)), torch.float32, False),
    "float64": (dict(), torch.float64, False),
    "float16": (dict(), torch.float16, False),
    "non-contiguous": (dict(), torch.float32, True),
}


@pytest.mark.parametrize("name", sorted(INELIGIBLE))
def test_ineligible_configuration_takes_torchs_step_and_warns_once(name):
    kw, dtype, strided = INELIGIBLE[name]
    kw = dict(dict(lr=2e-3, weight_decay=0.01), **kw)
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(64, 6, generator=gen)
    grads = [torch.randn(64, 6, generator=gen) for _ in range(2)]

    def run(cls):
        base = p0.to(device=DEV, dtype=dtype).clone()
        p = base.t() if strided else base                      # (plain tensors: differentiable=True steps leaves in place)
        opt = cls([p], **kw)
        for g in grads:
            g = g.to(device=DEV, dtype=dtype)
            p.grad = g.t() if strided else g
            opt.step()
        return p, opt.state[p]

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        p, st = run(optim.HipAdamW)
    ours = [w for w in caught if "lg_adam_step" in str(w.message)]
    assert len(ours) == 1, [str(w.message) for w in caught]
    q, sq = run(torch.optim.AdamW)
    assert torch.equal(p.detach().cpu(), q.detach().cpu())
    assert torch.equal(st["exp_avg"].cpu(), sq["exp_avg"].cpu()) and torch.equal(st["exp_avg_sq"].cpu(), sq["exp_avg_sq"].cpu())
    assert float(st["step"]) == float(sq["step"]) == 2.0


def test_sparse_gradient_is_torchs_error():
    for cls in (torch.optim.AdamW, optim.HipAdamW):
        p = torch.nn.Parameter(torch.randn(8, 4, device=DEV))
        before = p.detach().clone()
        opt = cls([p], lr=1e-2)
        p.grad = torch.zeros(8, 4, device=DEV).to_sparse()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(RuntimeError, match="sparse gradients"):
                opt.step()
        assert same_bits(p, before)


# ---- 4. version counters --------------------------------------------------------------------------------------------------------

def test_version_counters_rise_and_autograd_sees_the_write():
    p = torch.nn.Parameter(torch.randn(500, device=DEV))
    opt = optim.HipAdamW([p], lr=1e-2)
    seen = []
    for _ in range(3):
        p.grad = torch.randn(500, device=DEV)
        opt.step()
        st = opt.state[p]
        seen.append((p._version, st["exp_avg"]._version, st["exp_avg_sq"]._version))
    assert all(b[k] > a[k] for a, b in zip(seen, seen[1:]) for k in range(3)) and min(seen[0]) >= 1, seen
    for cls in (torch.optim.AdamW, optim.HipAdamW):
        q = torch.nn.Parameter(torch.randn(50, device=DEV))
        o = cls([q], lr=1e-2)
        q.grad = torch.ones(50, device=DEV)
        y = (q * q).sum()
        o.step()
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            y.backward()


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------

def test_deterministic_also_on_a_side_stream():
    first, _ = model_ours(1.0)
    again = run_model(optim.HipAdamW, 1.0, DEV, torch.float32)
    side = torch.cuda.Stream()
    busy = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):                                          # unrelated work in flight on the default stream
        busy = (busy @ busy).clamp_(-1.0, 1.0)
    streamed = run_model(optim.HipAdamW, 1.0, DEV, torch.float32, stream=side)
    torch.cuda.synchronize()
    for a, b, c in zip(first, again, streamed):
        for key in ("p", "m", "v"):
            assert same_bits(a[key], b[key]) and same_bits(a[key], c[key]), key


# ---- 6. state surgery and checkpoints -------------------------------------------------------------------------------------------

class StandIn:
    """The attribute surface prune.prune_points touches: six named one-tensor groups and the three bookkeeping tensors."""

    def __init__(self, cls, params, device, dtype):
        self.tensors = {n: torch.nn.Parameter(t.to(device=device, dtype=dtype).clone()) for n, t in params.items()}
        self.optimizer = cls([{"params": [self.tensors[n]], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=EPS)
        n = params["xyz"].shape[0]
        self.xyz_gradient_accum = torch.zeros(n, 1, device=device)
        self.denom = torch.zeros(n, 1, device=device)
        self.max_radii2D = torch.zeros(n, device=device)

    def params(self):
        return [g["params"][0] for g in self.optimizer.param_groups]

    def step(self, grads):
        for g, p in zip(self.optimizer.param_groups, self.params()):
            p.grad = grads[g["name"]].to(device=p.device, dtype=p.dtype)
        self.optimizer.step()

    def prune(self, mask):
        """Rows with mask set leave: prune.prune_points on the GPU, the same surgery by boolean indexing on the CPU reference."""
        if self.params()[0].is_cuda:
            from lightgaussian_amd import prune
            prune.prune_points(self, mask.to(self.params()[0].device))
            return
        keep = ~mask
        for g in self.optimizer.param_groups:
            old = g["params"][0]
            st = self.optimizer.state.pop(old)
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][keep].clone(), st["exp_avg_sq"][keep].clone()
            g["params"][0] = torch.nn.Parameter(old.detach()[keep].clone())
            self.optimizer.state[g["params"][0]] = st

    def extend(self, new_rows):
        """Append rows: the moments of the new rows start at zero, reached by their keys; every Parameter is replaced."""
        for g in self.optimizer.param_groups:
            old = g["params"][0]
            rows = new_rows[g["name"]].to(device=old.device, dtype=old.dtype)
            st = self.optimizer.state.pop(old)
            for key in ("exp_avg", "exp_avg_sq"):
                st[key] = torch.cat([st[key], torch.zeros_like(rows)], dim=0)
            g["params"][0] = torch.nn.Parameter(torch.cat([old.detach(), rows], dim=0))
            self.optimizer.state[g["params"][0]] = st


def surgery_inputs():
    gen = torch.Generator().manual_seed(99)
    N, added = 1500, 300
    shapes = model_shapes(N)
    params = {n: torch.randn(s, generator=gen) for n, s in shapes.items()}
    mask = torch.rand(N, generator=gen) < 0.3
    n2 = int((~mask).sum()) + added
    g_before = [{n: gradient(s, gen) for n, s in shapes.items()} for _ in range(2)]
    new_rows = {n: torch.randn(s, generator=gen) for n, s in model_shapes(added).items()}
    g_after = [{n: gradient(s, gen) for n, s in model_shapes(n2).items()} for _ in range(2)]
    return params, mask, g_before, new_rows, g_after


def run_surgery(cls, device, dtype, reload_into=None):
    params, mask, g_before, new_rows, g_after = surgery_inputs()
    model = StandIn(cls, params, device, dtype)
    for g in g_before:
        model.step(g)
    model.prune(mask)
    model.extend(new_rows)
    if reload_into is not None:                                 # checkpoint: continue in another optimizer class from the state_dict
        twin = StandIn(reload_into, {n: p.detach() for n, p in zip(NAMES, model.params())}, device, dtype)
        twin.optimizer.load_state_dict(model.optimizer.state_dict())
        model = twin
    for g in g_after:
        model.step(g)
    return snapshot(model.optimizer, model.params()), model


@functools.lru_cache(maxsize=None)
def surgery_references():
    return run_surgery(torch.optim.AdamW, DEV, torch.float32)[0], run_surgery(torch.optim.AdamW, "cpu", torch.float64)[0]


def test_state_surgery_prune_and_extend():
    t32, r64 = surgery_references()
    ours, model = run_surgery(optim.HipAdamW, DEV, torch.float32)
    assert ours[0]["p"].shape == r64[0]["p"].shape
    print("largest ratio:", check_rule("surgery", ours, t32, r64))
    assert all(int(model.optimizer.state[p]["step"]) == 4 for p in model.params())


@pytest.mark.parametrize("first, then", [(torch.optim.AdamW, optim.HipAdamW), (optim.HipAdamW, torch.optim.AdamW)])
def test_state_dict_moves_between_torch_and_hip(first, then):
    t32, r64 = surgery_references()
    ours, model = run_surgery(first, DEV, torch.float32, reload_into=then)
    assert type(model.optimizer) is then
    st = model.optimizer.state[model.params()[0]]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 4.0
    print("largest ratio:", check_rule(f"{first.__name__} -> {then.__name__}", ours, t32, r64))


# ---- 7. drop-in -----------------------------------------------------------------------------------------------------------------

def test_drop_in_hook_and_data_parallel_wrapper():
    from lightgaussian_amd import dp
    params0, grads, _ = model_inputs(1.0)

    def make():
        ps = {n: torch.nn.Parameter(t.to(DEV).clone()) for n, t in params0.items()}
        return ps, torch.optim.AdamW([{"params": [ps[n]], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=EPS)

    orig = torch.optim.Adam.__init__
    lg_run.hip_adam(True)
    try:
        ps, opt = make()
        explicit = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3, device=DEV))], foreach=True)
    finally:
        lg_run.hip_adam(False)
    assert torch.optim.Adam.__init__ is orig
    assert isinstance(opt, torch.optim.AdamW) and isinstance(opt, optim._HipStep) and type(opt).__mro__[2] is torch.optim.AdamW
    assert not isinstance(explicit, optim._HipStep)             # an explicit foreach / fused is the caller's choice
    calls = []
    opt.register_step_post_hook(lambda o, a, k: calls.append("post"))
    opt.register_step_pre_hook(lambda o, a, k: calls.append("pre"))
    dp.wrap_optimizer(opt)
    optim.set_profile(True)
    _lib.profile_reset()
    try:
        for k in range(2):
            for n in NAMES:
                ps[n].grad = grads[k][n].to(DEV)
            loss = opt.step(lambda: torch.tensor(3.0))
        n = launches()
    finally:
        optim.set_profile(False)
    assert n == 2 and calls == ["pre", "post"] * 2 and float(loss) == 3.0
    assert int(opt.state[ps["xyz"]]["step"]) == 2
    _, plain = make()
    assert type(plain) is torch.optim.AdamW


# ---- 8. compressed model --------------------------------------------------------------------------------------------------------

def test_compressed_model_sees_every_step():
    import vq_finetune_common as vc
    from common import syn
    from lightgaussian_amd import vectree
    from lightgaussian_amd.gaussian_renderer import render

    packed = vc.packed_random(2000, 2, 0.6, K=64, seed=5)
    W = H = 64
    bg = torch.tensor([0.3, 0.2, 0.1], device=DEV)
    cams = [syn.orbit_camera(k, 8, W, H).to(DEV) for k in range(3)]
    with torch.no_grad():
        teacher = vc.scene(2500, 1, seed=41, scale=0.05).to(DEV)
        targets = [render(c, teacher, syn.PipelineParams(), bg)["render"].clone() for c in cams]

    def make(cls):
        tc = vectree.CompressedGaussians.from_packed(packed, DEV).trainable(("rows", "xyz"))
        return tc, cls(tc.parameters(), lr=2e-3)

    ours, opt_o = make(optim.HipAdam)
    twin, opt_t = make(torch.optim.Adam)
    r_rows = ours._rows.detach().double().cpu().requires_grad_(True)
    r_xyz = ours._xyz.detach().double().cpu().requires_grad_(True)
    opt_r = torch.optim.Adam([r_rows, r_xyz], lr=2e-3)
    d = ours.sh_dim
    for cam, target in zip(cams, targets):
        # the gradients of OUR model's render feed all three optimizers: the comparison is of the step alone
        opt_o.zero_grad(set_to_none=True)
        vc.l1(render(cam, ours, syn.PipelineParams(), bg)["render"], target).backward()
        g_rows, g_xyz = ours._rows.grad.detach().clone(), ours._xyz.grad.detach().clone()
        opt_o.step()
        twin._rows.grad, twin._xyz.grad = g_rows.clone(), g_xyz.clone()
        opt_t.step()
        r_rows.grad, r_xyz.grad = g_rows.double().cpu(), g_xyz.double().cpu()
        opt_r.step()
        with torch.no_grad():
            ours.colors(cam.camera_center)                      # the forward's resync, triggered by _rows._version alone
        assert same_bits(ours.rows[:, :d], ours._rows.detach().half())
    snap = lambda o, ps: [dict(p=p.detach(), m=o.state[p]["exp_avg"], v=o.state[p]["exp_avg_sq"]) for p in ps]   # noqa: E731
    print("largest ratio:", check_rule("compressed", snap(opt_o, [ours._rows, ours._xyz]), snap(opt_t, [twin._rows, twin._xyz]),
                                       snap(opt_r, [r_rows, r_xyz])))
