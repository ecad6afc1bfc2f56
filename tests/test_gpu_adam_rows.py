"""-m gpu: lg_adam_step_rows through HipAdam / HipAdamW.step(visible=): the Adam step over the rows a byte mask names.

Reference by composition.  S = the state (p, exp_avg, exp_avg_sq, step) before a step, g its gradient, D = the DENSE step from S with g.
The masked step must give   R = where(row visible, D, S)   on p, exp_avg and exp_avg_sq.  With D from our own dense kernel
(HipAdam / HipAdamW without visible=) the comparison is bit for bit; with D from torch's optimizers (T32 float32 on the GPU, R64 on
float64 CPU copies) it is the parity rule of tests/test_gpu_adam.py:

    max|ours - R64| <= 4 max|T32 - R64| + 2^-23 max|R64|

Over several steps R is composed step by step: the dense optimizer starts every step from the masked state of the step before."""
import functools
import math

import numpy as np
import pytest
import torch

from lightgaussian_amd import _lib, dp, optim, run as lg_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAN, MAXT = optim.SPAN, optim.MAX_TENSORS
EPS = 1e-15                                 # training_setup's
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)
KEYS = ("p", "m", "v")


def model_shapes(N):
    return dict(xyz=(N, 3), f_dc=(N, 1, 3), f_rest=(N, 15, 3), opacity=(N, 1), scaling=(N, 3), rotation=(N, 4))


def bits(t):       # (not common.bits: an integer torch view of any element size, on the device)
    return t.detach().contiguous().view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def gradient(shape, gen):
    """Rows scaled log-normally (sigma 4 in log space), magnitudes no smaller than 1e-12, every third row exactly zero."""
    g = torch.randn(shape, generator=gen)
    g = g * torch.exp(4.0 * torch.randn((shape[0],) + (1,) * (len(shape) - 1), generator=gen))
    g = torch.where(g < 0, -1.0, 1.0) * g.abs().clamp_min(1e-12)
    g[0::3] = 0.0
    return g


def launches(name):
    torch.cuda.synchronize()
    return _lib.profile_read().get(name, (0.0, 0))[1]


def state_of(opt, p):
    st = opt.state[p]
    return dict(p=p.detach().clone(), m=st["exp_avg"].detach().clone(), v=st["exp_avg_sq"].detach().clone())


def zero_state(p):
    return {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}


def rowsel(mask, t):
    """mask [N] (any non-zero byte = visible) broadcast over the trailing dimensions of t [N, ...]."""
    return (mask != 0).view((-1,) + (1,) * (t.dim() - 1))


class DenseTwin:
    """A dense optimizer over clones that is set to a given state before each of its steps: D of the module docstring."""

    def __init__(self, cls, params, groups, device=DEV, dtype=torch.float32, **kw):
        self.ps = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in params]
        self.opt = cls([dict(g, params=[q]) for g, q in zip(groups, self.ps)], **kw)
        for q in self.ps:
            self.opt.state[q] = zero_state(q)

    def step_from(self, states, grads):
        """states: per tensor {"p", "m", "v"} to start from (None: where this optimizer stands); returns the dense result D per tensor."""
        with torch.no_grad():
            for q, s, g in zip(self.ps, states, grads):
                st = self.opt.state[q]
                if s is not None:
                    q.copy_(s["p"]); st["exp_avg"].copy_(s["m"]); st["exp_avg_sq"].copy_(s["v"])
                q.grad = g.to(device=q.device, dtype=q.dtype)
        self.opt.step()
        return [state_of(self.opt, q) for q in self.ps]


def compose(S, D, mask):
    return {k: torch.where(rowsel(mask.to(S[k].device), S[k]), D[k], S[k]) for k in KEYS}


# ---- 1. bit identity with the dense kernel -----------------------------------------------------------------------------------------

WIDTHS = (1, 2, 3, 4, 5, 7, 45, 48)
TARGETS = (SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3)
MASK_KINDS = ("zero", "one", "alternating", "first", "last", "straddle", "random25", "bytes")


def rows_for(w):
    return sorted({max(1, round(t / w)) for t in TARGETS} | {1})


def make_mask(kind, n, w, gen):
    m = torch.zeros(n, dtype=torch.uint8)
    if kind == "one":
        m[:] = 1
    elif kind == "alternating":
        m[0::2] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[n - 1] = 1
    elif kind == "straddle":                # the row that holds the first element of the second span (it starts in the first when w does not divide SPAN)
        m[min(SPAN // w, n - 1)] = 1
    elif kind == "random25":
        m = (torch.rand(n, generator=gen) < 0.25).to(torch.uint8)
    elif kind == "bytes":                   # any non-zero byte is "visible"
        m = torch.tensor([0, 2, 0xFF, 0], dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=gen)]
    return m


@pytest.mark.parametrize("first_kind", range(len(MASK_KINDS)))
@pytest.mark.parametrize("kind, wd", [("Adam", 0.1), ("AdamW", 0.01)])
def test_bit_identity_with_the_dense_kernel(kind, wd, first_kind):
    """[N, w] for every width and every N whose N w lands on SPAN - 1, SPAN, SPAN + 1, 2 SPAN + 3 (rounded to whole rows) and N = 1;
    three steps, the mask kind changing every step (first_kind, +1, +2), each tensor with its own optimizer (one mask length each)."""
    gen = torch.Generator().manual_seed(100 + first_kind)
    cls, kw = getattr(optim, "Hip" + kind), dict(lr=2e-3, eps=1e-8, weight_decay=wd)
    for w in WIDTHS:
        for n in rows_for(w):
            p = torch.nn.Parameter(torch.randn(n, w, generator=gen).to(DEV))
            ours = cls([p], **kw)
            twin = DenseTwin(cls, [p], [{}], **kw)
            S = dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p))
            for s in range(3):
                mk = MASK_KINDS[(first_kind + s) % len(MASK_KINDS)]
                mask = make_mask(mk, n, w, gen).to(DEV)
                g = gradient((n, w), gen).to(DEV)
                R = compose(S, twin.step_from([S], [g])[0], mask)
                p.grad = g
                ours.step(visible=mask)
                got = state_of(ours, p)
                for k in KEYS:
                    assert same_bits(got[k], R[k]), f"{kind} [{n}, {w}] step {s} mask {mk}: {k} differs from where(visible, dense, before)"
                S = got
            assert int(ours.state[p]["step"]) == 3


@pytest.mark.parametrize("kind, wd", [("Adam", 0.1), ("AdamW", 0.01)])
def test_many_tensors_in_one_step(kind, wd):
    """More than 2 MAX_TENSORS tensors [N, w] under one mask in one step (and one without elements): ceil(nonempty / MAX_TENSORS) launches
    per step, every tensor bit-identical to the composition.  N = 1367: rows straddle span boundaries for every width but 1, 2, 4."""
    gen = torch.Generator().manual_seed(5)
    n, steps = 1367, 3
    widths = list(WIDTHS) * 3 + [0]
    assert len(widths) - 1 > 2 * MAXT
    cls, kw = getattr(optim, "Hip" + kind), dict(lr=2e-3, eps=1e-8, weight_decay=wd)
    ps = [torch.nn.Parameter(torch.randn(n, w, generator=gen).to(DEV)) for w in widths]
    ours = cls(ps, **kw)
    twin = DenseTwin(cls, ps, [{} for _ in ps], **kw)
    S = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p)) for p in ps]
    optim.set_profile(True)
    _lib.profile_reset()
    try:
        for s in range(steps):
            mask = make_mask(("random25", "alternating", "bytes")[s], n, 1, gen).to(DEV)
            gs = [gradient((n, w), gen).to(DEV) if w else torch.zeros(n, 0, device=DEV) for w in widths]
            before = launches("adam_rows")
            D = twin.step_from(S, gs)
            assert launches("adam_rows") == before              # the dense twin goes through lg_adam_step
            for p, g in zip(ps, gs):
                p.grad = g
            ours.step(visible=mask)
            assert launches("adam_rows") - before == math.ceil((len(widths) - 1) / MAXT)
            got = [state_of(ours, p) for p in ps]
            for w, a, s_, d in zip(widths, got, S, D):
                r = compose(s_, d, mask)
                for k in KEYS:
                    assert same_bits(a[k], r[k]), f"{kind} [{n}, {w}] step {s}: {k}"
            S = got
    finally:
        optim.set_profile(False)


# ---- 2. guards and unread gradients ------------------------------------------------------------------------------------------------

PAD = 64                                    # floats of sentinel on either side (a multiple of 4: the view keeps the buffer's alignment)
SENTINEL = 0x7FC12345                       # a NaN with a payload: any arithmetic on it, and any stray store, shows
MASK_PAD, MASK_GUARD = 64, 0xA5             # bytes around the mask, non-zero: a mask byte read outside the mask would step a masked-out row


def guarded(values, shift):
    buf = torch.full((values.numel() + 2 * PAD + 1,), 0.0, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    view = buf[PAD + shift:PAD + shift + values.numel()]
    view.copy_(values.to(DEV).reshape(-1))
    return buf, view.view(values.shape)


def guards_intact(buf, shift, n):
    b = buf.view(torch.int32).cpu()
    return bool((b[:PAD + shift] == SENTINEL).all()) and bool((b[PAD + shift + n:] == SENTINEL).all())


def test_guards_mask_alignment_and_unread_gradients():
    """p, g, m, v inside sentinel-guarded buffers, two tensors with a pointer one float off the 16-byte grid (the scalar path), the mask
    at offsets 0..3 from a 16-byte boundary inside guard bytes, and the gradient rows outside the mask filled with the NaN sentinel."""
    gen = torch.Generator().manual_seed(21)
    n = 1025
    # (width, which of p / g / m / v starts one float into its storage)
    cases = [(1, ""), (3, ""), (4, ""), (45, ""), (48, ""), (45, "p"), (7, "v")]
    bufs, ps = [], []
    for w, mis in cases:
        e = {}
        for key in ("p", "g", "m", "v"):
            shift = 1 if key == mis else 0
            e[key] = guarded(torch.randn(n, w, generator=gen) if key == "p" else torch.zeros(n, w), shift) + (shift,)
            assert e[key][1].data_ptr() % 16 == 4 * shift
        bufs.append(e)
        ps.append(e["p"][1].requires_grad_(True))
    opt = optim.HipAdamW([{"params": [p], "lr": 1e-3 * (1 + k)} for k, p in enumerate(ps)], lr=0.0, eps=EPS, weight_decay=0.01)
    for p, e in zip(ps, bufs):
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": e["m"][1], "exp_avg_sq": e["v"][1]}
        p.grad = e["g"][1]
    nan = torch.full((1,), 0.0).view(torch.int32).fill_(SENTINEL).view(torch.float32).to(DEV)
    for off in range(4):
        mbuf = torch.full((n + 2 * MASK_PAD,), MASK_GUARD, dtype=torch.uint8, device=DEV)
        assert mbuf.data_ptr() % 16 == 0
        mask = mbuf[MASK_PAD + off:MASK_PAD + off + n]
        mask.copy_((torch.rand(n, generator=gen) < 0.5).to(torch.uint8))
        assert mask.data_ptr() % 16 == off and mask.is_contiguous()
        mask_before = mbuf.clone()
        before = []
        for (w, _), e in zip(cases, bufs):
            g = gradient((n, w), gen).to(DEV)
            e["g"][1].copy_(torch.where(rowsel(mask, g), g, nan))
            before.append({k: e[k][1].detach().clone() for k in KEYS})
        opt.step(visible=mask)
        torch.cuda.synchronize()
        assert torch.equal(mbuf, mask_before)
        for (w, mis), e, b in zip(cases, bufs, before):
            for key in ("p", "g", "m", "v"):
                assert guards_intact(e[key][0], e[key][2], n * w), f"[{n}, {w}] {mis} mask offset {off}: the sentinel around {key} was overwritten"
            for k in KEYS:
                now = e[k][1].detach()
                assert not torch.isnan(now).any(), f"[{n}, {w}] {mis} mask offset {off}: NaN in {k} (a gradient outside the mask was consumed)"
                sel = rowsel(mask, now).expand_as(now)
                assert torch.equal(bits(now)[~sel], bits(b[k])[~sel]), f"[{n}, {w}] {mis} mask offset {off}: a masked-out row of {k} changed"
            seen = rowsel(mask, e["m"][1]).expand_as(e["m"][1]) & (e["g"][1].detach() != 0)
            assert bool((bits(e["m"][1])[seen] != bits(b["m"])[seen]).any())      # and the step did happen in the rows it names
    assert all(int(opt.state[p]["step"]) == 4 for p in ps)


# ---- 3. independent of our dense kernel --------------------------------------------------------------------------------------------

STEPS3 = 4


@functools.lru_cache(maxsize=None)
def model_inputs():
    gen = torch.Generator().manual_seed(1234)
    shapes = model_shapes(1025)
    params = {n: torch.randn(s, generator=gen) for n, s in shapes.items()}
    grads = [{n: gradient(s, gen) for n, s in shapes.items()} for _ in range(STEPS3)]
    masks = [torch.rand(1025, generator=gen) < 0.4 for _ in range(STEPS3)]
    return params, grads, masks


def run_model_torch(device, dtype):
    """torch.optim.AdamW composed with the masks: after its dense step, the rows outside the mask get their earlier values back."""
    params0, grads, masks = model_inputs()
    ps = {n: torch.nn.Parameter(t.to(device=device, dtype=dtype).clone()) for n, t in params0.items()}
    opt = torch.optim.AdamW([{"params": [ps[n]], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=EPS, weight_decay=0.01)
    for n in NAMES:
        opt.state[ps[n]] = zero_state(ps[n])
    for k in range(STEPS3):
        S = [state_of(opt, ps[n]) for n in NAMES]
        for n in NAMES:
            ps[n].grad = grads[k][n].to(device=device, dtype=dtype)
        opt.step()
        with torch.no_grad():
            for n, s in zip(NAMES, S):
                st = opt.state[ps[n]]
                for t, key in ((ps[n], "p"), (st["exp_avg"], "m"), (st["exp_avg_sq"], "v")):
                    t.copy_(torch.where(rowsel(masks[k].to(device), t), t, s[key]))
    return [state_of(opt, ps[n]) for n in NAMES]


def test_model_shapes_against_torch():
    params0, grads, masks = model_inputs()
    t32, r64 = run_model_torch(DEV, torch.float32), run_model_torch("cpu", torch.float64)
    ps = {n: torch.nn.Parameter(t.to(DEV).clone()) for n, t in params0.items()}
    opt = optim.HipAdamW([{"params": [ps[n]], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=EPS, weight_decay=0.01)
    for k in range(STEPS3):
        for n in NAMES:
            ps[n].grad = grads[k][n].to(DEV)
        opt.step(visible=masks[k].to(DEV))
    ours = [state_of(opt, ps[n]) for n in NAMES]
    worst = 0.0
    for name, o, t, r in zip(NAMES, ours, t32, r64):
        for key in KEYS:
            ref = r[key].double().cpu()
            eo = (o[key].double().cpu() - ref).abs().max().item()
            et = (t[key].double().cpu() - ref).abs().max().item()
            bound = 4.0 * et + 2.0 ** -23 * ref.abs().max().item()
            ratio = eo / et if et > 0 else (0.0 if eo == 0 else math.inf)
            print(f"{name} {key}: ours {eo:.3e} T32 {et:.3e} ratio {ratio:.3f}")
            assert math.isfinite(eo) and eo <= bound, f"{name} {key}: |ours - R64| {eo:.3e} > bound {bound:.3e} (T32 {et:.3e})"
            if et > 0:
                worst = max(worst, ratio)
    print("largest ratio:", worst)


# ---- 4. mixed call -----------------------------------------------------------------------------------------------------------------

def test_mixed_masked_and_dense_entries_in_one_launch():
    gen = torch.Generator().manual_seed(8)
    n, k_rows = 1500, 97
    shapes = [(n, 3), (n, 15, 3), (k_rows, 48)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in shapes]
    kw = dict(lr=1e-3, eps=EPS, weight_decay=0.01)
    ours = optim.HipAdamW(ps, **kw)
    twin = DenseTwin(optim.HipAdamW, ps, [{} for _ in ps], **kw)
    S = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p)) for p in ps]
    optim.set_profile(True)
    _lib.profile_reset()
    try:
        for s in range(2):
            mask = (torch.rand(n, generator=gen) < 0.5).to(DEV)
            gs = [gradient(sh, gen).to(DEV) for sh in shapes]
            D = twin.step_from(S, gs)
            for p, g in zip(ps, gs):
                p.grad = g
            ours.step(visible=mask)
            got = [state_of(ours, p) for p in ps]
            for i in range(2):
                r = compose(S[i], D[i], mask)
                assert all(same_bits(got[i][k], r[k]) for k in KEYS), shapes[i]
                assert not all(same_bits(got[i][k], D[i][k]) for k in KEYS)         # (the mask did something)
            assert all(same_bits(got[2][k], D[2][k]) for k in KEYS), "the [K, 48] tensor is a dense entry: bit-identical to a dense step"
            S = got
        assert launches("adam_rows") == 2 and launches("adam") == 2                # one launch per step, ours and the twin's
    finally:
        optim.set_profile(False)


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors_move_nothing():
    gen = torch.Generator().manual_seed(9)
    n = 300

    def fresh(dtype=torch.float32, wrap=False, **kw):
        p = torch.nn.Parameter(torch.randn(n, 3, generator=gen).to(device=DEV, dtype=dtype))
        opt = optim.HipAdamW([p], lr=1e-2, **kw)
        if not kw and dtype == torch.float32:
            p.grad = torch.randn(n, 3, generator=gen).to(DEV)
            opt.step()                                          # a state to keep: exp_avg, exp_avg_sq, step = 1
        p.grad = torch.randn(n, 3, generator=gen).to(device=DEV, dtype=dtype)
        if wrap:
            dp.wrap_optimizer(opt)
        return p, opt

    good = torch.rand(n, generator=gen).to(DEV) < 0.5
    cases = [
        ("wrong dtype", RuntimeError, dict(), good.float()),
        ("2-D", RuntimeError, dict(), good.view(n, 1)),
        ("non-contiguous", RuntimeError, dict(), torch.stack([good, good], dim=1)[:, 0]),
        ("CPU mask", RuntimeError, dict(), good.cpu()),
        ("no parameter with N rows", ValueError, dict(), torch.ones(n + 1, dtype=torch.bool, device=DEV)),
        ("amsgrad", RuntimeError, dict(amsgrad=True), good),
        ("float64", RuntimeError, dict(dtype=torch.float64), good),
        ("dp.wrap_optimizer", RuntimeError, dict(wrap=True), good),
    ]
    for label, exc, kw, mask in cases:
        assert mask.shape[0] in (n, n + 1)
        p, opt = fresh(**kw)
        before_p = p.detach().clone()
        before = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state.get(p, {}).items()}
        with pytest.raises(exc):
            opt.step(visible=mask)
        assert same_bits(p, before_p), label
        now = opt.state.get(p, {})
        assert set(now) == set(before), label
        for k, v in before.items():
            assert same_bits(now[k], v), f"{label}: state[{k}] moved"
    # the wrapped optimizer still takes its dense step
    p, opt = fresh(wrap=True)
    opt.step()
    assert int(opt.state[p]["step"]) == 2


# ---- 6. plumbing -------------------------------------------------------------------------------------------------------------------

def run_plumbing(stream=None, visible=True, cls=None):
    params0, grads, masks = model_inputs()
    ps = {n: torch.nn.Parameter(t.to(DEV).clone()) for n, t in params0.items()}
    gs = [{n: g.to(DEV) for n, g in step.items()} for step in grads]
    ms = [m.to(DEV) for m in masks]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        opt = (cls or optim.HipAdamW)([{"params": [ps[n]], "lr": LRS[n], "name": n} for n in NAMES], lr=0.0, eps=EPS)
        for k in range(STEPS3):
            for n in NAMES:
                ps[n].grad = gs[k][n]
            if visible is True:
                opt.step(visible=ms[k])
            elif visible is None:
                opt.step(visible=None)
            else:
                opt.step()
        out = [state_of(opt, ps[n]) for n in NAMES]
    if stream is not None:
        stream.synchronize()
    return out, opt, ps


def test_visible_none_is_the_dense_step():
    a, _, _ = run_plumbing(visible=None)
    b, _, _ = run_plumbing(visible=False)
    optim.set_profile(True)
    _lib.profile_reset()
    try:
        run_plumbing(visible=None)
        assert launches("adam") == STEPS3 and launches("adam_rows") == 0
    finally:
        optim.set_profile(False)
    for x, y in zip(a, b):
        assert all(same_bits(x[k], y[k]) for k in KEYS)


def test_versions_hooks_state_dict_and_side_stream():
    first, opt, ps = run_plumbing()
    # version counters
    p = ps["xyz"]
    st = opt.state[p]
    seen = [(p._version, st["exp_avg"]._version, st["exp_avg_sq"]._version)]
    calls = []
    opt.register_step_pre_hook(lambda o, a, k: calls.append(("pre", "visible" in k)))
    opt.register_step_post_hook(lambda o, a, k: calls.append(("post", "visible" in k)))
    mask = torch.ones(p.shape[0], dtype=torch.bool, device=DEV)
    opt.step(visible=mask)
    seen.append((p._version, st["exp_avg"]._version, st["exp_avg_sq"]._version))
    assert all(b > a for a, b in zip(*seen)), seen
    assert calls == [("pre", True), ("post", True)]
    y = (p * p).sum()
    opt.step(visible=mask)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()
    # state_dict into torch's own AdamW and on from there
    twin_ps = [torch.nn.Parameter(ps[n].detach().clone()) for n in NAMES]
    twin = torch.optim.AdamW([{"params": [q], "lr": LRS[n], "name": n} for n, q in zip(NAMES, twin_ps)], lr=0.0, eps=EPS)
    twin.load_state_dict(opt.state_dict())
    ts = twin.state[twin_ps[0]]
    assert ts["step"].device.type == "cpu" and ts["step"].dtype == torch.float32 and float(ts["step"]) == STEPS3 + 2
    assert same_bits(ts["exp_avg"], st["exp_avg"]) and same_bits(ts["exp_avg_sq"], st["exp_avg_sq"])
    for q in twin_ps:
        q.grad = torch.ones_like(q)
    twin.step()
    assert float(ts["step"]) == STEPS3 + 3
    # a side stream, with unrelated work in flight on the default stream
    side = torch.cuda.Stream()
    busy = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):
        busy = (busy @ busy).clamp_(-1.0, 1.0)
    streamed, _, _ = run_plumbing(stream=side)
    torch.cuda.synchronize()
    for a, b in zip(first, streamed):
        assert all(same_bits(a[k], b[k]) for k in KEYS)


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------

E2E_N, E2E_W, E2E_SEED, E2E_ITERS = 2000, 64, 7, 4
ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")


def e2e_scene():
    from common import syn
    g = syn.make_gaussians(E2E_N, sh_degree=3, seed=E2E_SEED, log_scale_mean=math.log(0.05))
    cams = [syn.orbit_camera(0, 8, E2E_W, E2E_W, fovx_deg=30.0, target=(tx, 0.0, 0.0)) for tx in (-1.5, 1.5)]
    return g, cams


def test_end_to_end_visibility_of_the_render():
    import common
    from common import syn
    from lightgaussian_amd.gaussian_renderer import render
    from oracle import oracle
    g, cams = e2e_scene()
    seen = [oracle.forward(**common.scene_kwargs(g, c, E2E_W, E2E_W)).radii > 0 for c in cams]
    for s in seen:
        assert 0.2 <= float(np.mean(s)) <= 0.8, float(np.mean(s))
    assert int((seen[0] & ~seen[1]).sum()) > 0 and int((seen[1] & ~seen[0]).sum()) > 0
    bg = torch.tensor([0.3, 0.2, 0.1], device=DEV)
    pipe = syn.PipelineParams()
    dcams = [c.to(DEV) for c in cams]
    with torch.no_grad():
        teacher = syn.make_gaussians(E2E_N, sh_degree=3, seed=E2E_SEED + 1, log_scale_mean=math.log(0.05)).to(DEV)
        targets = [render(c, teacher, pipe, bg)["render"].clone() for c in dcams]

    def loop(make_opt, render_fn, explicit):
        pc = g.to(DEV).requires_grad_(True)
        params = [getattr(pc, ATTRS[n]) for n in NAMES]
        groups = [{"lr": LRS[n] * 20.0, "name": n} for n in NAMES]
        opt = make_opt([dict(gr, params=[p]) for gr, p in zip(groups, params)])
        twin = DenseTwin(optim.HipAdamW, params, groups, lr=0.0, eps=EPS) if explicit else None
        fracs = []
        for it in range(E2E_ITERS):
            opt.zero_grad(set_to_none=True)
            pkg = render_fn(dcams[it % 2], pc, pipe, bg)
            (pkg["render"] - targets[it % 2]).abs().mean().backward()
            if not explicit:
                opt.step()
                continue
            vis = pkg["visibility_filter"].clone()
            fracs.append(float(vis.float().mean()))
            S = [state_of(opt, p) if opt.state.get(p) else dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p)) for p in params]
            D = twin.step_from(S, [p.grad for p in params])
            opt.step(visible=pkg["visibility_filter"])
            for n, p, s, d in zip(NAMES, params, S, D):
                got, r = state_of(opt, p), compose(s, d, vis)
                out = ~rowsel(vis, p).expand_as(p)
                for k in KEYS:
                    assert torch.equal(bits(got[k])[out], bits(s[k])[out]), f"iteration {it} {n} {k}: a row outside the view moved"
                    assert same_bits(got[k], r[k]), f"iteration {it} {n} {k}: rows inside the view differ from the dense step"
                assert not same_bits(got["p"], s["p"]), f"iteration {it} {n}: nothing moved"
        return [state_of(opt, p) for p in params], fracs

    first, fracs = loop(lambda groups: optim.HipAdamW(groups, lr=0.0, eps=EPS), render, True)
    print("visible fraction per iteration:", fracs)
    assert all(0.2 <= f <= 0.8 for f in fracs)
    # the same loop as an unmodified trainer runs it under run.py --hip-adam=visible: torch's constructor, a plain step()
    before = dp.stats()
    lg_run.hip_adam(True, visible=True)
    try:
        second, _ = loop(lambda groups: torch.optim.AdamW(groups, lr=0.0, eps=EPS), lg_run.recording_render(), False)
    finally:
        lg_run.hip_adam(False)
    after = dp.stats()
    assert after["adam_dense_fallbacks"] - before["adam_dense_fallbacks"] == 0
    assert after["adam_visible_steps"] - before["adam_visible_steps"] == E2E_ITERS
    for n, a, b in zip(NAMES, first, second):
        for k in KEYS:
            assert same_bits(a[k], b[k]), f"{n} {k}: run.hip_adam(visible=True) differs from step(visible=visibility_filter)"
