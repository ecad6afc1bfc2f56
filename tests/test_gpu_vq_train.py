"""-m gpu: the fused VecTree training step (lightgaussian_amd.vq.ema_update -> lg_vq_ema_step) against the golden vectors of the
reference's own vectree/vq.py (tests/golden/reference_vq_train.npz, written by make_golden_vq_train.py), plus what the design
promises beyond parity: bit-reproducibility, conservation, no n x K intermediate, errors, and the train_codebook loop.

Parity rule.  Indices must equal the reference's exactly (near-ties were removed by the maker).  cluster_size and embed are
compared with the stored float64 values; error per code row = max|got - f64| / max(row L-inf norm, tensor L-inf norm * 2^-20);
bound = 4 x the stored deviation of the reference's own float32 result from the same float64 values, floor 2^-22 (both are
float32 evaluations of one exact quantity that differ in summation order only).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import vq_train_common as vc
from lightgaussian_amd import _lib, vq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def _step(x, w, embed_pre, cs_pre, form3=True, **kw):
    """One ema_update on fresh device copies of the pre-state: (ind, quant or None, embed, cluster_size) as numpy."""
    e, c = _dev(embed_pre), _dev(cs_pre)
    xd, wd = _dev(x), _dev(w)
    if form3:
        out = vq.ema_update(xd[None], e[None], c[None], weight=None if wd is None else wd.reshape(1, -1, 1), **kw)
    else:
        out = vq.ema_update(xd, e, c, weight=wd, **kw)
    ind, quant = out if isinstance(out, tuple) else (out, None)
    return ind.reshape(-1).cpu().numpy(), None if quant is None else quant.reshape(len(x), -1).cpu().numpy(), e.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("name", vc.CASES)
def test_golden_steps_of_the_reference(name):
    case = vc.load_case(np.load(vc.GOLD), name)
    failures = []
    for t, s in enumerate(case["steps"]):
        x = case["x"][s["keep"]]
        ind, quant, embed, cs = _step(x, s["w"], s["embed_pre"], s["cs_pre"], decay=vc.DECAY, eps=vc.EPS, return_quantized=True)
        err_e, err_c = vc.row_error(embed, s["embed_f64"]), vc.row_error(cs, s["cs_f64"])
        print(f"[vq_train golden] {name} step {t}: n={len(x)} d={case['d']} K={case['K']} index mismatches {int((ind != s['ind']).sum())} "
              f"embed err {err_e:.3g} (reference {s['dev_embed']:.3g}, bound {vc.bound(s['dev_embed']):.3g}) "
              f"cluster_size err {err_c:.3g} (reference {s['dev_cs']:.3g}, bound {vc.bound(s['dev_cs']):.3g})")
        if not np.array_equal(ind, s["ind"]):
            failures.append((t, "indices", int((ind != s["ind"]).sum())))
            continue
        if not np.array_equal(quant, s["embed_pre"][s["ind"]]):              # a gather of PRE-update values, bit for bit
            failures.append((t, "quantised rows"))
        if not err_e <= vc.bound(s["dev_embed"]):
            failures.append((t, "embed", err_e, vc.bound(s["dev_embed"])))
        if not err_c <= vc.bound(s["dev_cs"]):
            failures.append((t, "cluster_size", err_c, vc.bound(s["dev_cs"])))
    assert not failures, (name, failures)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bit_identical_run_to_run_across_streams_and_input_forms():
    case = vc.load_case(np.load(vc.GOLD), "deg2")
    s = case["steps"][1]
    x = case["x"][s["keep"]]
    i0, _, e0, c0 = _step(x, s["w"], s["embed_pre"], s["cs_pre"])
    i1, _, e1, c1 = _step(x, s["w"], s["embed_pre"], s["cs_pre"])
    i2, _, e2, c2 = _step(x, s["w"], s["embed_pre"], s["cs_pre"], form3=False)               # [n, d] / [K, d] / [K] / weight [n]
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        i3, _, e3, c3 = _step(x, s["w"], s["embed_pre"], s["cs_pre"])
    side.synchronize()
    for i, e, c in ((i1, e1, c1), (i2, e2, c2), (i3, e3, c3)):
        assert np.array_equal(i, i0) and _same(e, e0) and _same(c, c0)


def _heavy_case(n=80000, K=8192, d=27, seed=11):
    rng = np.random.default_rng(seed)
    embed = (rng.standard_normal((K, d)) * 0.3).astype(np.float32)
    x = (embed[rng.integers(0, K, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    x[::2] = x[0]                                                            # half the rows are copies of one point: one list of ~n / 2 rows
    w = np.exp(2.0 * rng.standard_normal(n)).astype(np.float32)              # heavy-tailed importance
    cs = (rng.random(K) * 10).astype(np.float32)
    return x, w, embed, cs


def test_full_size_skewed_lists_are_reproducible_and_within_the_summation_bound():
    """n = 80 000, K = 8192, d = 27 (vectree.py's training shape), one list of ~40 000 rows so that the chunk split and the
    ordered second step are exercised.  No reference deviation exists for this size; the bound is derived: an m-term float32
    sum in ANY order is within m * 2^-24 of the exact one relative to the sum of magnitudes, and the epilogue adds a handful of
    roundings:  |embed - f64| <= (m_c + 8) * 2^-24 * (|decay * embed_pre| + (1 - decay) * sum_i |w_i x_i| / smoothed_c),
    |cluster_size - f64| <= (m_c + 8) * 2^-24 * cluster_size."""
    x, w, embed_pre, cs_pre = _heavy_case()
    i0, _, e0, c0 = _step(x, w, embed_pre, cs_pre)
    i1, _, e1, c1 = _step(x, w, embed_pre, cs_pre)
    assert np.array_equal(i0, i1) and _same(e0, e1) and _same(c0, c1)
    K = len(cs_pre)
    m = np.bincount(i0, minlength=K).astype(np.float64)
    assert m.max() >= len(x) // 2 and i0.min() >= 0 and i0.max() < K
    e64, c64, _, _ = vc.ema_step_f64(x, w, embed_pre, cs_pre, i0)
    wn = vc.normalised_weight64(w, len(x))
    mag = np.zeros_like(e64)
    np.add.at(mag, i0, np.abs(x.astype(np.float64)) * wn[:, None])
    total = c64.sum()
    smoothed = (c64 + vc.EPS) / (total + K * vc.EPS) * total
    u = (m + 8) * 2.0 ** -24
    bound_e = u[:, None] * (np.abs(vc.DECAY * embed_pre.astype(np.float64)) + (1 - vc.DECAY) * mag / smoothed[:, None])
    bound_c = u * np.abs(c64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio_e = np.nan_to_num(np.abs(e0 - e64) / bound_e, nan=0.0)
        ratio_c = np.nan_to_num(np.abs(c0 - c64) / bound_c, nan=0.0)
    print(f"[vq_train full size] longest list {int(m.max())} rows, codes used {int((m > 0).sum())}/{K}; worst |err| / bound: "
          f"embed {ratio_e.max():.3g}, cluster_size {ratio_c.max():.3g}; embed row error {vc.row_error(e0, e64):.3g}, "
          f"cluster_size row error {vc.row_error(c0, c64):.3g}")
    assert np.isfinite(e0).all() and np.isfinite(c0).all()
    assert (np.abs(e0 - e64) <= bound_e).all(), float(ratio_e.max())
    assert (np.abs(c0 - c64) <= bound_c).all(), float(ratio_c.max())


def test_conservation_and_codes_without_rows():
    rng = np.random.default_rng(3)
    n, K, d = 6000, 300, 27
    embed_pre = (rng.standard_normal((K, d)) * 0.3).astype(np.float32)
    embed_pre[200:] += 50.0                                                   # a third of the codes is out of reach: no rows
    x = (embed_pre[rng.integers(0, 200, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    w = np.exp(rng.standard_normal(n)).astype(np.float32)
    zeros = np.zeros(K, dtype=np.float32)
    decay32, rest32 = np.float32(vc.DECAY), np.float32(1.0 - vc.DECAY)
    # weighted, from an all-zero cluster_size: the new sizes sum to n, so cluster_size sums to (1 - decay) * n
    ind, _, embed, cs = _step(x, w, embed_pre, zeros)
    m = np.bincount(ind, minlength=K)
    slack = float(((m + 8) * 2.0 ** -24 * cs.astype(np.float64)).sum())
    print(f"[vq_train conservation] sum(cluster_size) = {cs.astype(np.float64).sum():.9g}, (1 - decay) n = {(1 - vc.DECAY) * n:.9g}, slack {slack:.3g}")
    assert abs(cs.astype(np.float64).sum() - (1 - vc.DECAY) * n) <= slack
    # unweighted: cluster_size / (1 - decay) rounds to the exact row counts
    ind_u, _, embed_u, cs_u = _step(x, None, embed_pre, zeros)
    assert np.array_equal(ind_u, ind)
    assert np.array_equal(np.rint(cs_u.astype(np.float64) / (1 - vc.DECAY)).astype(np.int64), m)
    assert np.array_equal(cs_u, rest32 * m.astype(np.float32))                # fl(0 * decay + fl(1 - decay) * count), no contraction
    # codes without rows end at exactly fl(decay * embed) and fl(decay * cluster_size)
    cs_pre = (rng.random(K) * 5 + 0.5).astype(np.float32)
    ind_r, _, embed_r, cs_r = _step(x, w, embed_pre, cs_pre)
    empty = np.nonzero(np.bincount(ind_r, minlength=K) == 0)[0]
    assert len(empty) >= 100
    assert _same(embed_r[empty], (decay32 * embed_pre)[empty]) and _same(cs_r[empty], (decay32 * cs_pre)[empty])
    assert _same(embed[empty], (decay32 * embed_pre)[empty]) and np.array_equal(cs[empty], zeros[empty])


def test_no_dense_intermediate_and_linear_scratch():
    lib = _lib.load()
    for n, K, d in ((80000, 8192, 27), (80000, 8192, 48), (1000, 65536, 3), (2000000, 256, 63)):
        b = lib.lg_vq_ema_scratch_bytes(n, K, d)
        assert 0 < b < 128 * n + 16 * K * (d + 2) + (1 << 20) + lib.lg_vq_scratch_bytes(K, d), (n, K, d, b)
    n, K, d = 80000, 8192, 27
    g = torch.Generator(device=DEV).manual_seed(0)
    embed = torch.randn(K, d, device=DEV, generator=g) * 0.3
    x = embed[torch.randint(0, K, (n,), device=DEV, generator=g)] + 0.05 * torch.randn(n, d, device=DEV, generator=g)
    w = torch.rand(n, device=DEV, generator=g) + 0.01
    cs = torch.zeros(K, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    ind, quant = vq.ema_update(x, embed, cs, weight=w, return_quantized=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(DEV) - before
    print(f"[vq_train memory] peak growth over one step at ({n}, {K}, {d}): {grown / 2 ** 20:.1f} MiB (n * K bytes = {n * K / 2 ** 20:.0f} MiB)")
    assert grown < n * K
    assert ind.shape == (n,) and ind.dtype == torch.int64 and quant.shape == (n, d)
    assert torch.isfinite(embed).all() and abs(float(cs.sum()) - (1 - 0.8) * n) < 1e-3 * n


def test_errors():
    e, c = torch.zeros(8, 27, device=DEV), torch.zeros(8, device=DEV)
    x = torch.zeros(20, 27, device=DEV)
    with pytest.raises(RuntimeError):
        vq.ema_update(torch.zeros(20, 27), torch.zeros(8, 27), torch.zeros(8))
    with pytest.raises(RuntimeError):
        vq.ema_update(x, e, torch.zeros(8))
    with pytest.raises(ValueError):
        vq.ema_update(x, torch.zeros(8, 26, device=DEV), c)
    with pytest.raises(ValueError):
        vq.ema_update(x, e, torch.zeros(9, device=DEV))
    with pytest.raises(ValueError):
        vq.ema_update(x, e, c, weight=torch.ones(19, device=DEV))
    with pytest.raises(ValueError):
        vq.ema_update(torch.zeros(0, 27, device=DEV), e, c)
    with pytest.raises(ValueError):
        vq.ema_update(x, e.double(), c)
    with pytest.raises(Exception):
        vq.ema_update(torch.zeros(20, 64, device=DEV), torch.zeros(8, 64, device=DEV), c)
    assert torch.equal(e, torch.zeros_like(e)) and torch.equal(c, torch.zeros_like(c))     # nothing was touched on the way


def _clustered(seed, N=20000, d=12, centres=64):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mu = torch.randn(centres, d, device=DEV, generator=g)
    feats = mu[torch.randint(0, centres, (N,), device=DEV, generator=g)] + 0.1 * torch.randn(N, d, device=DEV, generator=g)
    imp = torch.exp(torch.randn(N, device=DEV, generator=g))
    embed = (feats[torch.randperm(N, device=DEV, generator=g)[:centres]] + 0.05 * torch.randn(centres, d, device=DEV, generator=g)).contiguous()
    return feats, imp, embed


def test_train_codebook_improves_and_is_reproducible():
    runs = []
    for _ in range(2):
        feats, imp, embed = _clustered(7)
        cs = torch.zeros(embed.shape[0], device=DEV)
        errors = vq.train_codebook(feats, imp, embed, cs, iterations=20, chunk=4000, k_expire=2,
                                   generator=torch.Generator(device=DEV).manual_seed(5))
        runs.append((errors.cpu().numpy(), embed.cpu().numpy(), cs.cpu().numpy()))
    err = runs[0][0]
    print("[vq_train train_codebook] weighted quantisation error per iteration:", " ".join(f"{v:.4f}" for v in err))
    assert np.isfinite(err).all() and err.shape == (20,)
    assert err[-1] < err[1]                                                   # err[1] = the codebook after the first step
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))
