"""Shared by the tests of the fused VecTree training step (lightgaussian_amd.vq.ema_update): the float64 restatement of one
step of the reference's EuclideanCodebook.forward in training mode, the error measure of the parity tests, and the reader of
tests/golden/reference_vq_train.npz (written by tests/golden/make_golden_vq_train.py from the reference's own module)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reference_vq_train.npz")
CASES = ("deg2", "deg3", "tiny", "unweighted", "wide")       # (n, d, K) in the file's <case>_meta
X_SCALE = 64.0                                                 # rows are stored as int8 multiples of 1 / 64 (exact in float32)
DECAY, EPS = 0.8, 1e-5


def normalised_weight64(w, n):
    """w * n / sum(w) in float64 (ones when w is None)."""
    if w is None:
        return np.ones(n, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    return w * n / w.sum()


def ema_step_f64(x, w, embed, cluster_size, ind, decay=DECAY, eps=EPS):
    """One training step in float64 from GIVEN indices: (embed_after, cluster_size_after, new_size, embed_sum).
        new_size[c] = sum of w over the rows of c, embed_sum[c] = sum of w * x over them      (w = weight * n / sum weight)
        cluster_size <- decay * cluster_size + (1 - decay) * new_size
        smoothed = (cluster_size + eps) / (sum(cluster_size) + K * eps) * sum(cluster_size)
        embed <- decay * embed + (1 - decay) * embed_sum / smoothed[:, None]"""
    x = np.asarray(x, dtype=np.float64)
    embed = np.asarray(embed, dtype=np.float64)
    cs = np.asarray(cluster_size, dtype=np.float64)
    n, K = x.shape[0], embed.shape[0]
    wn = normalised_weight64(w, n)
    new_size = np.zeros(K)
    np.add.at(new_size, ind, wn)
    embed_sum = np.zeros_like(embed)
    np.add.at(embed_sum, ind, x * wn[:, None])
    cs = decay * cs + (1 - decay) * new_size
    total = cs.sum()
    smoothed = (cs + eps) / (total + K * eps) * total
    embed = decay * embed + (1 - decay) * embed_sum / smoothed[:, None]
    return embed, cs, new_size, embed_sum


def nearest_f64(x, embed):
    """(argmin_c |x - embed[c]|, that distance, gap to the second-best distance) in float64 from the differences themselves
    (no expanded square), ties to the lowest c."""
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(embed, dtype=np.float64)
    ind = np.empty(x.shape[0], dtype=np.int64)
    best = np.empty(x.shape[0])
    gap = np.full(x.shape[0], np.inf)
    for i in range(0, x.shape[0], 256):
        dist = np.sqrt(((x[i:i + 256, None, :] - e[None, :, :]) ** 2).sum(-1))
        ind[i:i + 256] = dist.argmin(1)
        two = np.sort(dist, axis=1)[:, :2]
        best[i:i + 256] = two[:, 0]
        if e.shape[0] > 1:
            gap[i:i + 256] = two[:, 1] - two[:, 0]
    return ind, best, gap


def row_error(got, want64):
    """max over the code rows of max|got - want| / max(row L-inf norm, tensor L-inf norm * 2^-20); a [K] vector counts as K rows
    of one element."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want64, dtype=np.float64)
    if want.ndim == 1:
        got, want = got[:, None], want[:, None]
    scale = np.maximum(np.abs(want).max(1), np.abs(want).max() * 2.0 ** -20)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want).max(1) / scale
    return float(np.nan_to_num(err, nan=np.inf).max())


def bound(reference_deviation):
    """The parity bound of a tensor: four times the deviation of the reference's own float32 result from the same float64
    values, with a floor of 2^-22."""
    return max(4.0 * float(reference_deviation), 2.0 ** -22)


def load_case(z, name):
    """{n, d, K, weighted, x [n_all, d] float32, steps: [{keep, w, embed_pre, cs_pre, embed_ref, cs_ref, embed_f64, cs_f64, ind,
    loss, dev_embed, dev_cs}]}.  A step runs on x[keep] (the rows that are no near-tie against its pre-step codebook); its
    pre-state is the reference's float32 post-state of the step before (the stored initial state for step 0); the float64
    post-state is stored as the reference's float32 result plus a float32 correction."""
    n, d, K, T, weighted = (int(v) for v in z[f"{name}_meta"])
    x = z[f"{name}_xq"].astype(np.float32) / np.float32(X_SCALE)
    embed, cs = z[f"{name}_embed0"], z[f"{name}_cs0"]
    steps = []
    for t in range(T):
        p = f"{name}_s{t}_"
        keep = np.unpackbits(z[p + "keep"])[:n].astype(bool)
        e_ref, c_ref = z[p + "embed_ref"], z[p + "cs_ref"]
        steps.append(dict(keep=keep, w=z[p + "w"].astype(np.float32) if weighted else None, embed_pre=embed, cs_pre=cs,
                          embed_ref=e_ref, cs_ref=c_ref, embed_f64=e_ref.astype(np.float64) + z[p + "embed_corr"].astype(np.float64),
                          cs_f64=c_ref.astype(np.float64) + z[p + "cs_corr"].astype(np.float64), ind=z[p + "ind"].astype(np.int64),
                          loss=float(z[p + "loss"]), dev_embed=float(z[p + "dev"][0]), dev_cs=float(z[p + "dev"][1])))
        embed, cs = e_ref, c_ref
    return dict(n=n, d=d, K=K, weighted=bool(weighted), x=x, steps=steps)
