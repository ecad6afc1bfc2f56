"""Nearest-code search of the VecTree vector quantiser on the MI355X matrix cores (second half).

Replaces the two lines of the reference's EuclideanCodebook.forward that hold all of its arithmetic weight
(vectree/vq.py:265-266):
    dist = -torch.cdist(flatten, embed, p = 2)
    embed_ind = gumbel_sample(dist, dim = -1, temperature = self.sample_codebook_temp)      # temperature 0 -> dist.argmax(-1)
as driven by vectree/vectree.py:87-101 (chunks of 8192 feature rows against the 8192-entry codebook, 27 or 48 dimensions)
and :176-186 (the EMA k-means iterations on 80 000 sampled rows).  The kernel (csrc/lg_vq.h) evaluates |c|^2 - 2 x.c with
exact-f32 MFMA (v_mfma_f32_32x32x2_f32) and keeps the running argmin in registers; ties go to the lowest code index.

ema_update() is the rest of that forward in training mode (vq.py:278-298): the importance-weighted EMA k-means step that the
reference writes as F.one_hot(embed_ind, K) -- n x K -- and a dense einsum against it.  csrc/lg_vq_train.h lists every code's
rows (stable radix sort of (code, row)) and adds them in ascending row order: no n x K intermediate, no float atomics, bit-
reproducible.  train_codebook() is the loop of vectree/vectree.py:176-204 around it in this package's own words.
"""
import torch

from . import _lib


def nearest_code(flatten, embed):
    """embed_ind = (-torch.cdist(flatten, embed, p=2)).argmax(-1) for flatten [h, n, d] (or [n, d]) and embed [h, K, d] (or
    [K, d]): int64 indices [h, n] (or [n]).  HIP tensors only -- no CPU / torch fallback."""
    squeeze = flatten.dim() == 2
    x = flatten.unsqueeze(0) if squeeze else flatten
    cb = embed.unsqueeze(0) if embed.dim() == 2 else embed
    if x.dim() != 3 or cb.dim() != 3 or x.shape[0] != cb.shape[0] or x.shape[2] != cb.shape[2]:
        raise ValueError(f"nearest_code: incompatible shapes {tuple(flatten.shape)} / {tuple(embed.shape)}")
    if not (x.is_cuda and cb.is_cuda):
        raise RuntimeError("nearest_code runs on the MI355X HIP library only (no CPU fallback)")
    lib = _lib.load()
    h, n, d = x.shape
    K = cb.shape[1]
    nbytes = lib.lg_vq_scratch_bytes(K, d)
    if nbytes == 0:
        raise Exception(f"nearest_code: unsupported shape (K={K}, d={d}; need K >= 1, 1 <= d <= 63)")
    dev = x.device
    out = torch.empty((h, n), dtype=torch.int32, device=dev)
    scratch = _lib.scratch(nbytes, dev)
    stream = _lib.stream(dev)
    for i in range(h):
        xi = x[i].detach().contiguous().float()
        ci = cb[i].detach().contiguous().float()
        _lib.check(lib.lg_vq_nearest(n, d, K, _lib.ptr(xi), _lib.ptr(ci), _lib.ptr(out[i]), _lib.ptr(scratch), 0, stream))
    out = out.long()
    return out[0] if squeeze else out


def quantize(flatten, embed):
    """(quantized rows, indices): the codebook lookup that follows the search (vectree/vq.py:269 batched_embedding)."""
    ind = nearest_code(flatten, embed)
    if embed.dim() == 2:
        return embed[ind], ind
    return torch.stack([embed[i][ind[i]] for i in range(embed.shape[0])]), ind


def _as3(t, what):
    if t.dim() == 2:
        return t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f"ema_update: {what} must be [h, rows, d] or [rows, d], got {tuple(t.shape)}")
    return t


def ema_update(flatten, embed, cluster_size, weight=None, decay=0.8, eps=1e-5, return_quantized=False):
    """One training step of the reference's EuclideanCodebook.forward(x, weight) (vectree/vq.py:262-299; temperature 0, no DDP,
    threshold_ema_dead_code 0), fused:  with w = weight * n / weight.sum() (ones when weight is None)
        ind = nearest_code(flatten, embed)                       (on the codebook as handed in)
        cluster_size <- decay * cluster_size + (1 - decay) * [sum of w over the rows of each code]
        smoothed = (cluster_size + eps) / (cluster_size.sum() + K * eps) * cluster_size.sum()
        embed <- decay * embed + (1 - decay) * [sum of w * x over the rows of each code] / smoothed[:, None]
    flatten [h, n, d] or [n, d]; embed [h, K, d] or [K, d] and cluster_size [h, K] or [K]: contiguous float32, updated IN PLACE;
    weight [h, n, 1], [h, n], [n, 1] or [n] (the same weights for every codebook when it has no h).  Returns int64 indices
    [h, n] (or [n]); with return_quantized also the rows embed_pre[ind] of the codebook BEFORE the update, which is what the
    reference's forward returns.  A code that received no row decays towards zero, as in the reference.  The weight sum stays
    on the device (no synchronisation per step): an all-zero weight gives the reference's NaN in both buffers.
    HIP tensors only -- no CPU / torch fallback."""
    squeeze = flatten.dim() == 2
    x = _as3(flatten, "flatten")
    cb = _as3(embed, "embed")
    cs = cluster_size.unsqueeze(0) if cluster_size.dim() == 1 else cluster_size
    if cs.dim() != 2 or x.shape[0] != cb.shape[0] or x.shape[2] != cb.shape[2] or tuple(cs.shape) != tuple(cb.shape[:2]):
        raise ValueError(f"ema_update: incompatible shapes {tuple(flatten.shape)} / {tuple(embed.shape)} / {tuple(cluster_size.shape)}")
    h, n, d = x.shape
    K = cb.shape[1]
    if n == 0:
        raise ValueError("ema_update: no rows (n == 0)")
    w = None
    if weight is not None:
        if weight.numel() == h * n:
            w = weight.reshape(h, n)
        elif weight.numel() == n:
            w = weight.reshape(1, n).expand(h, n)
        else:
            raise ValueError(f"ema_update: weight {tuple(weight.shape)} does not match {h} x {n} rows")
    if not (x.is_cuda and cb.is_cuda and cs.is_cuda and (w is None or w.is_cuda)):
        raise RuntimeError("ema_update runs on the MI355X HIP library only (no CPU fallback)")
    if cb.dtype != torch.float32 or cs.dtype != torch.float32 or not cb.is_contiguous() or not cs.is_contiguous():
        raise ValueError("ema_update: embed and cluster_size are updated in place and must be contiguous float32")
    lib = _lib.load()
    nbytes = lib.lg_vq_ema_scratch_bytes(n, K, d)
    if nbytes == 0:
        raise Exception(f"ema_update: unsupported shape (n={n}, K={K}, d={d}; need K >= 1, 1 <= d <= 63)")
    dev = x.device
    out = torch.empty((h, n), dtype=torch.int32, device=dev)
    scratch = _lib.scratch(nbytes, dev)
    stream = _lib.stream(dev)
    pre = cb.detach().clone() if return_quantized else None
    for i in range(h):
        xi = x[i].detach().contiguous().float()
        wi = None if w is None else w[i].detach().contiguous().float()
        _lib.check(lib.lg_vq_ema_step(n, d, K, _lib.ptr(xi), _lib.ptr(wi), _lib.ptr(cb[i]), _lib.ptr(cs[i]), float(decay), float(eps),
                                      _lib.ptr(out[i]), _lib.ptr(scratch), 0, stream))
    ind = out.long()
    if not return_quantized:
        return ind[0] if squeeze else ind
    quant = torch.stack([pre[i][ind[i]] for i in range(h)])
    return (ind[0], quant[0]) if squeeze else (ind, quant)


def train_codebook(feats, importance, embed, cluster_size, iterations=1000, chunk=80000, k_expire=10, decay=0.8, eps=1e-5, generator=None):
    """EMA k-means training of one codebook on importance-weighted rows, the loop of vectree/vectree.py:196-204: `iterations`
    times, draw `chunk` row numbers of feats [N, d] uniformly with replacement (on the device, from `generator`), run
    ema_update() on those rows with their importance as the weight, then re-seed the `k_expire` least-used codes (smallest
    cluster_size) with the `k_expire` most important rows of the draw.  embed [K, d] and cluster_size [K] are updated in
    place.  Returns the importance-weighted mean squared quantisation error of each draw against the codebook it was searched
    on, a device tensor [iterations] (element i + 1 judges the codebook that iteration i left; nothing is read back inside
    the loop).  Same generator state, same inputs: the same bits."""
    if feats.dim() != 2 or embed.dim() != 2 or cluster_size.dim() != 1 or importance.numel() != feats.shape[0]:
        raise ValueError(f"train_codebook: feats [N, d], importance [N], embed [K, d], cluster_size [K] expected, got "
                         f"{tuple(feats.shape)} / {tuple(importance.shape)} / {tuple(embed.shape)} / {tuple(cluster_size.shape)}")
    if not (feats.is_cuda and importance.is_cuda and embed.is_cuda and cluster_size.is_cuda):
        raise RuntimeError("train_codebook runs on the MI355X HIP library only (no CPU fallback)")
    N, K = feats.shape[0], embed.shape[0]
    imp = importance.reshape(-1).float()
    k_expire = 0 if k_expire > K else min(int(k_expire), chunk)           # (vectree.py:194-195)
    errors = torch.zeros(iterations, dtype=torch.float32, device=feats.device)
    with torch.no_grad():
        for it in range(iterations):
            rows = torch.randint(0, N, (chunk,), device=feats.device, generator=generator)
            x, w = feats[rows].float(), imp[rows]
            ind, quant = ema_update(x, embed, cluster_size, weight=w, decay=decay, eps=eps, return_quantized=True)
            errors[it] = (w * (x - quant).square().sum(-1)).sum() / w.sum()
            if k_expire > 0:
                dead = torch.topk(cluster_size, k_expire, largest=False).indices
                best = torch.topk(w, k_expire, largest=True).indices
                embed[dead] = x[best]
    return errors
