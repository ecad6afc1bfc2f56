"""Golden vectors for the VecTree TRAINING step, produced by the REFERENCE's own code: imports /root/reference/vectree/vq.py
(unmodified, like make_golden_vq.py) and runs, on the CPU,
    model = VectorQuantize(dim=d, codebook_size=K, decay=0.8, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0)
    model.train(); model(x[None], weight=w.reshape(1, -1, 1))                 (vectree/vectree.py:200)
for T consecutive steps per case.  Stored per step: the weights, the rows that take part, the reference's indices, loss and
float32 post-state (which is the next step's pre-state), the float64 post-state computed from the reference's own indices
(tests/vq_train_common.ema_step_f64; stored as a float32 correction on top of the float32 result) and the deviation of the
reference's float32 result from it under the parity tests' error measure (vq_train_common.row_error).

Near-ties.  An index flip moves a whole row between two codes and cannot be tolerated in a sum, so the rows whose best /
second-best distance gap (float64) against the step's pre-step codebook is below 1e-4 x the mean nearest distance are left
out of that step; at most 2 % of a step's rows may go (asserted), and on the rows that stay the reference's indices equal the
float64 argmin (asserted).  The codebook starts as K sampled rows + 0.05 x noise (the regime the k_expire replacement of
vectree.py:202-204 keeps it in); with the default Kaiming-uniform start the first step alone would lose 10-13 % of its rows.

Size.  Rows live on a 1/64 grid and are stored as int8, weights are half-precision values, the reference's quantised rows are
not stored (asserted here to be the straight-through form x + (embed_pre[ind] - x) of the pre-update codebook, bit for bit): the file stays below the 1 MiB limit of a committed file.
Run:  python tests/golden/make_golden_vq_train.py   (needs /root/reference and einops; the committed .npz travels)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/vectree")
import vq_train_common as vc  # noqa: E402
from vq import VectorQuantize  # noqa: E402

T = 3
CASES = (("deg2", 4000, 27, 256, True), ("deg3", 3000, 48, 192, True), ("tiny", 300, 3, 16, True),
         ("unweighted", 1000, 12, 40, False), ("wide", 1500, 63, 72, True))
assert tuple(c[0] for c in CASES) == vc.CASES

out = {}
gen = torch.Generator().manual_seed(20261016)
for name, n, d, K, weighted in CASES:
    centres = 0.5 * torch.randn(K, d, generator=gen)
    x = centres[torch.randint(0, K, (n,), generator=gen)] + 0.1 * torch.randn(n, d, generator=gen)
    xq = torch.clamp(torch.round(x * vc.X_SCALE), -127, 127).to(torch.int8)
    x = xq.float() / vc.X_SCALE
    embed0 = (x[torch.randperm(n, generator=gen)[:K]] + 0.05 * torch.randn(K, d, generator=gen)).contiguous()
    model = VectorQuantize(dim=d, codebook_size=K, decay=vc.DECAY, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0)
    model.train()
    cb = model._codebook
    cb.embed.data.copy_(embed0[None])
    out[f"{name}_meta"] = np.array([n, d, K, T, int(weighted)], dtype=np.int64)
    out[f"{name}_xq"] = xq.numpy()
    out[f"{name}_embed0"] = cb.embed[0].numpy().copy()
    out[f"{name}_cs0"] = cb.cluster_size[0].numpy().copy()
    for t in range(T):
        p = f"{name}_s{t}_"
        embed_pre, cs_pre = cb.embed[0].numpy().copy(), cb.cluster_size[0].numpy().copy()
        ind64, best, gap = vc.nearest_f64(x.numpy(), embed_pre)
        keep = gap >= 1e-4 * best.mean()
        dropped = 1.0 - keep.mean()
        assert dropped <= 0.02, (name, t, dropped)
        xs = x[torch.from_numpy(keep)]
        w = torch.exp(1.5 * torch.randn(n, generator=gen)).half().float()          # heavy-tailed importance, one per row of the pool
        ws = w[torch.from_numpy(keep)]
        with torch.no_grad():
            quant, ind, loss = model(xs[None], weight=ws.reshape(1, -1, 1) if weighted else None)
        ind = ind.reshape(-1).numpy()
        assert np.array_equal(ind, ind64[keep]), (name, t, int((ind != ind64[keep]).sum()))
        # what the codebook returns is embed_pre[ind]; VectorQuantize.forward hands out its straight-through form x + (q - x)
        assert np.array_equal(quant[0].numpy(), xs.numpy() + (embed_pre[ind] - xs.numpy())), (name, t)
        e_ref, c_ref = cb.embed[0].numpy().copy(), cb.cluster_size[0].numpy().copy()
        e64, c64, _, _ = vc.ema_step_f64(xs.numpy(), ws.numpy() if weighted else None, embed_pre, cs_pre, ind)
        e_corr, c_corr = (e64 - e_ref).astype(np.float32), (c64 - c_ref).astype(np.float32)
        for full, ref, corr in ((e64, e_ref, e_corr), (c64, c_ref, c_corr)):          # the stored pair reproduces the float64 value
            assert np.abs(ref.astype(np.float64) + corr.astype(np.float64) - full).max() <= 1e-13 * np.abs(full).max()
        dev = np.array([vc.row_error(e_ref, e64), vc.row_error(c_ref, c64)])
        out[p + "keep"] = np.packbits(keep)
        if weighted:
            out[p + "w"] = w.numpy().astype(np.float16)[keep]
        out[p + "ind"] = ind.astype(np.int16)
        out[p + "loss"] = np.float32(loss.item())
        out[p + "embed_ref"], out[p + "cs_ref"] = e_ref, c_ref
        out[p + "embed_corr"], out[p + "cs_corr"] = e_corr, c_corr
        out[p + "dev"] = dev
        print(f"{name} step {t}: rows {int(keep.sum())}/{n} (dropped {100 * dropped:.2f} %), codes used {len(np.unique(ind))}/{K}, "
              f"reference deviation embed {dev[0]:.3g} cluster_size {dev[1]:.3g}, loss {loss.item():.6f}")
path = os.path.join(HERE, "reference_vq_train.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1000 * 1024
