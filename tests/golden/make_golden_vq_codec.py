"""Golden vectors for the VecTree model FORMAT, produced by the REFERENCE's own code: imports /root/reference/vectree/
vectree.py, utils.py and vq.py unmodified (plyfile, which only the PLY helpers of utils.py use, is stubbed), and for every case
    q = Quantization.__new__(Quantization)            -- no constructor: it reads a PLY file
    q.feats_bak / feats / sh_dim / codebook_size / vq_way / save_path / all_one_mask / non_vq_mask / model_vq = ...
    q.fully_vq_reformat()                             -- vectree.py:100-155 writes <tmp>/extreme_saving
    load_vqgaussian(<tmp>/extreme_saving, "cpu")      -- utils.py:5-65 reads it back
with the mask chosen as Quantization.quantize() chooses it (topk of a random importance, k = int(N (1 - vq_ratio))) and the
codebook of q.model_vq set to the case's.  Stored per case: the inputs (the full table, the mask, the reference's own codes of
ALL rows, i.e. all_indice), the seven arrays exactly as the reference's files hold them, and the dequantised table.
The generator also lets the reference's load_vqgaussian read a directory written by lightgaussian_amd.vectree.save and asserts
the same table (the tests, which run without the reference, cover the direction reference -> this package).

Cases: both SH widths, N never a multiple of 8, index widths that do not divide 8 (5, 6 and the pipeline's 13 bits), vq_ratio
0.6 throughout except one case with vq_ratio 1 (an empty non-VQ set).
Size.  All inputs live on a float16 grid, so the float32 tables are stored as float16 (asserted lossless); the 8192-row
codebook takes its values from nine levels and deflates well.  The file stays below the 1 MiB limit of a committed file.
Run:  python tests/golden/make_golden_vq_codec.py   (needs /root/reference, einops and tqdm; the committed .npz travels)."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.modules.setdefault("plyfile", types.SimpleNamespace(PlyData=None, PlyElement=None))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference/vectree")
import vectree as ref_vectree  # noqa: E402
from utils import load_vqgaussian  # noqa: E402
from vq import VectorQuantize  # noqa: E402
from lightgaussian_amd import vectree as our_vectree  # noqa: E402

ref_vectree.device = torch.device("cpu")

# name, N, sh_dim, K, vq_ratio
CASES = (("deg2_k32", 1003, 27, 32, 0.6), ("deg3_k64", 517, 48, 64, 0.6), ("deg2_k8192", 203, 27, 8192, 0.6),
         ("deg3_all_vq", 301, 48, 32, 1.0))
FILES = ("vq_indexs", "codebook", "non_vq_mask", "non_vq_feats", "other_attribute", "xyz")

out = {}
gen = torch.Generator().manual_seed(20261017)
for name, N, d, K, ratio in CASES:
    C = 6 + d + 8
    if K >= 4096:
        codebook = (torch.randint(-4, 5, (K, d), generator=gen).float() / 8).half().float()
    else:
        codebook = (0.3 * torch.randn(K, d, generator=gen)).half().float()
    feats = torch.zeros(N, C)
    feats[:, 0:3] = 3.0 * torch.randn(N, 3, generator=gen)
    feats[:, 3:6] = torch.randn(N, 3, generator=gen)              # normals: present in a PLY, dropped by the format
    feats[:, 6:6 + d] = codebook[torch.randint(0, K, (N,), generator=gen)] + 0.05 * torch.randn(N, d, generator=gen)
    feats[:, -8:] = torch.randn(N, 8, generator=gen) * torch.tensor([1.5, 0.5, 0.5, 0.5, 1, 1, 1, 1]) + torch.tensor([-1.0, -5, -5, -5, 0, 0, 0, 0])
    feats = feats.half().float()
    importance = torch.rand(N, generator=gen).double()
    q = ref_vectree.Quantization.__new__(ref_vectree.Quantization)
    q.feats_bak = feats.clone()
    q.feats = feats[:, 6:6 + d]
    q.sh_dim, q.codebook_size, q.vq_way = d, K, "half"
    # the mask as vectree.py:175-179 builds it
    _, large_index = torch.topk(importance, k=int(importance.shape[0] * (1 - ratio)), largest=True)
    q.all_one_mask = torch.ones_like(importance).bool()
    q.non_vq_mask = torch.zeros_like(importance).bool()
    q.non_vq_mask[large_index] = True
    q.model_vq = VectorQuantize(dim=d, codebook_size=K, decay=0.8, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0)
    q.model_vq._codebook.embed.data.copy_(codebook[None])
    with tempfile.TemporaryDirectory() as tmp:
        q.save_path = tmp
        _, all_indice = q.fully_vq_reformat()
        folder = os.path.join(tmp, "extreme_saving")
        assert sorted(os.listdir(folder)) == sorted(f + ".npz" for f in FILES + ("metadata",))
        meta = np.load(os.path.join(folder, "metadata.npz"), allow_pickle=True)["metadata"].item()
        stored = {}
        for f in FILES:
            z = np.load(os.path.join(folder, f + ".npz"))
            assert z.files == ["arr_0"]
            stored[f] = z["arr_0"]
        table = load_vqgaussian(folder, device="cpu").numpy()
        # the other direction, checked here because only this machine has the reference: ITS reader on a directory WE wrote
        ours = os.path.join(tmp, "ours")
        our_vectree.save(ours, our_vectree.pack(feats, q.non_vq_mask, codebook, all_indice.reshape(-1)))
        assert np.array_equal(load_vqgaussian(ours, device="cpu").numpy().view(np.uint32), table.view(np.uint32)), name
    assert table.dtype == np.float32 and table.shape == (N, C)
    assert np.array_equal(table.astype(np.float16).astype(np.float32), table)
    assert np.array_equal(feats.numpy().astype(np.float16).astype(np.float32), feats.numpy())
    ind = all_indice.reshape(-1).numpy()
    assert ind.shape == (N,) and ind.min() >= 0 and ind.max() < K
    out[f"{name}_meta"] = np.array([meta["input_pc_num"], meta["input_pc_dim"], meta["codebook_size"], meta["codebook_dim"]], np.int64)
    assert all(type(v) is int for v in meta.values()) and len(meta) == 4
    out[f"{name}_in_feats"] = feats.numpy().astype(np.float16)
    out[f"{name}_in_mask"] = np.packbits(q.non_vq_mask.numpy())
    out[f"{name}_in_indices"] = ind.astype(np.uint16)
    for f in FILES:
        out[f"{name}_{f}"] = stored[f]
    out[f"{name}_table"] = table.astype(np.float16)
    print(f"{name}: N {N}, d {d}, K {K}, non-VQ rows {int(q.non_vq_mask.sum())}, index bytes {stored['vq_indexs'].shape[0]}, "
          f"dtypes {[str(stored[f].dtype) for f in FILES]}")
path = os.path.join(HERE, "reference_vq_codec.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1000 * 1024
