"""The VecTree-compressed model ("extreme_saving") of LightGaussian's third stage: codec, device-resident form, colour kernel.

What the reference writes in vectree/vectree.py:100-155 (Quantization.fully_vq_reformat) and reads back in
vectree/utils.py:5-65 (load_vqgaussian) and scene/gaussian_model.py:420-461 (GaussianModel.load_vq) is a directory of seven
.npz files:
    metadata.npz         key "metadata": a pickled dict  input_pc_num N, input_pc_dim C, codebook_size K, codebook_dim d
    vq_indexs.npz        uint8: the codebook index of every VQ row, log2(K) bits each, most significant bit first, one after
                         the other, padded to whole bytes (numpy.packbits)
    codebook.npz         float16 [K, d]
    non_vq_mask.npz      uint8: one bit per Gaussian (1 = its SH row is stored itself), packbits-padded
    non_vq_feats.npz     [n_nonvq, d] SH rows of the non-VQ Gaussians, in ascending Gaussian order
    other_attribute.npz  [N, 8] opacity logit, 3 log-scales, 4 quaternion components
    xyz.npz              float32 [N, 3]
(all but the first under the key "arr_0"; with vq_way "half" non_vq_feats and other_attribute are float16).  A row of the
model is the PLY row  x y z  nx ny nz  f_dc_0..2  f_rest_0..(d-4) (channel-major)  opacity  scale_0..2  rot_0..3,  C = 6 + d + 8
columns, d = 27 (SH degree 2) or 48 (degree 3).

pack / save / load / unpack speak that format bit for bit in both directions; quantize_model is the whole of
Quantization.quantize() on the GPU (vq.train_codebook, vq.nearest_code); CompressedGaussians keeps a loaded model on the
device in its compressed form and colors() / gaussian_renderer.render_compressed() render it without ever building the
[N, d] float32 SH table (csrc/lg_vq_color.h).  CompressedGaussians.trainable() makes that form trainable in place
(TrainableCompressed: float32 masters of the rows and of the other attributes, a straight-through forward on their float16
values, lg_vq_colors_bwd of csrc/lg_vq_color_bwd.h as the backward of colors()); repack() gives the model back as the seven arrays.
"""
import math
import os

import numpy as np
import torch

from . import _lib

FILES = ("metadata", "vq_indexs", "codebook", "non_vq_mask", "non_vq_feats", "other_attribute", "xyz")
SH_DIMS = (27, 48)
MAX_CODEBOOK = 65536


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _bits_of(K):
    K = int(K)
    if K < 1 or K > MAX_CODEBOOK or K & (K - 1):
        raise ValueError(f"codebook size {K}: a power of two, at most {MAX_CODEBOOK}, is required (indices are stored as log2(K) bits)")
    return K.bit_length() - 1


def _narrow(a, vq_way):
    a = np.ascontiguousarray(a)
    return a.astype(np.float16) if vq_way == "half" else a


def pack(feats, non_vq_mask, codebook, indices, vq_way="half"):
    """The seven arrays of vectree.py:110-146 from a full table.  feats [N, 6 + d + 8] float32 (PLY rows), non_vq_mask [N]
    bool, codebook [K, d] float, indices [N] integer codes (those of non-VQ rows are ignored, as all_indice's are).
    vq_way "half": non-VQ rows and the 8 other attributes as float16; anything else keeps them float32 (the codebook is
    float16 either way, as in the reference)."""
    f, mask, cb, ind = _np(feats), _np(non_vq_mask), _np(codebook), _np(indices)
    if cb.ndim != 2 or cb.shape[1] not in SH_DIMS:
        raise ValueError(f"pack: codebook [K, 27 or 48] expected, got {cb.shape}")
    K, d = cb.shape
    bits = _bits_of(K)
    if f.ndim != 2 or f.shape[1] != 6 + d + 8:
        raise ValueError(f"pack: feats must have 6 + {d} + 8 = {d + 14} columns, got {f.shape}")
    N = f.shape[0]
    if mask.dtype != np.bool_:
        raise ValueError(f"pack: non_vq_mask must be boolean, got {mask.dtype}")
    mask, ind = mask.reshape(-1), ind.reshape(-1)
    if mask.shape[0] != N or ind.shape[0] != N:
        raise ValueError(f"pack: {N} rows, but a mask of {mask.shape[0]} and {ind.shape[0]} indices")
    if ind.dtype.kind not in "iu":
        raise ValueError(f"pack: indices must be integers, got {ind.dtype}")
    f = f.astype(np.float32, copy=False)
    code = ind[~mask].astype(np.int64)
    if code.size and (code.min() < 0 or code.max() >= K):
        raise ValueError(f"pack: a code outside [0, {K})")
    shifts = np.arange(bits - 1, -1, -1, dtype=np.int64)
    bit_rows = ((code[:, None] >> shifts[None, :]) & 1).astype(np.bool_)
    return {
        "metadata": {"input_pc_num": int(N), "input_pc_dim": int(f.shape[1]), "codebook_size": int(K), "codebook_dim": int(d)},
        "vq_indexs": np.packbits(bit_rows.reshape(-1)),
        "codebook": np.ascontiguousarray(cb).astype(np.float32, copy=False).astype(np.float16),
        "non_vq_mask": np.packbits(mask),
        "non_vq_feats": _narrow(f[mask, 6:6 + d], vq_way),
        "other_attribute": _narrow(f[:, -8:], vq_way),
        "xyz": np.ascontiguousarray(f[:, 0:3]),
    }


def save(path, packed):
    """Write `packed` as the reference's extreme_saving directory (`path` is that directory itself)."""
    _decode(packed)                     # nothing malformed reaches the disk
    os.makedirs(path, exist_ok=True)
    np.savez_compressed(os.path.join(path, "metadata.npz"), metadata=dict(packed["metadata"]))
    for name in FILES[1:]:
        np.savez_compressed(os.path.join(path, name + ".npz"), packed[name])


def load(path):
    """Read an extreme_saving directory (ours or the reference's) into the dict pack() returns."""
    with np.load(os.path.join(path, "metadata.npz"), allow_pickle=True) as z:
        meta = z["metadata"].item()
    packed = {"metadata": {k: int(meta[k]) for k in ("input_pc_num", "input_pc_dim", "codebook_size", "codebook_dim")}}
    for name in FILES[1:]:
        with np.load(os.path.join(path, name + ".npz")) as z:
            packed[name] = z["arr_0"]
    _decode(packed)
    return packed


def _decode(packed):
    """Checks a packed model and returns (N, C, K, d, mask bool [N], codes int64 [n_vq])."""
    missing = [k for k in FILES if k not in packed]
    if missing:
        raise ValueError(f"packed model lacks {missing}")
    meta = packed["metadata"]
    N, Cdim, K, d = (int(meta[k]) for k in ("input_pc_num", "input_pc_dim", "codebook_size", "codebook_dim"))
    bits = _bits_of(K)
    if d not in SH_DIMS or Cdim != 6 + d + 8 or N < 0:
        raise ValueError(f"packed model: codebook_dim {d} must be 27 or 48 and input_pc_dim {Cdim} = 6 + codebook_dim + 8")
    cb, nv, oa, xyz = (np.asarray(packed[k]) for k in ("codebook", "non_vq_feats", "other_attribute", "xyz"))
    mbits, ibits = np.asarray(packed["non_vq_mask"]), np.asarray(packed["vq_indexs"])
    if mbits.dtype != np.uint8 or ibits.dtype != np.uint8 or mbits.ndim != 1 or ibits.ndim != 1:
        raise ValueError("packed model: non_vq_mask and vq_indexs are flat uint8 bit strings")
    if cb.shape != (K, d) or oa.shape != (N, 8) or xyz.shape != (N, 3):
        raise ValueError(f"packed model: codebook {cb.shape}, other_attribute {oa.shape}, xyz {xyz.shape} do not fit N = {N}, K = {K}, d = {d}")
    if mbits.shape[0] != (N + 7) // 8:
        raise ValueError(f"packed model: a mask of {mbits.shape[0]} bytes for {N} Gaussians")
    mask = np.unpackbits(mbits)[:N].astype(np.bool_)
    n_nv = int(mask.sum())
    n_vq = N - n_nv
    if nv.ndim != 2 or nv.shape != (n_nv, d):
        raise ValueError(f"packed model: {n_nv} non-VQ rows in the mask, non_vq_feats is {nv.shape}")
    if ibits.shape[0] != (n_vq * bits + 7) // 8:
        raise ValueError(f"packed model: {ibits.shape[0]} index bytes for {n_vq} VQ rows of {bits} bits")
    b = np.unpackbits(ibits)[:n_vq * bits].reshape(n_vq, bits).astype(np.int64)
    codes = (b << np.arange(bits - 1, -1, -1, dtype=np.int64)[None, :]).sum(1) if bits else np.zeros(n_vq, np.int64)
    return N, Cdim, K, d, mask, codes


def unpack(packed, device="cpu"):
    """The table load_vqgaussian returns: float32 [N, input_pc_dim], normals zero, bit for bit."""
    N, Cdim, K, d, mask, codes = _decode(packed)
    full = np.zeros((N, Cdim), np.float32)
    full[:, 0:3] = np.asarray(packed["xyz"], np.float32)
    full[:, -8:] = np.asarray(packed["other_attribute"]).astype(np.float32)
    sh = full[:, 6:6 + d]
    sh[~mask] = np.asarray(packed["codebook"]).astype(np.float32)[codes]
    sh[mask] = np.asarray(packed["non_vq_feats"]).astype(np.float32)
    return torch.from_numpy(full).to(device)


def quantize_model(feats, importance, vq_ratio=0.6, codebook_size=8192, iterations=1000, chunk=80000, k_expire=10, decay=0.8,
                   eps=1e-5, vq_way="half", search_chunk=1 << 18, embed=None, generator=None):
    """Quantization.quantize() (vectree/vectree.py:166-207) on the GPU, without the files in between: the
    int(N * (1 - vq_ratio)) most important rows keep their own SH row, vq.train_codebook() trains one codebook on the others
    (importance-weighted EMA k-means from a Kaiming-uniform start, as the reference's VectorQuantize begins), the codebook is
    rounded through float16 -- the values a reader of the model will see -- vq.nearest_code() assigns EVERY row against it
    in chunks of `search_chunk`, and pack() lays the result out.  feats [N, 6 + d + 8] and importance [N] on the HIP device;
    `embed` [K, d]: a start codebook of the caller's instead (not modified); `generator` (a device generator) makes the run
    reproducible.  Returns the packed dict."""
    from . import vq
    if not (torch.is_tensor(feats) and feats.is_cuda and torch.is_tensor(importance) and importance.is_cuda):
        raise RuntimeError("quantize_model runs on the MI355X HIP library only (no CPU fallback)")
    K = int(codebook_size)
    _bits_of(K)
    if feats.dim() != 2 or feats.shape[1] - 14 not in SH_DIMS:
        raise ValueError(f"quantize_model: feats must have 6 + (27 or 48) + 8 columns, got {tuple(feats.shape)}")
    N, d = feats.shape[0], feats.shape[1] - 14
    imp = importance.reshape(-1)
    if imp.shape[0] != N:
        raise ValueError(f"quantize_model: {N} rows, {imp.shape[0]} importance values")
    if not 0.0 <= vq_ratio <= 1.0:
        raise ValueError(f"quantize_model: vq_ratio {vq_ratio} outside [0, 1]")
    dev = feats.device
    with torch.no_grad():
        sh = feats[:, 6:6 + d].float().contiguous()
        keep = torch.topk(imp, k=int(N * (1 - vq_ratio)), largest=True).indices
        non_vq = torch.zeros(N, dtype=torch.bool, device=dev)
        non_vq[keep] = True
        if embed is None:
            bound = math.sqrt(6.0 / (K * d))                    # nn.init.kaiming_uniform_ of a [1, K, d] tensor (vq.py:25-28)
            embed = ((torch.rand(K, d, device=dev, generator=generator) * 2 - 1) * bound).contiguous()
        else:
            if tuple(embed.shape) != (K, d) or not embed.is_cuda:
                raise ValueError(f"quantize_model: embed must be a [{K}, {d}] tensor on the device, got {tuple(embed.shape)}")
            embed = embed.detach().float().clone().contiguous()
        cluster_size = torch.zeros(K, device=dev)
        if int(N - keep.numel()) > 0 and iterations > 0:
            vq_rows = ~non_vq
            vq.train_codebook(sh[vq_rows], imp[vq_rows].float(), embed, cluster_size, iterations=int(iterations), chunk=chunk,
                              k_expire=k_expire, decay=decay, eps=eps, generator=generator)
        codebook = embed.half().float()
        ind = torch.empty(N, dtype=torch.int64, device=dev)
        for lo in range(0, N, search_chunk):
            ind[lo:lo + search_chunk] = vq.nearest_code(sh[lo:lo + search_chunk], codebook)
    return pack(feats, non_vq, codebook, ind, vq_way)


class CompressedGaussians:
    """A loaded extreme_saving model, resident on `device` in its compressed form:
        xyz      float32 [N, 3]
        opacity  float32 [N, 1], scaling [N, 3], rotation [N, 4]: the 8 other attributes, float16 -> float32 and ACTIVATED once
                 here with torch (sigmoid, exp, F.normalize) -- exactly what the reference's getters return after load_vq
        rows     float16 [K + n_nonvq, row_stride / 2]: the codebook rows, then the non-VQ rows, each padded with zeros to a
                 multiple of 16 bytes (d = 27: 54 -> 64 bytes; d = 48: 96)
        slot     uint32 [N]: the row of each Gaussian -- its code for a VQ row, K + its rank among the non-VQ rows otherwise
    The raw attributes as stored stay on the host for to_dense().  Forward-only: no tensor here takes gradients; trainable()
    returns the form that does."""

    def __init__(self, xyz, opacity, scaling, rotation, rows, slot, codebook_size, sh_dim, other_raw):
        self.xyz, self.opacity, self.scaling, self.rotation = xyz, opacity, scaling, rotation
        self.rows, self._slot = rows, slot                      # _slot: the same words as int32 (torch indexes with it)
        self.codebook_size, self.sh_dim = int(codebook_size), int(sh_dim)
        self.max_sh_degree = int(round(math.sqrt(sh_dim // 3))) - 1
        self.active_sh_degree = self.max_sh_degree
        self._other_raw = other_raw                             # host copy of other_attribute (raw logit / log-scale / quaternion)

    @classmethod
    def from_packed(cls, packed, device="cuda"):
        N, Cdim, K, d, mask, codes = _decode(packed)
        n_nv = int(mask.sum())
        if np.asarray(packed["non_vq_feats"]).dtype != np.float16:
            raise ValueError("CompressedGaussians holds float16 SH rows: a model written with another vq_way than 'half' goes through unpack()")
        if K + n_nv >= 1 << 31:
            raise ValueError("CompressedGaussians: more than 2^31 - 1 SH rows")
        stride_h = (2 * d + 15) // 16 * 8                       # halfs per padded row
        table = np.zeros((K + n_nv, stride_h), np.float16)
        table[:K, :d] = np.asarray(packed["codebook"]).astype(np.float16)
        table[K:, :d] = np.asarray(packed["non_vq_feats"])
        slot = np.empty(N, np.int64)
        slot[~mask] = codes
        slot[mask] = K + np.arange(n_nv)
        other_raw = torch.from_numpy(np.ascontiguousarray(packed["other_attribute"]))
        other = other_raw.to(device).float()
        return cls(xyz=torch.from_numpy(np.asarray(packed["xyz"], np.float32).copy()).to(device),
                   # (on contiguous columns, as load_vq's parameters are: torch's CPU kernels round a strided view differently)
                   opacity=torch.sigmoid(other[:, 0:1].contiguous()), scaling=torch.exp(other[:, 1:4].contiguous()),
                   rotation=torch.nn.functional.normalize(other[:, 4:8].contiguous()),
                   rows=torch.from_numpy(table).to(device), slot=torch.from_numpy(slot.astype(np.int32)).to(device),
                   codebook_size=K, sh_dim=d, other_raw=other_raw)

    @classmethod
    def load(cls, path, device="cuda"):
        return cls.from_packed(load(path), device)

    # the getter surface render() reads (scene/gaussian_model.py:98-118)
    @property
    def get_xyz(self):
        return self.xyz

    @property
    def get_opacity(self):
        return self.opacity

    @property
    def get_scaling(self):
        return self.scaling

    @property
    def get_rotation(self):
        return self.rotation

    @property
    def slot(self):
        return self._slot.view(torch.uint32)

    @property
    def num(self):
        return self.xyz.shape[0]

    @property
    def row_stride(self):
        """bytes between two rows of the table"""
        return self.rows.shape[1] * 2

    def nbytes(self):
        """Resident device bytes: N (12 + 32 + 4) + (K + n_nonvq) row_stride."""
        return sum(t.numel() * t.element_size() for t in (self.xyz, self.opacity, self.scaling, self.rotation, self._slot, self.rows))

    def to_dense(self):
        """The model load_vq builds (gaussian_model.py:420-461), as a synthetic.SyntheticGaussians on the same device: raw
        _opacity / _scaling / _rotation, _features_dc [N, 1, 3] and _features_rest [N, M - 1, 3] (the row's f_rest part reshaped
        (N, 3, M - 1), then transposed).  For comparison and for fine-tuning; this is the 59-float-per-Gaussian form."""
        from .synthetic import SyntheticGaussians
        dev, N, d = self.xyz.device, self.num, self.sh_dim
        sh = self.rows[self._slot.long(), :d].float()
        other = self._other_raw.to(dev).float()
        return SyntheticGaussians(
            _xyz=self.xyz.clone(), _features_dc=sh[:, 0:3].reshape(N, 3, 1).transpose(1, 2).contiguous(),
            _features_rest=sh[:, 3:].reshape(N, 3, d // 3 - 1).transpose(1, 2).contiguous(),
            _scaling=other[:, 1:4].contiguous(), _rotation=other[:, 4:8].contiguous(), _opacity=other[:, 0:1].contiguous(),
            active_sh_degree=self.active_sh_degree, max_sh_degree=self.max_sh_degree)

    def trainable(self, params=("rows",)):
        """This model as a TrainableCompressed: float32 masters, the tensors named in `params` (of "rows", "xyz", "opacity",
        "scaling", "rotation") as nn.Parameters.  The model itself is left as it is (the trainable copy owns its tensors)."""
        return TrainableCompressed(self, params)

    def colors(self, camera_center, sh_degree=None, out=None, flags=0):
        """[N, 3] float32: clamp_min(eval_sh(degree, SH row, normalised view direction) + 0.5, 0) of every Gaussian for a camera
        at `camera_center` -- lg_vq_colors, one HIP launch on the current stream, no synchronisation.  HIP tensors only."""
        if not self.xyz.is_cuda:
            raise RuntimeError("CompressedGaussians.colors runs on the MI355X HIP library only (no CPU fallback): use to_dense()")
        D = self.active_sh_degree if sh_degree is None else int(sh_degree)
        dev, N = self.xyz.device, self.num
        if out is None:
            out = torch.empty((N, 3), dtype=torch.float32, device=dev)
        elif out.shape != (N, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError("colors: out must be a contiguous float32 [N, 3] tensor on the model's device")
        cam = camera_center.detach().to(device=dev, dtype=torch.float32).contiguous()
        lib = _lib.load()
        stream = _lib.stream(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.lg_vq_colors(N, self.sh_dim // 3, D, _lib.ptr(self.xyz), _lib.ptr(cam), _lib.ptr(self._slot),
                                        _lib.ptr(self.rows), self.row_stride, _lib.ptr(out), int(flags), stream))
        return out


class _RoundHalf(torch.autograd.Function):
    """x -> float32(float16(x)) with a straight-through gradient: the forward sees the value the file will hold."""

    @staticmethod
    def forward(ctx, x):
        return x.half().float()

    @staticmethod
    def backward(ctx, g):
        return g


class _VqColors(torch.autograd.Function):
    """colors() of a TrainableCompressed: lg_vq_colors forward on the fp16 table, lg_vq_colors_bwd backward onto the float32
    master of the rows (straight-through) and, when it takes gradients, onto xyz."""

    @staticmethod
    def forward(ctx, rows_master, xyz, model, cam, D):
        ctx.model, ctx.cam, ctx.D = model, cam, D
        return CompressedGaussians.colors(model, cam, sh_degree=D)

    @staticmethod
    def backward(ctx, g):
        m = ctx.model
        dev, N, d, K = m._xyz.device, m.num, m.sh_dim, m.codebook_size
        g = g.to(torch.float32).contiguous()
        lib = _lib.load()
        drows = torch.empty((m.rows.shape[0], d), dtype=torch.float32, device=dev)
        dxyz = torch.empty((N, 3), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        scratch = _lib.scratch(lib.lg_vq_colors_bwd_scratch_bytes(N, d // 3, K), dev)
        stream = _lib.stream(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.lg_vq_colors_bwd(N, d // 3, ctx.D, K, m.rows.shape[0], _lib.ptr(m._xyz), _lib.ptr(ctx.cam), _lib.ptr(m._slot),
                                            _lib.ptr(m.rows), m.row_stride, _lib.ptr(g), _lib.ptr(m._index), _lib.ptr(drows),
                                            _lib.ptr(dxyz), _lib.ptr(scratch), 0, stream))
        return (drows if ctx.needs_input_grad[0] else None), dxyz, None, None, None


class TrainableCompressed(CompressedGaussians):
    """A CompressedGaussians that can be fine-tuned in its compressed form (CompressedGaussians.trainable()):
        _rows     float32 master [K + n_nonvq, d] of the row table, unpadded, in the file's column order
        _xyz      float32 [N, 3]
        _opacity  [N, 1], _scaling [N, 3], _rotation [N, 4]: float32 masters of the raw other attributes
    each an nn.Parameter when named in `params`.  The forward is straight-through on the values the file will hold: colors()
    reads the padded float16 table `rows` (= _rows.half(); sync_rows() refreshes it after an optimizer step, colors() does so
    itself when _rows has been modified in place), the geometry getters return the activation of raw.half().float() -- what is
    trained is exactly what repack() / save() write.  slot (the assignment) is fixed; its inverted index for the backward is
    built once, here."""
    PARAMS = ("rows", "xyz", "opacity", "scaling", "rotation")

    def __init__(self, cg, params=("rows",)):
        params = (params,) if isinstance(params, str) else tuple(params)
        unknown = [p for p in params if p not in self.PARAMS]
        if unknown:
            raise ValueError(f"trainable: unknown parameter names {unknown}; choose from {self.PARAMS}")
        d = cg.sh_dim
        dev = cg.xyz.device
        self._slot = cg._slot
        self.codebook_size, self.sh_dim = cg.codebook_size, d
        self.max_sh_degree, self.active_sh_degree = cg.max_sh_degree, cg.active_sh_degree
        self.rows = cg.rows.detach().clone()
        other = cg._other_raw.to(dev).float()

        def own(name, t):
            t = t.detach().clone().contiguous()
            return torch.nn.Parameter(t) if name in params else t

        self._rows = own("rows", self.rows[:, :d].float())
        self._xyz = own("xyz", cg.xyz)
        self._opacity = own("opacity", other[:, 0:1])
        self._scaling = own("scaling", other[:, 1:4])
        self._rotation = own("rotation", other[:, 4:8])
        # the activations of a tensor that is not trained never change: keep the source's
        self._fixed = {"opacity": cg.opacity, "scaling": cg.scaling, "rotation": cg.rotation}
        self._synced = self._rows._version
        self._index = None
        if dev.type == "cuda":
            self._build_index()

    def _build_index(self):
        """lg_vq_code_index: the inverted index of slot[] (per code, its Gaussians in ascending order), once per model."""
        if not self._xyz.is_cuda:
            raise RuntimeError("TrainableCompressed runs on the MI355X HIP library only (no CPU fallback): use to_dense()")
        lib = _lib.load()
        dev, N, K = self._xyz.device, self.num, self.codebook_size
        nbytes = int(lib.lg_vq_code_index_bytes(N, K))
        if nbytes == 0:
            raise ValueError(f"trainable: no code index for N = {N}, K = {K}")
        self._index = _lib.scratch(nbytes, dev)
        scratch = _lib.scratch(lib.lg_vq_code_index_scratch_bytes(N, K), dev)
        stream = _lib.stream(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.lg_vq_code_index(N, K, _lib.ptr(self._slot), _lib.ptr(self._index), _lib.ptr(scratch), stream))

    def parameters(self):
        """The tensors named in trainable(params=...), for an optimizer."""
        return [t for t in (self._rows, self._xyz, self._opacity, self._scaling, self._rotation) if isinstance(t, torch.nn.Parameter)]

    @property
    def xyz(self):
        return self._xyz

    @property
    def get_xyz(self):
        return self._xyz

    def _activated(self, name, raw, fn):
        if not raw.requires_grad:
            return self._fixed[name]
        return fn(_RoundHalf.apply(raw))

    @property
    def get_opacity(self):
        return self._activated("opacity", self._opacity, torch.sigmoid)

    @property
    def get_scaling(self):
        return self._activated("scaling", self._scaling, torch.exp)

    @property
    def get_rotation(self):
        return self._activated("rotation", self._rotation, torch.nn.functional.normalize)

    opacity, scaling, rotation = get_opacity, get_scaling, get_rotation

    @property
    def _other_raw(self):
        """other_attribute as the file will hold it: float16 [N, 8]"""
        return torch.cat([self._opacity, self._scaling, self._rotation], dim=1).detach().half()

    def to_dense(self):
        """CompressedGaussians.to_dense() of the model as it stands now (detached: the dense model has leaves of its own)."""
        with torch.no_grad():
            if self._rows._version != self._synced:
                self.sync_rows()
            return super().to_dense()

    def sync_rows(self):
        """rows[:, :d] <- _rows.half(): the float16 table the forward reads.  The zero padding of every row is not touched."""
        with torch.no_grad():
            self.rows[:, :self.sh_dim].copy_(self._rows)
        self._synced = self._rows._version

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self._xyz, self._opacity, self._scaling, self._rotation, self._slot, self.rows,
                                                          self._rows) + (() if self._index is None else (self._index,)))

    def colors(self, camera_center, sh_degree=None, out=None, flags=0):
        """CompressedGaussians.colors() on the float16 values of _rows, differentiable: dL/d_rows (and dL/d_xyz when _xyz
        takes gradients) by lg_vq_colors_bwd -- a fixed-order segmented sum onto the codebook rows, no atomics."""
        if not self._xyz.is_cuda:
            raise RuntimeError("CompressedGaussians.colors runs on the MI355X HIP library only (no CPU fallback): use to_dense()")
        if self._rows._version != self._synced:
            self.sync_rows()
        if out is not None or flags or not (torch.is_grad_enabled() and (self._rows.requires_grad or self._xyz.requires_grad)):
            return CompressedGaussians.colors(self, camera_center, sh_degree, out, flags)
        D = self.active_sh_degree if sh_degree is None else int(sh_degree)
        cam = camera_center.detach().to(device=self._xyz.device, dtype=torch.float32).contiguous()
        return _VqColors.apply(self._rows, self._xyz, self, cam, D)

    def repack(self):
        """The seven arrays of pack() for save(): indices and mask as the model came (they follow from slot), rows and
        attributes cast to float16, xyz float32.  Of an untouched trainable(): the dict it was loaded from, bit for bit."""
        K, d, N = self.codebook_size, self.sh_dim, self.num
        bits = _bits_of(K)
        slot = _np(self._slot).astype(np.int64)
        mask = slot >= K
        shifts = np.arange(bits - 1, -1, -1, dtype=np.int64)
        bit_rows = ((slot[~mask][:, None] >> shifts[None, :]) & 1).astype(np.bool_)
        rows = _np(self._rows.detach().half())
        return {
            "metadata": {"input_pc_num": int(N), "input_pc_dim": int(6 + d + 8), "codebook_size": int(K), "codebook_dim": int(d)},
            "vq_indexs": np.packbits(bit_rows.reshape(-1)),
            "codebook": np.ascontiguousarray(rows[:K]),
            "non_vq_mask": np.packbits(mask),
            "non_vq_feats": np.ascontiguousarray(rows[K:]),
            "other_attribute": np.ascontiguousarray(_np(self._other_raw)),
            "xyz": np.ascontiguousarray(_np(self._xyz.detach()), dtype=np.float32),
        }
