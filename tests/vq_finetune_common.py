"""Helpers of test_gpu_vq_finetune.py / test_vq_finetune_host.py: small packed scenes (random and hand-built assignments), the
torch restatement of the compressed model's colour stage, and the dL/dcolours of one rasterizer backward."""
import functools
import math

import numpy as np
import torch

from common import syn
from lightgaussian_amd import vectree
from lightgaussian_amd.gaussian_renderer import render
from lightgaussian_amd.sh_utils import eval_sh

DEV = "cuda:0"
UNFUSED = {"fuse_getters": False}
W, H = 320, 240
ALL_PARAMS = ("rows", "xyz", "opacity", "scaling", "rotation")


def ply_rows(g):
    """The PLY table of a SyntheticGaussians (scene/gaussian_model.py save_ply order): f_rest channel-major."""
    N = g.num
    return torch.cat([g._xyz, torch.zeros(N, 3), g._features_dc.transpose(1, 2).reshape(N, 3),
                      g._features_rest.transpose(1, 2).reshape(N, -1), g._opacity, g._scaling, g._rotation], dim=1).contiguous()


def scene(N, deg, seed=1, scale=0.02, rest_std=0.25):
    """rest_std well above the generator's default and the base colour lowered by 0.14 (0.5 in SH units): a good share of the
    colour channels falls below 0 and is clamped, at active degree 0 too."""
    g = syn.make_gaussians(N, sh_degree=deg, seed=seed, log_scale_mean=math.log(scale), rest_std=rest_std)
    g._features_dc.sub_(0.5)
    return g


def packed_random(N, deg, vq_ratio, K=256, seed=1):
    """Random assignment: the codebook is K of the scene's SH rows plus noise, every row gets a random code, the
    int(N (1 - vq_ratio)) rows of largest random importance keep a row of their own."""
    feats = ply_rows(scene(N, deg, seed))
    d = 3 * (deg + 1) ** 2
    gen = torch.Generator().manual_seed(100 + seed)
    codebook = feats[torch.randint(0, N, (K,), generator=gen), 6:6 + d] + 0.02 * torch.randn(K, d, generator=gen)
    ind = torch.randint(0, K, (N,), generator=gen)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[torch.topk(torch.rand(N, generator=gen), k=int(N * (1 - vq_ratio))).indices] = True
    return vectree.pack(feats, mask, codebook, ind)


HAND_K = 16
HAND_EMPTY = (13, 14, 15)


def packed_by_hand(N, deg, seed=1):
    """K = 16, 40 % of the rows non-VQ; among the VQ Gaussians code 0 holds 600 (three chunks of the segmented sum), code 1
    exactly 256 (one full chunk), code 2 exactly 257 (a chunk of one), codes 13..15 nobody, codes 3..12 the rest at random."""
    feats = ply_rows(scene(N, deg, seed))
    d = 3 * (deg + 1) ** 2
    gen = torch.Generator().manual_seed(300 + seed)
    codebook = feats[torch.randint(0, N, (HAND_K,), generator=gen), 6:6 + d] + 0.02 * torch.randn(HAND_K, d, generator=gen)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[torch.topk(torch.rand(N, generator=gen), k=int(N * 0.4)).indices] = True
    vq = torch.nonzero(~mask).reshape(-1)
    vq = vq[torch.randperm(vq.numel(), generator=gen)]
    assert vq.numel() >= 600 + 256 + 257 + 100
    ind = torch.zeros(N, dtype=torch.int64)
    ind[vq[:600]] = 0
    ind[vq[600:856]] = 1
    ind[vq[856:1113]] = 2
    ind[vq[1113:]] = torch.randint(3, 13, (vq.numel() - 1113,), generator=gen)
    return vectree.pack(feats, mask, codebook, ind)


def packed_case(N, deg, how, seed=1):
    """how: a vq_ratio (random assignment, K = 256) or "hand"."""
    return packed_by_hand(N, deg, seed) if how == "hand" else packed_random(N, deg, how, seed=seed)


def bits(t):       # (not common.bits: an int32 torch view on the device, for torch.equal)
    return t.detach().contiguous().view(torch.int32)


def file_order_to_m3(rows, M):
    """[n, 3 M] in the file's column order -> [n, M, 3]"""
    n = rows.shape[0]
    return torch.cat([rows[:, 0:3].reshape(n, 3, 1), rows[:, 3:].reshape(n, 3, M - 1)], dim=2).transpose(1, 2)


def m3_to_file_order(sh):
    """[n, M, 3] -> [n, 3 M] in the file's column order"""
    n = sh.shape[0]
    return torch.cat([sh[:, 0, :], sh[:, 1:, :].transpose(1, 2).reshape(n, -1)], dim=1)


def restated_gradients(rows, xyz, slot, campos, D, M, g, dtype):
    """The colour stage in torch at `dtype` on the dequantised values: rows[slot] -> [N, 3, M] -> eval_sh, + 0.5, clamp_min(0);
    backward of `g` (dL/dcolours).  Returns (dL/drows [n_rows, 3 M], dL/dxyz [N, 3], colours)."""
    rows = rows.detach().to(dtype).requires_grad_(True)
    xyz = xyz.detach().to(dtype).requires_grad_(True)
    sh = file_order_to_m3(rows[slot.long()], M).transpose(1, 2)
    dirs = xyz - campos.to(dtype)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    col = torch.clamp_min(eval_sh(D, sh, dirs) + 0.5, 0.0)
    col.backward(g.to(dtype))
    return rows.grad, (xyz.grad if xyz.grad is not None else torch.zeros_like(xyz)), col.detach()


@functools.lru_cache(maxsize=None)
def target_image(k):
    """The render of a second scene: what the L1 losses of these tests compare against."""
    g = scene(2500, 1, seed=41, scale=0.05).to(DEV)
    with torch.no_grad():
        return render(syn.orbit_camera(k, 8, W, H).to(DEV), g, syn.PipelineParams(), torch.tensor([0.3, 0.2, 0.1], device=DEV))["render"].clone()


def l1(img, target):
    return (img - target).abs().mean()


def dl_dcolors(model, cam, k, bg):
    """dL/dcolours [N, 3] of one rasterizer backward: L1 of the model's render against target_image(k)."""
    with torch.no_grad():
        col = model.colors(cam.camera_center).clone()
    col.requires_grad_(True)
    pkg = render(cam, model, syn.PipelineParams(), bg, override_color=col, options=UNFUSED)
    l1(pkg["render"], target_image(k)).backward()
    return col.grad.detach().clone()


def np_equal_packed(a, b):
    """Two packed dicts equal in all seven arrays, bit for bit (dtype and shape included)."""
    if set(a) != set(b) or dict(a["metadata"]) != dict(b["metadata"]):
        return False
    for name in vectree.FILES[1:]:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True
