"""-m gpu: rendering a VecTree-compressed model from its compressed form (vectree.CompressedGaussians, lg_vq_colors,
gaussian_renderer.render_compressed) against the dense path on the dequantised model, the CPU oracle and sh_utils.eval_sh; and
the whole quantisation stage (vectree.quantize_model) against topk and the nearest-code oracle."""
import math

import numpy as np
import pytest
import torch

import common
import gpu_common
from common import syn
from lightgaussian_amd import _lib, gaussian_renderer, vectree
from lightgaussian_amd.gaussian_renderer import render, render_compressed
from lightgaussian_amd.sh_utils import eval_sh
from oracle import oracle, vq_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNFUSED = {"fuse_getters": False}        # K1 reads the activated tensors and the SH table: the comparand of the colour kernel


def ply_rows(g):
    """The PLY table of a SyntheticGaussians (scene/gaussian_model.py save_ply order): f_rest channel-major."""
    N = g.num
    return torch.cat([g._xyz, torch.zeros(N, 3), g._features_dc.transpose(1, 2).reshape(N, 3),
                      g._features_rest.transpose(1, 2).reshape(N, -1), g._opacity, g._scaling, g._rotation], dim=1).contiguous()


def packed_scene(N, deg, vq_ratio, K=256, seed=1, scale=0.02):
    """A synthetic scene packed with a random codebook assignment: the codebook is K of its SH rows plus noise, every row gets
    a random code, the int(N (1 - vq_ratio)) rows of largest random importance stay non-VQ."""
    g = syn.make_gaussians(N, sh_degree=deg, seed=seed, log_scale_mean=math.log(scale))
    feats = ply_rows(g)
    d = 3 * (deg + 1) ** 2
    gen = torch.Generator().manual_seed(100 + seed)
    codebook = feats[torch.randint(0, N, (K,), generator=gen), 6:6 + d] + 0.02 * torch.randn(K, d, generator=gen)
    ind = torch.randint(0, K, (N,), generator=gen)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[torch.topk(torch.rand(N, generator=gen), k=int(N * (1 - vq_ratio))).indices] = True
    return vectree.pack(feats, mask, codebook, ind)


def bits(t):       # (not common.bits: an int32 torch view on the device, for torch.equal)
    return t.detach().contiguous().view(torch.int32)


# N (small ones not divisible by 64), max degree, active degree, vq_ratio
PARITY = [(3001, 3, 3, 0.6), (4999, 2, 2, 0.6), (3001, 3, 1, 0.6), (2113, 3, 3, 0.0), (2113, 2, 2, 1.0), (2113, 2, 0, 1.0),
          (200003, 3, 3, 0.6), (200003, 2, 2, 0.6)]


@pytest.mark.parametrize("N,deg,active,ratio", PARITY)
def test_compressed_render_equals_the_dense_render_bit_for_bit(N, deg, active, ratio):
    cg = vectree.CompressedGaussians.from_packed(packed_scene(N, deg, ratio, scale=0.02 if N < 10000 else 0.008), DEV)
    cg.active_sh_degree = active
    dense = cg.to_dense()
    assert dense.active_sh_degree == active and dense.max_sh_degree == deg
    pipe = syn.PipelineParams()
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    for k in (1, 6):
        cam = syn.orbit_camera(k, 8, 320, 240).to(DEV)
        a = render_compressed(cam, cg, pipe, bg, options=UNFUSED)
        with torch.no_grad():
            b = render(cam, dense, pipe, bg, options=UNFUSED)
        assert int((b["radii"] > 0).sum()) > N // 20
        diff = (a["render"] - b["render"]).abs().max().item()
        print(f"N {N} degree {active}/{deg} vq_ratio {ratio} camera {k}: max |compressed - dense| = {diff:.3g}")
        assert torch.equal(a["radii"], b["radii"])
        assert torch.equal(bits(a["render"]), bits(b["render"])), diff
        assert torch.equal(a["visibility_filter"], b["visibility_filter"])
        assert set(a) == set(b) and not any(torch.is_tensor(v) and v.requires_grad for v in a.values())


def test_compressed_render_against_the_cpu_oracle():
    N, W, H = 20000, 320, 240
    cg = vectree.CompressedGaussians.from_packed(packed_scene(N, 3, 0.6, seed=3), DEV)
    cam = syn.orbit_camera(3, 16, W, H)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    img = render_compressed(cam.to(DEV), cg, syn.PipelineParams(), bg)["render"].cpu().numpy()
    dense = cg.to_dense()
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    ref = oracle.forward(means3D=c(dense.get_xyz), opacities=c(dense.get_opacity), W=W, H=H, tanfovx=math.tan(cam.FoVx * 0.5),
                         tanfovy=math.tan(cam.FoVy * 0.5), bg=bg.cpu().numpy(), viewmatrix=cam.world_view_transform.numpy(),
                         projmatrix=cam.full_proj_transform.numpy(), campos=cam.camera_center.numpy(), sh_degree=3,
                         shs=c(dense.get_features), scales=c(dense.get_scaling), rotations=c(dense.get_rotation))
    err = gpu_common.rel_err(img, ref.color)
    print(f"compressed render against the oracle: rel err {err:.3g}")
    assert err <= 1e-4


@pytest.mark.parametrize("deg,active,ratio", [(3, 3, 0.6), (3, 2, 0.6), (3, 1, 0.0), (3, 0, 1.0), (2, 2, 0.6), (2, 1, 1.0)])
def test_lg_vq_colors_against_eval_sh(deg, active, ratio):
    N = 50021
    cg = vectree.CompressedGaussians.from_packed(packed_scene(N, deg, ratio, seed=5), DEV)
    campos = torch.tensor([0.3, -0.2, 5.5], device=DEV)
    got = cg.colors(campos, sh_degree=active)
    dense = cg.to_dense()

    def colours(dtype):
        sh = dense.get_features.to(dtype).transpose(1, 2)
        dirs = dense.get_xyz.to(dtype) - campos.to(dtype)
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        return torch.clamp_min(eval_sh(active, sh, dirs) + 0.5, 0.0)

    ref32, ref64 = colours(torch.float32), colours(torch.float64)
    dev32 = (ref32.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    print(f"lg_vq_colors degree {active}/{deg}: |kernel - float64| {err:.3g}, |torch float32 - float64| {dev32:.3g}")
    assert dev32 > 0 and err <= 4 * dev32
    assert got.min().item() >= 0.0
    if active == deg:
        assert (ref64 == 0).sum().item() > 10 and (got == 0).any()         # the clamp is exercised


def test_peak_memory_of_the_compressed_render():
    N, deg = 1_000_003, 3
    d = 48
    packed = packed_scene(N, deg, 0.6, K=8192, seed=9, scale=0.004)
    cam = syn.orbit_camera(2, 8, 640, 360).to(DEV)
    pipe = syn.PipelineParams()
    bg = torch.zeros(3, device=DEV)
    cg = vectree.CompressedGaussians.from_packed(packed, DEV)
    del packed
    cg_sh_bytes = cg.rows.numel() * 2 + 4 * N
    render_compressed(cam, cg, pipe, bg)                                   # warm-up: code objects, the shared zero buffer

    from torch.utils._python_dispatch import TorchDispatchMode

    class NoDenseTable(TorchDispatchMode):
        worst = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            for t in (out if isinstance(out, (tuple, list)) else (out,)):
                if torch.is_tensor(t) and t.dtype == torch.float32:
                    NoDenseTable.worst = max(NoDenseTable.worst, t.numel())
            return out

    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    with NoDenseTable():
        a = render_compressed(cam, cg, pipe, bg)
    torch.cuda.synchronize()
    peak_c = torch.cuda.max_memory_allocated()
    assert NoDenseTable.worst < N * d, "a float32 tensor of the SH table's size was created"
    img_c = a["render"].clone()
    dense = cg.to_dense()
    del cg, a
    dense_sh_bytes = 4 * (dense._features_dc.numel() + dense._features_rest.numel())
    with torch.no_grad():
        render(cam, dense, pipe, bg)
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        b = render(cam, dense, pipe, bg)                                   # the parent's way: the fused-getter forward on the dense model
    torch.cuda.synchronize()
    peak_d = torch.cuda.max_memory_allocated()
    need = 0.9 * (dense_sh_bytes - cg_sh_bytes - 12 * N)
    print(f"peak allocated: compressed {peak_c / 1e6:.1f} MB, dense {peak_d / 1e6:.1f} MB, saved {(peak_d - peak_c) / 1e6:.1f} MB, "
          f"required {need / 1e6:.1f} MB (dense SH {dense_sh_bytes / 1e6:.1f} MB, compressed SH {cg_sh_bytes / 1e6:.1f} MB)")
    assert need > 100e6 and peak_d - peak_c >= need
    assert gpu_common.rel_err(img_c.cpu().numpy(), b["render"].cpu().numpy()) <= 1e-4


def test_two_calls_give_the_same_bits():
    cg = vectree.CompressedGaussians.from_packed(packed_scene(100003, 3, 0.6, seed=11, scale=0.01), DEV)
    cam = syn.orbit_camera(5, 8, 320, 240).to(DEV)
    bg = torch.tensor([0.0, 0.5, 1.0], device=DEV)
    a = render_compressed(cam, cg, syn.PipelineParams(), bg)
    c1 = cg.colors(cam.camera_center).clone()
    b = render_compressed(cam, cg, syn.PipelineParams(), bg)
    assert torch.equal(bits(a["render"]), bits(b["render"])) and torch.equal(a["radii"], b["radii"])
    assert torch.equal(bits(c1), bits(cg.colors(cam.camera_center)))


def test_render_dispatches_on_the_model_type(monkeypatch):
    cg = vectree.CompressedGaussians.from_packed(packed_scene(3001, 3, 0.6), DEV)
    dense = cg.to_dense()
    cam = syn.orbit_camera(1, 8, 160, 120).to(DEV)
    pipe = syn.PipelineParams()
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    calls = []
    real = gaussian_renderer.render_compressed
    monkeypatch.setattr(gaussian_renderer, "render_compressed", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    via_render = render(cam, cg, pipe, bg)
    assert calls == [1]
    assert torch.equal(bits(via_render["render"]), bits(real(cam, cg, pipe, bg)["render"]))
    with torch.no_grad():
        fused = render(cam, dense, pipe, bg)
        unfused = render(cam, dense, pipe, bg, options=UNFUSED)
        assert calls == [1]                                                 # a dense model never takes the compressed route
        assert torch.equal(bits(fused["render"]), bits(gaussian_renderer.render_fused(cam, dense, pipe, bg)["render"]))
        assert torch.equal(bits(unfused["render"]), bits(gaussian_renderer._render_unfused(cam, dense, pipe, bg)["render"]))
        # override_color: the ordinary path, for either model
        col = torch.rand(3001, 3, device=DEV)
        assert torch.equal(bits(render(cam, cg, pipe, bg, override_color=col)["render"]),
                           bits(render(cam, dense, pipe, bg, override_color=col, options=UNFUSED)["render"]))
    assert calls == [1]
    with pytest.raises(Exception):
        _lib.check(_lib.load().lg_vq_colors(10, 16, 3, cg.xyz.data_ptr(), bg.data_ptr(), cg.slot.data_ptr(), cg.rows.data_ptr(), 40,
                                            cg.xyz.data_ptr(), 0, None))   # a stride that is no multiple of 16


def test_the_whole_quantisation_stage():
    N, deg, K, d = 100003, 2, 256, 27
    gen = torch.Generator().manual_seed(77)
    centres = 0.5 * torch.randn(K, d, generator=gen)
    g = syn.make_gaussians(N, sh_degree=deg, seed=13)
    feats = ply_rows(g)
    feats[:, 6:6 + d] = centres[torch.randint(0, K, (N,), generator=gen)] + 0.1 * torch.randn(N, d, generator=gen)
    importance = (torch.randperm(N, generator=gen).float() + 1.0) / N       # tie-free
    embed0 = feats[torch.randperm(N, generator=gen)[:K], 6:6 + d] + 0.05 * torch.randn(K, d, generator=gen)

    def near_ties(codebook):
        x = feats[:, 6:6 + d].numpy()
        ref, gap = vq_oracle.nearest_code(x, codebook)
        best = np.sqrt(((x.astype(np.float64) - codebook.astype(np.float64)[ref]) ** 2).sum(1))
        return ref, gap < 1e-4 * best.mean()

    # the inputs themselves (CPU): against the start codebook, fp16-rounded, far fewer than 2 % of the rows are near ties
    assert near_ties(embed0.half().float().numpy())[1].mean() <= 0.02
    dgen = torch.Generator(device=DEV).manual_seed(5)
    packed = vectree.quantize_model(feats.to(DEV), importance.to(DEV), vq_ratio=0.6, codebook_size=K, iterations=4, chunk=20000,
                                    embed=embed0.to(DEV), generator=dgen)
    n_keep = int(N * (1 - 0.6))
    mask = np.unpackbits(packed["non_vq_mask"])[:N].astype(bool)
    want = np.zeros(N, bool)
    want[torch.topk(importance, k=n_keep, largest=True).indices.numpy()] = True
    assert np.array_equal(mask, want) and mask.sum() == n_keep
    assert packed["codebook"].dtype == np.float16 and packed["codebook"].shape == (K, d)
    codebook = packed["codebook"].astype(np.float32)
    assert not np.array_equal(codebook, embed0.half().float().numpy())      # it was trained
    ref, tie = near_ties(codebook)
    print(f"near ties against the trained codebook: {100 * tie.mean():.3f} % of the rows")
    assert tie.mean() <= 0.02
    table = vectree.unpack(packed).numpy()
    codes = vectree._decode(packed)[5]
    judged = ~tie[~mask]
    assert np.array_equal(codes[judged], ref[~mask][judged]), int((codes[judged] != ref[~mask][judged]).sum())
    assert np.array_equal(table[~mask, 6:6 + d], codebook[codes])                                   # VQ rows: codebook rows
    assert np.array_equal(table[mask, 6:6 + d], feats[:, 6:6 + d].half().float().numpy()[mask])     # non-VQ rows: fp16-rounded inputs
    assert np.array_equal(table[:, -8:], feats[:, -8:].half().float().numpy()) and np.array_equal(table[:, :3], feats[:, :3].numpy())
    # and the model renders
    cg = vectree.CompressedGaussians.from_packed(packed, DEV)
    out = render(syn.orbit_camera(0, 8, 160, 120).to(DEV), cg, syn.PipelineParams(), torch.zeros(3, device=DEV))
    assert torch.isfinite(out["render"]).all() and int((out["radii"] > 0).sum()) > 0
