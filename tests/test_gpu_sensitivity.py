"""lightgaussian_amd.sensitivity on the GPU: the per-Gaussian 6 x 6 blocks of lg_sensitivity_walk / lg_sensitivity_accum and the scores of
lg_sensitivity_score against the golden blocks of the dense twin (tests/golden/sensitivity_blocks.npz), against a brute force through
the existing backward, and the properties of the accumulation: additive over views, deterministic, independent of what the scratch held,
the edge cases, the ranking."""
import functools
import math

import numpy as np
import pytest
import torch

import common
import poison_common
import sensitivity_common as sc
import tolerance
from common import syn
from lightgaussian_amd import _lib, prune, sensitivity
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIPE = syn.PipelineParams()


def _bg():
    return torch.tensor(sc.GOLDEN_BG, dtype=torch.float32, device=DEV)


def _accumulate(g, colors, cams, H=None, **kw):
    gd, cd = g.to(DEV), colors.to(DEV)
    for cam in cams:
        H = sensitivity.accumulate(cam.to(DEV), gd, PIPE, _bg(), H, override_color=cd, **kw)
    return H


@functools.lru_cache(maxsize=None)
def _golden():
    """(reference dict of the golden file, kernel H per view [2, 24, 21], kernel H of both views [24, 21], kernel scores [24]): once."""
    z = dict(np.load(sc.GOLDEN))
    g, colors, cams = sc.golden_scene()
    views = [_accumulate(g, colors, [cam]) for cam in cams]
    both = _accumulate(g, colors, cams)
    score = sensitivity.score(both)
    torch.cuda.synchronize()
    return z, np.stack([v.cpu().numpy() for v in views]), both.cpu().numpy(), score.cpu().numpy()


def _bounds(ref, r32):
    """Per Gaussian: the float32 twin's scaled error (the floor), the rule-3 bound on it, kappa of the scaled reference block."""
    floor = sc.scaled_err(r32, ref)
    return floor, np.array([tolerance.rule3_bound(f) for f in floor]), sc.kappa(ref)


def test_golden_scene_blocks_and_scores():
    z, views, both, score = _golden()
    ref, r32, got = sc.full(z["sum_f64"]), sc.full(z["sum_f32"]), sc.full(both)
    floor, bound, kap = _bounds(ref, r32)
    err = sc.scaled_err(got, ref)
    ld = sc.logdet(ref)
    assert np.isfinite(ld).all() and np.isfinite(kap).all(), "the golden blocks are positive definite"
    bad = []
    for i in range(24):
        dl = abs(score[i] - ld[i])
        print(f"Gaussian {i:2d}: scaled block error {err[i]:.3e} (float32 twin {floor[i]:.3e}, bound {bound[i]:.3e}), kappa {kap[i]:.3g}, "
              f"log det {score[i]:.6f} (twin {ld[i]:.6f}, |d| {dl:.3e}, bound {6 * kap[i] * bound[i]:.3e})")
        if not (err[i] <= bound[i] and dl <= 6 * kap[i] * bound[i]):
            bad.append(i)
    assert not bad, f"Gaussians {bad} miss their bound"
    # a single view's block is singular along the viewing ray by nature: entries only
    for v in range(2):
        rv, rv32, gv = sc.full(z["views_f64"][v]), sc.full(z["views_f32"][v]), sc.full(views[v])
        fl, bd, _ = _bounds(rv, rv32)
        ev = sc.scaled_err(gv, rv)
        print(f"view {int(z['views'][v])}: worst scaled block error {ev.max():.3e} (float32 twin {fl.max():.3e}); worst error / bound {float((ev / bd).max()):.3f}")
        assert (ev <= bd).all(), f"view {v}: Gaussians {np.flatnonzero(ev > bd).tolist()} miss their bound"


def _brute_blocks(g, colors, cams):
    """[N, 6, 6] float64 on the host: the sum over the views and over every one-hot image gradient of g g^T, g = the existing backward's
    gradient with respect to (means3D, scales) of render(..., colors_precomp)."""
    gd = g.to(DEV)
    with torch.no_grad():
        xyz, sc_, rot, op = gd.get_xyz.clone(), gd.get_scaling.clone(), gd.get_rotation.clone(), gd.get_opacity.clone()
    xyz.requires_grad_(True); sc_.requires_grad_(True)
    col = colors.to(DEV)
    n = xyz.shape[0]
    H = torch.zeros((n, 6, 6), dtype=torch.float64, device=DEV)
    for cam in cams:
        cam = cam.to(DEV)
        rs = GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
                                           tanfovy=math.tan(cam.FoVy * 0.5), bg=_bg(), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                                           projmatrix=cam.full_proj_transform, sh_degree=0, campos=cam.camera_center, prefiltered=False,
                                           debug=False, f_count=False)
        means2D = torch.zeros((n, 3), device=DEV, requires_grad=True)
        color, _radii = GaussianRasterizer(rs)(means3D=xyz, means2D=means2D, opacities=op, colors_precomp=col, scales=sc_, rotations=rot)
        onehot = torch.zeros_like(color)
        flat = onehot.view(-1)
        for p in range(flat.numel()):
            flat[p] = 1.0
            gm, gs = torch.autograd.grad(color, (xyz, sc_), grad_outputs=onehot, retain_graph=True)
            flat[p] = 0.0
            j = torch.cat([gm, gs], 1).double()
            H += j[:, :, None] * j[:, None, :]
    torch.cuda.synchronize()
    return H.cpu().numpy()


def test_brute_force_through_the_existing_backward():
    """The reference is the existing backward: g g^T summed in float64 over every one-hot image gradient, 2880 per view.  A single view's
    blocks have rank 5 -- their kappa is infinite and the kappa rule would leave every Gaussian out -- so the scene has two views 90 degrees
    apart, 5760 backward passes in all.  Both sides carry float32 rounding of the same chain: twice the bound of the golden test, whose
    floors (the float32 twin's, about 1e-6) all lie below a third of rule 3's 1e-4 -- so 2e-4 on the scaled entries.  Left out only where
    the reference's kappa is above 1e3; the share must be below 10 %."""
    g, colors, cams = sc.brute_scene()
    ref = _brute_blocks(g, colors, cams)
    got = sc.full(_accumulate(g, colors, cams).cpu().numpy())
    walk, info = None, []
    for cam in cams:
        walk, _radii, i = sc.harness_view(sc.scene_kw(g, colors, cam, sc.BRUTE_W, sc.BRUTE_H, sc.GOLDEN_BG), walk)
        info.append(i)
    print(f"lists: {info}")
    assert all(i["longest"] > 64 and i["early"] > 0 for i in info), "the scene must have lists longer than one batch and rays that end early"
    kap = sc.kappa(ref)
    keep = kap <= 1e3
    share = 1.0 - float(keep.mean())
    print(f"left out (kappa > 1e3): {int((~keep).sum())} of {len(kap)} = {100 * share:.1f} %")
    assert share < 0.10
    err, cpu = sc.scaled_err(got, ref), sc.scaled_err(sc.full(walk), ref)
    bound = 2.0 * tolerance.rule3_bound(0.0)
    ratio = err[keep] / bound
    print(f"worst scaled block error {err[keep].max():.3e} (the CPU walk of the same arithmetic: {cpu[keep].max():.3e}); bound {bound:.1e}; "
          f"worst error / bound {ratio.max():.3f}; over all 200 Gaussians {err.max():.3e}")
    assert (ratio <= 1.0).all(), f"Gaussians {np.flatnonzero(keep)[ratio > 1.0].tolist()} miss their bound"


def test_views_add_in_float64_bit_for_bit():
    g, colors, cams = sc.golden_scene()
    a, b = _accumulate(g, colors, cams[:1]), _accumulate(g, colors, cams[1:])
    ab = _accumulate(g, colors, cams)
    assert a.abs().sum() > 0 and b.abs().sum() > 0
    assert torch.equal(ab, a + b)


def test_two_runs_give_identical_bits():
    z, _views, both, score = _golden()
    g, colors, cams = sc.golden_scene()
    again = _accumulate(g, colors, cams)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), both.view(np.uint64))
    assert np.array_equal(sensitivity.score(again).cpu().numpy().view(np.uint64), score.view(np.uint64))


def test_result_does_not_depend_on_what_the_scratch_held():
    g, colors, cams = sc.golden_scene()

    def run():
        H = _accumulate(g, colors, cams)
        return dict(H=H, score=sensitivity.score(H), log=sensitivity.score(H, g.to(DEV), "log"))

    poison_common.assert_identical(poison_common.run_all(run), "sensitivity")


def test_empty_model():
    g, colors, cams = sc.golden_scene()
    empty = syn.SyntheticGaussians(g._xyz[:0], g._features_dc[:0], g._features_rest[:0], g._scaling[:0], g._rotation[:0], g._opacity[:0],
                                   g.max_sh_degree, g.active_sh_degree)
    H = _accumulate(empty, colors[:0], cams[:1])
    assert tuple(H.shape) == (0, 21) and H.dtype == torch.float64
    assert tuple(sensitivity.score(H).shape) == (0,)


def test_a_gaussian_behind_the_camera_keeps_zeros_and_scores_minus_infinity():
    g, colors, cams = sc.golden_scene()
    with torch.no_grad():
        g._xyz[5] = torch.tensor([0.0, 0.0, -8.0])          # view 0 stands at (0, 0, -6) and looks along +z
    H = _accumulate(g, colors, cams[:1])
    assert not H[5].any() and H[4].any()
    s = sensitivity.score(_accumulate(g, colors, cams[1:], H))      # (the second view does not see it either: outside its frustum)
    print(f"scores: {s.cpu().numpy()}")
    assert torch.isfinite(s[4]) and not H[5].any()
    assert s[5] == -math.inf


def test_another_segment_length_than_the_forwards_adds_nothing():
    g, colors, cams = sc.golden_scene()
    state = sensitivity._forward(cams[0].to(DEV), g.to(DEV), PIPE, _bg(), None, colors.to(DEV))
    assert state[-1] > 0
    H = sensitivity.new_accumulator(24, torch.device(DEV))
    state[0].view.segment_length = 128 if int(state[0].view.segment_length) != 128 else 256
    sensitivity._accumulate_view(state, H)
    torch.cuda.synchronize()
    assert not H.any()


def test_antialiasing_is_refused():
    g, colors, cams = sc.golden_scene()
    with pytest.raises(NotImplementedError, match="antialiasing"):
        _accumulate(g, colors, cams[:1], options={"antialiasing": True})
    state = sensitivity._forward(cams[0].to(DEV), g.to(DEV), PIPE, _bg(), None, colors.to(DEV))
    state[0].view.flags |= _lib.FLAG_ANTIALIAS
    with pytest.raises(Exception, match="LG_FLAG_ANTIALIAS"):
        sensitivity._accumulate_view(state, sensitivity.new_accumulator(24, torch.device(DEV)))


def test_log_scale_space_adds_twice_the_log_scales():
    _z, _views, both, score = _golden()
    g = sc.golden_scene()[0].to(DEV)
    H = torch.tensor(both, device=DEV)
    log = sensitivity.score(H, g, scale_space="log")
    s = g.get_scaling.detach().float().double()
    want = torch.tensor(score, device=DEV) + 2.0 * ((torch.log(s[:, 0]) + torch.log(s[:, 1])) + torch.log(s[:, 2]))
    diff = (log - want).abs().max().item()
    print(f"log-space score against linear + 2 sum log s: max |d| {diff:.3e}")
    assert torch.equal(log, want)
    with pytest.raises(ValueError, match="model"):
        sensitivity.score(H, None, scale_space="log")


def test_ranking_matches_the_references():
    z, _views, _both, score = _golden()
    ref, r32 = sc.full(z["sum_f64"]), sc.full(z["sum_f32"])
    _floor, bound, kap = _bounds(ref, r32)
    ld = sc.logdet(ref)
    want = prune.prune_mask(0.5, torch.tensor(ld)).numpy()
    got = prune.prune_mask(0.5, torch.tensor(score)).numpy()
    thr = np.sort(ld)[int(0.5 * 23)]
    near = np.abs(ld - thr) <= 6 * kap * bound
    print(f"threshold {thr:.6f}; within their bound of it: {np.flatnonzero(near).tolist()}; masks differ at {np.flatnonzero(want != got).tolist()}")
    assert want.sum() == 12 and ((want == got) | near).all()
    # -inf ranks first, on the device's radix select as in the sort
    s = torch.tensor(score, dtype=torch.float32, device=DEV)
    s[[3, 17]] = -math.inf
    _thr, mask = prune._select_mask(s, int(0.25 * 23))
    assert torch.equal(mask.bool().cpu(), prune.prune_mask(0.25, s.cpu())) and mask[3] and mask[17]
