"""The sensitivity pieces of lg_math.h on the CPU, through tests/cpu_harness/lg_sensitivity_harness.cpp: the per-hit step against float64
on hand-made rays, the moments -> M -> A^T M A path against blocks formed from the Jacobian of the dense twin on hand-made scenes, the
Cholesky log-det against numpy on the golden blocks, the ranking of -inf scores by the prune masks, and the binding (header, prototype
table, exports, Makefile)."""
import math
import os

import numpy as np
import pytest
import torch

import common
import sensitivity_common as sc
import test_abi
import tolerance
from common import ptr
from lightgaussian_amd import prune, sensitivity

ROOT = common.ROOT

# ---- the per-hit step on one pixel -------------------------------------------------------------------------------------------
# an entry: x, y, ha, nb, hc, opacity, r, g, b  (conic A = 0.02, B = 0.004, C = 0.03: ha = -A/2, nb = -B, hc = -C/2)
_CONIC = (-0.01, -0.004, -0.015)
RAYS = {
    # name -> (entries, background, contributors)
    "one_hit": ([(10.0, 9.0) + _CONIC + (0.6, 0.9, 0.2, 0.4)], (0.0, 0.0, 0.0), 1),
    "two_hits_background": ([(10.0, 9.0) + _CONIC + (0.6, 0.9, 0.2, 0.4), (6.0, 12.0) + _CONIC + (0.8, 0.1, 0.7, 0.3)], (0.2, 0.3, 0.1), 2),
    "occluder": ([(8.5, 8.0) + _CONIC + (1.0, 0.5, 0.5, 0.5), (9.0, 9.0) + _CONIC + (0.7, 0.9, 0.1, 0.2)], (0.2, 0.3, 0.1), 2),      # alpha 0.99 in front: T = 0.01 behind it
    "rejected_entry": ([(10.0, 9.0) + _CONIC + (0.6, 0.9, 0.2, 0.4), (8.0, 8.0) + _CONIC + (0.003, 1.0, 1.0, 1.0),
                        (6.0, 12.0) + _CONIC + (0.8, 0.1, 0.7, 0.3)], (0.2, 0.3, 0.1), 2),                                        # alpha < 1/255 takes no part
    "ends_early": ([(8.0, 8.0) + _CONIC + (1.0, 0.5, 0.5, 0.5), (8.0, 8.5) + _CONIC + (0.9, 0.2, 0.9, 0.1), (8.5, 8.0) + _CONIC + (1.0, 0.9, 0.1, 0.2)],
                   (0.2, 0.3, 0.1), 2),                                                                                           # T: 1 -> 0.01 -> 1.03e-3; the third would leave 1e-5
}
PIXEL = (8.0, 8.0)


def _ray64(entries, bg):
    """float64 on the same float32 inputs: (moments [n, 12], contributors, final T); the decisions are the contract's."""
    e = np.asarray(np.asarray(entries, np.float32), np.float64)
    bg = np.asarray(np.asarray(bg, np.float32), np.float64)
    n = e.shape[0]
    dx, dy = e[:, 0] - PIXEL[0], e[:, 1] - PIXEL[1]
    power = e[:, 2] * dx * dx + e[:, 3] * dx * dy + e[:, 4] * dy * dy
    G = np.exp(np.minimum(power, 0.0))
    alpha = np.minimum(0.99, e[:, 5] * G)
    T, live = 1.0, []
    for k in range(n):
        if power[k] > 0 or alpha[k] < 1.0 / 255.0:
            continue
        if T * (1.0 - alpha[k]) < 1e-4:
            break
        live.append(k)
        T *= 1.0 - alpha[k]
    Tf, S, mom = T, np.zeros(3), np.zeros((n, 12))
    for k in reversed(live):
        inv = 1.0 / (1.0 - alpha[k])
        Tn = T * inv
        v = (e[k, 6:9] - S) * Tn - Tf * bg * inv
        w = float(v @ v) * G[k] ** 2
        x, y = dx[k], dy[k]
        mom[k] = w * np.array([x * x, x * y, y * y, x ** 3, x * x * y, x * y * y, y ** 3, x ** 4, x ** 3 * y, x * x * y * y, x * y ** 3, y ** 4])
        S = S + alpha[k] * (e[k, 6:9] - S)
        T = Tn
    return mom, len(live), Tf


@pytest.mark.parametrize("name", list(RAYS))
def test_step_against_float64(name):
    entries, bg, contributors = RAYS[name]
    rec = np.ascontiguousarray(entries, np.float32)
    bgf = np.asarray(bg, np.float32)
    mom = np.zeros((rec.shape[0], 12), np.float32)
    Tf = np.zeros(1, np.float32)
    n = sc.harness().h_sens_ray(rec.shape[0], ptr(rec), PIXEL[0], PIXEL[1], ptr(bgf), ptr(mom), ptr(Tf))
    want, n64, Tf64 = _ray64(entries, bg)
    assert n64 == contributors, "the float64 walk disagrees with the ray's description"
    assert n == contributors and abs(float(Tf[0]) - Tf64) <= 1e-6
    for k in range(rec.shape[0]):
        if not want[k].any():
            assert not mom[k].any(), f"{name}: entry {k} takes no part, its moments must be exact zeros"
            continue
        # per monomial degree: the moments of one degree share a scale
        for lo, hi in ((0, 3), (3, 7), (7, 12)):
            err = tolerance.rel_err(mom[k, lo:hi], want[k, lo:hi])
            print(f"{name}: entry {k} moments {lo}..{hi - 1} rel err {err:.3e}")
            assert err <= tolerance.TOL


# ---- moments -> M -> A^T M A against the twin's Jacobian --------------------------------------------------------------------
def _view_scene(items, bg, W=16, H=16):
    """Scene kwargs (CPU torch) of Gaussians placed in VIEW space: items = (view position, scales, quaternion, opacity, colour)."""
    cam = common.syn.orbit_camera(1, 8, W, H, radius=4.0, fovx_deg=40)
    inv = torch.linalg.inv(cam.world_view_transform.double())
    xyz = torch.stack([(torch.tensor(tuple(p) + (1.0,), dtype=torch.float64) @ inv)[:3].float() for p, *_ in items])
    rot = torch.tensor([q for _p, _s, q, _o, _c in items], dtype=torch.float32)
    return dict(means3D=xyz, opacities=torch.tensor([[o] for _p, _s, _q, o, _c in items], dtype=torch.float32),
                scales=torch.tensor([s for _p, s, _q, _o, _c in items], dtype=torch.float32), rotations=rot / rot.norm(dim=1, keepdim=True),
                colors_precomp=torch.tensor([c for *_r, c in items], dtype=torch.float32), W=W, H=H, tanfovx=math.tan(cam.FoVx * 0.5),
                tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.tensor(bg, dtype=torch.float32), viewmatrix=cam.world_view_transform,
                projmatrix=cam.full_proj_transform, campos=cam.camera_center, sh_degree=0)


_A = ((0.05, -0.03, 4.0), (0.12, 0.07, 0.09), (0.9, 0.2, -0.3, 0.1), 0.7, (0.9, 0.2, 0.4))
_B = ((-0.1, 0.08, 4.3), (0.10, 0.16, 0.06), (0.7, -0.4, 0.2, 0.5), 0.5, (0.1, 0.7, 0.3))
SCENES = {
    # name -> (items, background, Gaussians with a zero block)
    "single": ([_A], (0.0, 0.0, 0.0), ()),
    "two_background": ([_A, _B], (0.2, 0.3, 0.1), ()),
    "occluder": ([((0.0, 0.0, 3.6), (0.2, 0.2, 0.2), (1.0, 0.0, 0.0, 0.0), 1.0, (0.5, 0.5, 0.5)), _A, _B], (0.2, 0.3, 0.1), ()),
    "rejected": ([_A, ((0.0, 0.0, 3.8), (0.1, 0.1, 0.1), (1.0, 0.0, 0.0, 0.0), 0.003, (1.0, 1.0, 1.0)), _B], (0.2, 0.3, 0.1), (1,)),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_blocks_against_the_twins_jacobian(name):
    """One view: the blocks are singular along the viewing ray by nature (A has five rows), so they are compared entry-wise, scaled by
    the reference's diagonal; the bound is rule 3 on the float32 twin's own figure."""
    items, bg, zero = SCENES[name]
    kw = _view_scene(items, bg)
    got = sc.full(sc.harness_view(kw)[0])
    ref, r32 = sc.twin_blocks(kw, torch.float64), sc.twin_blocks(kw, torch.float32)
    for i in range(len(items)):
        if i in zero:
            print(f"{name}: Gaussian {i} takes no part")
            assert not ref[i].any() and not got[i].any()
            continue
        assert ref[i].diagonal().min() > 0
        floor, err = sc.scaled_err(r32[i:i + 1], ref[i:i + 1])[0], sc.scaled_err(got[i:i + 1], ref[i:i + 1])[0]
        print(f"{name}: Gaussian {i} scaled block error {err:.3e} (float32 twin {floor:.3e}), diagonal {ref[i].diagonal().min():.3e} .. {ref[i].diagonal().max():.3e}")
        assert err <= tolerance.rule3_bound(floor)
    if name == "occluder":      # the occluder hides part of what is behind it: that block is smaller than in the open
        open_blocks = sc.twin_blocks(_view_scene(items[1:], bg), torch.float64)
        assert ref[1].trace() < 0.5 * open_blocks[0].trace()


# ---- the Cholesky log-det ----------------------------------------------------------------------------------------------------
def test_logdet_against_numpy_on_the_golden_blocks():
    z = np.load(sc.GOLDEN)
    blocks = sc.full(z["sum_f64"])
    want = sc.logdet(blocks)
    assert blocks.shape == (24, 6, 6) and np.isfinite(want).all(), "the golden blocks are all positive definite"
    for i in range(24):
        got = sc.harness_logdet(z["sum_f64"][i])
        # Cholesky in float64: the relative error of a pivot is about kappa eps; |d log det| <= 6 kappa eps, far below 1e-9 at kappa <= 13.2
        assert abs(got - want[i]) <= 1e-9 * max(1.0, abs(want[i])), (i, got, want[i])
    print(f"log det {want.min():.3f} .. {want.max():.3f}, kappa <= {sc.kappa(blocks).max():.3g}")


def test_logdet_of_a_block_that_is_not_positive_definite_is_minus_infinity():
    rs = np.random.RandomState(7)
    X = rs.standard_normal((5, 6))
    rank5 = X.T @ X                                         # five directions: singular, the last pivot is rounding of either sign
    assert sc.harness_logdet(sc.tri(rank5)) == -np.inf
    assert sc.harness_logdet(np.zeros(21)) == -np.inf       # never seen
    indefinite = np.diag([1.0, 2.0, -1.0, 1.0, 1.0, 1.0])
    assert sc.harness_logdet(sc.tri(indefinite)) == -np.inf
    z = np.load(sc.GOLDEN)                                  # a single view's block: A has five rows
    assert all(sc.harness_logdet(z["views_f64"][0][i]) == -np.inf for i in range(24))
    full = rank5 + 0.5 * np.eye(6)
    assert abs(sc.harness_logdet(sc.tri(full)) - np.linalg.slogdet(full)[1]) <= 1e-12


# ---- ranking with -inf -------------------------------------------------------------------------------------------------------
def test_prune_masks_rank_minus_infinity_first_and_leave_finite_masks_alone():
    s = torch.tensor([3.0, -np.inf, 7.5, -2.0, -np.inf, 0.5, 11.0, 4.0], dtype=torch.float64)
    mask = prune.prune_mask(0.5, s)                         # index int(0.5 * 7) = 3 of the ascending sort: -inf, -inf, -2, 0.5
    assert mask.tolist() == [False, True, False, True, True, True, False, False]
    assert prune.prune_mask(0.1, s).tolist() == [False, True, False, False, True, False, False, False]      # both -inf go together (ties)
    assert prune.prune_mask_select(0.5, s).tolist() == mask.tolist()
    assert prune.prune_mask_threshold(s, -100.0).tolist() == [False, True, False, False, True, False, False, False]
    finite = torch.tensor([3.0, 7.5, -2.0, 0.5, 11.0, 4.0], dtype=torch.float64)
    assert prune.prune_mask(0.5, finite).tolist() == [True, False, True, True, False, False]          # index int(0.5 * 5) = 2: the value 3


# ---- the binding -------------------------------------------------------------------------------------------------------------
def test_header_matches_binding():
    declared = test_abi.check_extension_header("lightgaussian_sensitivity.h", sensitivity.PROTOTYPES)
    assert len(declared) == 3 and declared["lg_sensitivity_score"] == ("int32", ["int32", "pointer", "pointer", "pointer", "pointer"])
    text = open(os.path.join(ROOT, "include", "lightgaussian_sensitivity.h")).read()
    assert "#define LG_ABI_VERSION" not in text and '#include "lightgaussian.h"' in text
    make = open(os.path.join(ROOT, "lightgaussian_amd", "csrc", "Makefile")).read()
    assert "lg_sensitivity.h" in make and "lightgaussian_sensitivity.h" in make


def test_library_exports_and_host_side_answers():
    lib = sensitivity.load()
    assert all(hasattr(lib, name) for name in sensitivity.PROTOTYPES)
    assert lib.lg_abi_version() == 7
    assert lib.lg_sensitivity_scratch_bytes(10, 1000) >= 1000 * 48 and lib.lg_sensitivity_scratch_bytes(10, 0) > 0
    assert lib.lg_sensitivity_scratch_bytes(10, -1) == 0
    # refusals before any device call
    from lightgaussian_amd import _lib
    assert lib.lg_sensitivity_accumulate(None, None, None, None, None, None, 0, None, None, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_sensitivity_score(4, None, None, None, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_sensitivity_score(0, None, None, None, None) == _lib.LG_OK


def test_python_refusals_without_a_device():
    with pytest.raises(ValueError, match="scale_space"):
        sensitivity.score(torch.zeros(2, 21, dtype=torch.float64), scale_space="sqrt")
    with pytest.raises(RuntimeError, match="no CPU path"):
        sensitivity.score(torch.zeros(2, 21, dtype=torch.float64))
    with pytest.raises(ValueError):
        sensitivity.score(torch.zeros(21, dtype=torch.float64))
