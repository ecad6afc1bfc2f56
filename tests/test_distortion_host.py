"""lg_distortion_step / lg_distortion_bwd_step (lg_math.h) on the CPU, through tests/cpu_harness/lg_distortion_harness.cpp: hand-made rays
against float64, the accuracy on thin slabs that is the reason the kernel exists, the backward replay against float64 autograd, and
the binding (header, prototype table, exports, Makefile)."""
import os

import numpy as np
import pytest
import torch

import common
import distortion_common as dc
import test_abi
import tolerance
from lightgaussian_amd import distortion

ROOT = common.ROOT

# name -> (alphas, m, index of the median entry, contributors)
RAYS = {
    "one_hit": ([0.5], [3.0], 0, 1),
    "two_hits_median_is_second": ([0.3, 0.9], [2.0, 2.5], 1, 2),                     # T: 1 -> 0.7 -> 0.07: the second carries T across 0.5
    "T_never_reaches_half": ([0.1, 0.1, 0.1], [1.0, 4.0, 2.0], 2, 3),                # T ends at 0.729: the last contributor
    "ends_early": ([0.99, 0.95, 0.95, 0.5, 0.5], [5.0, 5.5, 6.0, 7.0, 8.0], 0, 2),   # T: 1 -> 0.01 -> 5e-4, then 2.5e-5 < 1e-4 ends the ray
    "rejected_entries": ([0.2, 0.001, 0.4, 0.002, 0.6], [3.0, 9.0, 3.5, 9.0, 4.0], 2, 3),   # alpha < 1/255 takes no part; T: 1, 0.8, 0.48
}


@pytest.mark.parametrize("name", list(RAYS))
def test_forward_step_against_float64(name):
    alpha, m, sel, n = RAYS[name]
    got = dc.ray(alpha, m)
    D64, med64, sel64, w64, n64 = dc.ray64(alpha, m)
    D32 = dc.shifted32(w64, m)
    print(f"{name}: D {got['D']:.9e} (float64 {D64:.9e}, float32 recurrence {D32:.9e}), median {got['median']} at {got['med_pos']}, {got['n']} contributors")
    assert (sel64, n64) == (sel, n), "the float64 walk disagrees with the ray's description"
    assert got["n"] == n and got["med_pos"] == sel + 1
    assert got["median"] == np.float32(m[sel])          # a copy of the selected m
    assert np.abs(got["w"] - w64).max() <= 1e-6
    if D64 == 0.0:
        assert got["D"] == 0.0
    else:
        floor, err = abs(D32 - D64) / D64, abs(got["D"] - D64) / D64
        print(f"{name}: rel err {err:.3e} (float32 floor {floor:.3e})")
        assert err <= tolerance.rule3_bound(floor)


def test_a_pixel_without_contributors_is_zero():
    got = dc.ray([0.001, 0.002], [3.0, 4.0])
    assert (got["D"], got["median"], got["med_pos"], got["n"], got["T"]) == (0.0, 0.0, 0, 0, 1.0)


def test_step_state_is_the_documented_recurrence():
    """h_distortion_step on caller-held state against the independent float32 evaluation, bit for bit (the order of the operations is
    part of the contract)."""
    alpha, m = dc.slab_ray(30.0, 0)
    w = dc.ray(alpha, m)["w"]
    st, pos = np.zeros(6, np.float32), np.zeros(1, np.uint32)
    T = np.float32(1.0)
    for k in range(len(w)):
        dc.harness().h_distortion_step(float(w[k]), float(T), float(m[k]), k + 1, common.ptr(st), common.ptr(pos))
        T = np.float32(T * np.float32(np.float32(1.0) - alpha[k]))
    assert np.float32(st[3]) == np.float32(dc.shifted32(w, m)) and st[4] == m[0]


@pytest.mark.parametrize("depth", [30.0, 4.0])
def test_accuracy_on_thin_slabs(depth):
    """20 hits at depth +- 0.02, 200 seeds, per ray relative to the float64 value on the same float32 inputs.  The bound is rule 3 on the
    worst ray, the floor an independent float32 evaluation of the shifted recurrence.  The float32 composition A M2 - M1^2 is printed
    beside it; at depth 30 it must MISS the bound: that is the reason the kernel exists."""
    err = floor = comp = 0.0
    for seed in range(dc.SLAB_SEEDS):
        alpha, m = dc.slab_ray(depth, seed)
        got = dc.ray(alpha, m)
        D64, _med, _sel, w64, n = dc.ray64(alpha, m)
        assert n == dc.SLAB_HITS and got["n"] == n and D64 > 0
        err = max(err, abs(got["D"] - D64) / D64)
        floor = max(floor, abs(dc.shifted32(got["w"], m) - D64) / D64)
        comp = max(comp, abs(dc.composed32(got["w"], m) - D64) / D64)
    bound = tolerance.rule3_bound(floor)
    print(f"depth {depth} +- {dc.SLAB_HALF}: worst rel err of lg_distortion_step {err:.3e} (float32 recurrence {floor:.3e}, bound {bound:.3e}); "
          f"of the float32 composition A M2 - M1^2 {comp:.3e}")
    assert err <= bound
    if depth == 30.0:
        assert comp > bound, "the composed form is accurate here: the kernel would not be needed"


def _autograd(alpha, m, sel, gD, gM, dd):
    a = torch.tensor(np.asarray(alpha, np.float32)).to(dd).requires_grad_()
    mm = torch.tensor(np.asarray(m, np.float32)).to(dd).requires_grad_()
    keep = a.detach() >= 1.0 / 255.0
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=dd), torch.where(keep, 1 - a, torch.ones_like(a))[:-1]]), 0)
    w = torch.where(keep, a * T, torch.zeros_like(a))
    d = mm[:, None] - mm[None, :]
    D = (torch.triu(w[:, None] * w[None, :], 1) * d * d).sum()
    (gD * D + gM * mm[sel]).backward()
    return a.grad.numpy().astype(np.float64), mm.grad.numpy().astype(np.float64)


BWD_RAYS = {n: RAYS[n][:3] for n in ("two_hits_median_is_second", "T_never_reaches_half", "rejected_entries")}
BWD_RAYS.update({f"slab{int(d)}_{s}": dc.slab_ray(d, s) + (None,) for d in (30.0, 4.0) for s in (0, 1, 2)})
# a thick ray: depths spread over [2, 6], where D and its gradient are large
BWD_RAYS["spread"] = (np.random.RandomState(5).uniform(0.05, 0.4, 24).astype(np.float32), np.random.RandomState(6).uniform(2.0, 6.0, 24).astype(np.float32), None)


@pytest.mark.parametrize("gM", [-1.3, 0.0])
@pytest.mark.parametrize("name", list(BWD_RAYS))
def test_backward_step_against_float64_autograd(name, gM):
    """lg_distortion_bwd_step replayed back to front over a ray (every entry a contributor or rejected by alpha < 1/255: the ray does
    not end early, so the weights are smooth in the alphas) against float64 autograd of gD D + gM median, with respect to the alphas and
    the m; the float32 floor is the same autograd in float32."""
    alpha, m, sel = BWD_RAYS[name]
    gD = 0.7        # (gM = 0: d/dm is the distortion's alone, not dominated by the median's unit entry)
    got = dc.ray(alpha, m, gD, gM)
    _D, _med, sel64, _w, n64 = dc.ray64(alpha, m)
    assert got["n"] == n64 and got["med_pos"] == sel64 + 1 and (sel is None or sel == sel64)
    (a64, m64), (a32, m32) = _autograd(alpha, m, sel64, gD, gM, torch.float64), _autograd(alpha, m, sel64, gD, gM, torch.float32)
    tolerance.assert_rule3(got["dalpha"], a64, a32, f"{name} d/dalpha", ref="autograd")
    tolerance.assert_rule3(got["dm"], m64, m32, f"{name} d/dm", ref="autograd")


def test_header_matches_binding():
    declared = test_abi.check_extension_header("lightgaussian_distortion.h", distortion.PROTOTYPES)
    assert len(declared) == 4 and declared["lg_backward_distortion_scratch_bytes"] == ("size_t", ["int32", "int64", "int32"])
    text = open(os.path.join(ROOT, "include", "lightgaussian_distortion.h")).read()
    assert "#define LG_ABI_VERSION" not in text and '#include "lightgaussian.h"' in text
    make = open(os.path.join(ROOT, "lightgaussian_amd", "csrc", "Makefile")).read()
    assert "lg_distortion.h" in make and "lightgaussian_distortion.h" in make


def test_library_exports_the_prototypes():
    lib = distortion.load()
    assert all(hasattr(lib, name) for name in distortion.PROTOTYPES)
    assert lib.lg_abi_version() == 7
    # the two size queries run on the host: state = float4 + uint32 per pixel (each part padded), scratch grows with C and num_rendered
    assert lib.lg_distortion_state_bytes(33, 17) >= 33 * 17 * 20 and lib.lg_distortion_state_bytes(0, 17) == 0
    s0, s4 = lib.lg_backward_distortion_scratch_bytes(10, 1000, 0), lib.lg_backward_distortion_scratch_bytes(10, 1000, 4)
    assert s0 >= 1000 * 13 * 4 and s4 >= s0 + 1000 * 4 * 4 and lib.lg_backward_distortion_scratch_bytes(10, 1000, 65) == 0


def test_ndc_depth_is_the_published_mapping():
    z = torch.tensor([0.5, 1.0, 10.0, 100.0], dtype=torch.float64)
    near, far = 0.2, 1000.0
    want = far / (far - near) - far * near / ((far - near) * z)
    assert torch.equal(distortion.ndc_depth(z, near, far), want)
    assert abs(float(distortion.ndc_depth(torch.tensor(near), near, far))) < 1e-6 and abs(float(distortion.ndc_depth(torch.tensor(far), near, far)) - 1.0) < 1e-6
    with pytest.raises(ValueError):
        distortion.ndc_depth(z, 1.0, 0.5)
