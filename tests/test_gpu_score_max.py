"""-m gpu: score_reduce="max" (LG_FLAG_SCORE_MAX) -- important_score as the LARGEST per-hit weight of the view, for "alpha" / "alpha_t".

The reference is tests/cpu_harness/lg_scoremax_harness.cpp (tied to the oracle by tests/test_scoremax_host.py).  A maximum is exactly
associative and commutative and the value is one the blend computed, so everything here is demanded BIT-IDENTICAL: against the harness,
run to run, between the image-keeping variant (two global atomics into cleared slots) and the significance-only variant (merge in LDS,
one plain store per slot), across the exact and the capacity-bounded forward, on poisoned memory, and through the sharded pass for
every (streams, block)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import common
import gpu_common
import poison_common as pz
import scoremax_common as smc
from common import bits as _bits
from common import syn
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POLICIES = smc.POLICIES


def _count(kw, **options):
    from lightgaussian_amd import rasterizer
    with rasterizer.options(**options):
        return gpu_common.hip_forward_backward(kw, count=True)


def _assert_is_the_harness(out, ref, pol, what):
    assert np.array_equal(out["count"], ref["count"]), what
    bad = np.flatnonzero(_bits(out["score"]) != _bits(ref["max"][pol]))
    assert bad.size == 0, (f"{what}: {bad.size} scores differ from the harness, first: Gaussian {bad[0]} hip {out['score'][bad[0]]!r} "
                           f"harness {ref['max'][pol][bad[0]]!r} ({ref['count'][bad[0]]} hits)")


_IMAGES = {}


def _oracle_image(name, kw):
    if name not in _IMAGES:
        _IMAGES[name] = oracle.forward(count=True, **common.to_numpy(kw)).color
    return _IMAGES[name]


@pytest.mark.parametrize("pol", POLICIES)
@pytest.mark.parametrize("name", ["saturating", "early_stop", "ragged", "screen_filling", "partial_tile"])
def test_max_scores_are_bit_identical_to_the_harness(name, pol):
    """saturating / early_stop / ragged: tests/test_gpu_parity.py's CASES[1..3]; screen_filling: CASES[6], hundreds of slots per Gaussian
    (the whole-wave branch of lg_score_slots); partial_tile: 64 Gaussians on 13 x 9 pixels."""
    kw, ref = smc.scene(name)
    base = dict(weight_policy=pol, score_reduce="max")
    runs = {"image": _count(kw, **base), "image again": _count(kw, **base),
            "significance-only": _count(kw, skip_color_in_count=True, **base), "exact forward": _count(kw, sync_free=False, **base)}
    for what, out in runs.items():
        _assert_is_the_harness(out, ref, pol, f"{name} {pol} {what}")
    assert np.array_equal(_bits(runs["image"]["color"]), _bits(_oracle_image(name, kw)))       # the image does not depend on the reduction
    assert np.array_equal(_bits(runs["exact forward"]["color"]), _bits(_oracle_image(name, kw)))


@pytest.mark.parametrize("pol", POLICIES)
def test_empty_model_and_a_camera_that_sees_nothing(pol):
    kw, _ = smc.scene("partial_tile")
    N = kw["means3D"].shape[0]
    away = dict(kw, means3D=kw["means3D"] * 0 + torch.tensor([0.0, 0.0, -50.0]))              # everything behind the camera
    empty = {k: (v[:0] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == N else v) for k, v in kw.items()}
    for skip in (False, True):
        out = _count(away, weight_policy=pol, score_reduce="max", skip_color_in_count=skip)
        assert out["count"].shape == (N,) and not out["count"].any() and not _bits(out["score"]).any() and not out["radii"].any()
        out = _count(empty, weight_policy=pol, score_reduce="max", skip_color_in_count=skip)
        assert out["count"].shape == (0,) and out["score"].shape == (0,)


@pytest.mark.parametrize("pol", POLICIES)
def test_long_lists_with_every_chunk_fill_level(pol):
    """6000 Gaussians at 208 x 144: lists of several hundred entries, saturating piles, batches of 64 with every fill level of the 8-row
    chunks; with the default segment length and with segments of 64 entries (the image-keeping variant then writes checkpoints)."""
    kw, ref = smc.scene("long_lists")
    assert ref["instances"] / ((208 // 16) * (144 // 16)) > 300
    for extra in ({}, {"segment_length": 64}, {"segment_length": 64, "skip_color_in_count": True}, {"skip_color_in_count": True}):
        _assert_is_the_harness(_count(kw, weight_policy=pol, score_reduce="max", **extra), ref, pol, f"long lists {pol} {extra}")


@pytest.mark.parametrize("pol", POLICIES)
def test_antialiasing_maximises_the_compensated_alpha(pol):
    kw, ref = smc.scene("saturating", antialias=True)
    _, plain = smc.scene("saturating")
    assert not np.array_equal(ref["max"][pol], plain["max"][pol])
    for skip in (False, True):
        out = _count(kw, weight_policy=pol, score_reduce="max", antialiasing=True, skip_color_in_count=skip)
        _assert_is_the_harness(out, ref, pol, f"antialiasing {pol} skip_color={skip}")


def test_images_beyond_2_pow_24_pixels_are_not_refused_for_the_maximum():
    """The limit belongs to the Q24.40 sums (tests/test_gpu_weight_policies.py pins their refusal); a maximum cannot overflow."""
    g = syn.make_gaussians(50, seed=3, log_scale_mean=math.log(0.05))
    W, H = 4112, 4096
    kw = common.scene_kwargs(g, syn.orbit_camera(0, 4, W, H), W, H, deg=3, as_torch=True)
    ref = smc.score_max(kw)
    assert ref["count"].sum() > 0
    _assert_is_the_harness(_count(kw, weight_policy="alpha_t", score_reduce="max", skip_color_in_count=True), ref, "alpha_t", "16.8 M pixels")


@pytest.mark.parametrize("skip_color", [False, True])
@pytest.mark.parametrize("pol", POLICIES)
def test_the_four_variants_do_not_depend_on_what_memory_held(pol, skip_color):
    """As tests/test_gpu_memory_independence.py::test_count_render: the merging variant stores every slot once without a clear, the
    image-keeping one adds into slots a clear must have zeroed -- on the exact forward and on the bounded one."""
    from lightgaussian_amd import rasterizer
    kw, ref = smc.scene("saturating")
    keys = ("count", "score", "radii") + (() if skip_color else ("color",))

    def run():
        rasterizer._CAPACITY.clear()
        out = {}
        for which in ("exact", "bounded"):           # the first forward of a shape learns the capacity, the second is bounded by it
            o = _count(kw, weight_policy=pol, score_reduce="max", skip_color_in_count=skip_color, sync_free="validated")
            out[which] = {k: o[k] for k in keys}
        return out

    runs = pz.run_all(run)
    pz.assert_identical(runs, f"max {pol} skip_color={skip_color}")
    for which, o in runs[0][1].items():
        _assert_is_the_harness(o, ref, pol, which)


def test_score_out_and_count_sum_under_max_equal_the_plain_outputs():
    from lightgaussian_amd.gaussian_renderer import count_render
    g, cams = smc.shard_scene()
    N = smc.SHARD_N
    pc, cams = g.to(DEV), [c.to(DEV) for c in cams[:3]]
    bg, pipe = torch.zeros(3, device=DEV), syn.PipelineParams()
    opts = {"weight_policy": "alpha_t", "score_reduce": "max", "skip_color_in_count": True}
    rows = torch.full((3, N + 7), -1.0, device=DEV)
    running = torch.zeros(N, dtype=torch.int32, device=DEV)
    plain_cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for k, cam in enumerate(cams):
            ref = count_render(cam, pc, pipe, bg, options=opts)
            plain_cnt += ref["gaussians_count"]
            out = count_render(cam, pc, pipe, bg, options=dict(opts, score_out=rows[k, :N], count_sum=running))
            assert out["important_score"].data_ptr() == rows[k].data_ptr()
            assert torch.equal(out["gaussians_count"], ref["gaussians_count"])
            assert torch.equal(rows[k, :N].view(torch.int32), ref["important_score"].view(torch.int32))
            assert float(ref["important_score"].max()) <= 0.99 and int(ref["gaussians_count"].sum()) > 0
    assert torch.equal(running, plain_cnt) and bool((rows[:, N:] == -1.0).all())


@pytest.mark.parametrize("pol", POLICIES)
def test_sharded_pass_is_the_maximum_over_the_harness_views_and_prune_below_keeps_the_cpu_mask(pol):
    """The 9-view scene of the per-hit sum test, 4 views in flight / the plain loop / 3 streams with blocks of 4: scores bit-identical to
    the maximum over the harness's per-view scores, counts their sum; prune_below on a model with Adam state against plain indexing."""
    from lightgaussian_amd import prune as lg_prune
    from test_gpu_compact import _Model, _state
    from test_gpu_full_size import _activated_on_device, _oracle_kw
    g, cams = smc.shard_scene()
    N, W, H = smc.SHARD_N, smc.SHARD_W, smc.SHARD_H
    pc = g.to(DEV)
    act = _activated_on_device(pc)      # the harness is fed what the kernels see: the getters evaluated by torch ON THE DEVICE
    views = [smc.score_max(_oracle_kw(act, cam, W, H, 3, np.zeros(3))) for cam in cams]
    cnt_ref = np.sum([v["count"] for v in views], axis=0)
    max_ref = np.max([v["max"][pol] for v in views], axis=0)
    dcams, bg = [c.to(DEV) for c in cams], torch.zeros(3, device=DEV)
    with torch.no_grad():
        for streams, block in ((4, 24), (1, 2), (3, 4)):
            cnt, imp = lg_prune.prune_list_sharded(pc, dcams, syn.PipelineParams(), bg, weight_policy=pol, score_reduce="max", streams=streams, block=block)
            assert np.array_equal(cnt.cpu().numpy(), cnt_ref), (streams, block)
            assert np.array_equal(_bits(imp), _bits(max_ref)), (streams, block)
    for thr in (smc.THRESHOLD, 0.25):
        want = torch.from_numpy(max_ref < np.float32(thr))
        assert 0 < int(want.sum()) < N or (pol, thr) == ("alpha", smc.THRESHOLD)    # (every Gaussian of this scene has alpha >= 0.01 somewhere)
        a, b = _Model(N, 5), _Model(N, 5)
        a.reference_prune_points(want.to(DEV))
        mask = lg_prune.prune_below(b, imp, thr)
        assert torch.equal(mask.cpu(), want)
        sa, sb = _state(a), _state(b)
        assert sa.keys() == sb.keys() and sb["_xyz"].shape[0] == N - int(want.sum())
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (thr, k)


def test_explicit_sum_gives_the_bits_of_no_option_at_all():
    kw, ref = smc.scene("early_stop")
    for pol in POLICIES:
        for skip in (False, True):
            a = _count(kw, weight_policy=pol, skip_color_in_count=skip)
            b = _count(kw, weight_policy=pol, skip_color_in_count=skip, score_reduce="sum")
            assert np.array_equal(a["count"], b["count"]) and np.array_equal(_bits(a["score"]), _bits(b["score"]))
            assert np.array_equal(_bits(b["score"]), _bits(ref["score_sum"][pol])) and np.array_equal(b["count"], ref["count"])


def test_refusals():
    """Python: "max" over an equal-addend policy raises before any native call.  C ABI: the flag with LG_WEIGHT_ONE / _OPACITY, or together
    with LG_FLAG_FAST_EXP, in a count forward is LG_ERR_INVALID_ARGUMENT before the first HIP call (the allocator callback is never
    called, the outputs keep their fill); a colour forward ignores the flag."""
    from lightgaussian_amd import _lib, rasterizer
    from lightgaussian_amd.rasterizer import GaussianRasterizationSettings
    kw, ref = smc.scene("partial_tile")
    for pol in ("one", "opacity"):
        with pytest.raises(ValueError, match="alpha"):
            _count(kw, weight_policy=pol, score_reduce="max")
    plain = gpu_common.hip_forward_backward(kw)
    with rasterizer.options(score_reduce="max", weight_policy="opacity"):      # render() ignores the option, as it ignores the policy
        assert np.array_equal(_bits(gpu_common.hip_forward_backward(kw)["color"]), _bits(plain["color"]))

    lib = _lib.load()
    t = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
    N, W, H = t["means3D"].shape[0], t["W"], t["H"]
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=t["tanfovx"], tanfovy=t["tanfovy"], bg=t["bg"], scale_modifier=1.0,
                                       viewmatrix=t["viewmatrix"], projmatrix=t["projmatrix"], sh_degree=t["sh_degree"], campos=t["campos"],
                                       prefiltered=False, debug=False, f_count=True)
    opts = rasterizer.resolve_options({"weight_policy": "alpha_t", "score_reduce": "max", "sync_free": False})
    call = rasterizer._Call(rs, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, exact=True, opts=opts)
    assert call.view.flags & rasterizer.FLAG_SCORE_MAX and not call.view.flags & _lib.FLAG_FAST_EXP
    u8 = dict(dtype=torch.uint8, device=DEV)
    geom, img = torch.empty(lib.lg_geom_bytes(N), **u8), torch.empty(lib.lg_img_bytes(W, H), **u8)
    color = torch.empty((3, H, W), device=DEV)
    radii = torch.empty(N, dtype=torch.int32, device=DEV)
    allocations = []

    def _alloc(_user, nbytes):
        allocations.append(_lib.scratch(nbytes, torch.device(DEV)))
        return allocations[-1].data_ptr()

    cb = _lib.ALLOC_FN(_alloc)

    def forward_count(flags, policy):
        call.view.flags = flags
        gcount = torch.full((N,), -7, dtype=torch.int32, device=DEV)
        score = torch.full((N,), -7.0, device=DEV)
        bin_ptr, R = C.c_void_p(), C.c_int64(0)
        rc = lib.lg_forward_count(C.byref(call.view), C.byref(call.g), _lib.ptr(geom), _lib.ptr(img), cb, None, policy, _lib.ptr(color),
                                  _lib.ptr(radii), _lib.ptr(gcount), _lib.ptr(score), C.byref(bin_ptr), C.byref(R), _lib.stream())
        torch.cuda.synchronize()
        return rc, gcount.cpu().numpy(), score.cpu().numpy()

    good = call.view.flags
    for flags, policy in ((good | _lib.FLAG_FAST_EXP, _lib.WEIGHT_ALPHA_T), (good | _lib.FLAG_FAST_EXP, _lib.WEIGHT_ALPHA),
                          (good, _lib.WEIGHT_ONE), (good, _lib.WEIGHT_OPACITY)):
        rc, gcount, score = forward_count(flags, policy)
        assert rc == _lib.LG_ERR_INVALID_ARGUMENT and not allocations, (hex(flags), policy)
        assert (gcount == -7).all() and (score == -7.0).all()                          # nothing ran
    rc, gcount, score = forward_count(good, _lib.WEIGHT_ALPHA_T)                        # the same raw call, accepted
    assert rc == _lib.LG_OK and len(allocations) == 1
    assert np.array_equal(gcount, ref["count"]) and np.array_equal(_bits(score), _bits(ref["max"]["alpha_t"]))
