"""score_reduce="max" without a GPU: the reference harness (tests/cpu_harness/lg_scoremax_harness.cpp) tied to the oracle, the plan bit,
the option's validation in the rasterizer and in run.py, the max fold of prune_list / prune_list_sharded (single process and gloo at
world size 2 and 3, with the harness standing in for count_render) and the threshold mask.

The oracle has no maximum.  What ties the harness's maxima to it: over the same walk the harness also adds the Q24.40 quanta of the
very per-hit values it maximises, and those sums must be the oracle's W_ALPHA / W_ALPHA_T scores bit for bit, with the oracle's hit
counts -- so the per-hit values are the oracle's."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import common
import scoremax_common as smc
from common import syn
from lightgaussian_amd import prune as lg_prune
from oracle import oracle
from test_forward_plan import ALPHA, ALPHA_T, FIELDS, _cases, forward_plan

ORACLE_POLICY = {"alpha": oracle.W_ALPHA, "alpha_t": oracle.W_ALPHA_T}
SCORE_MAX, SCORE_SLOTS_MAX = 65536, 4
SCENES = sorted(smc.SCENES)


def _np(kw):
    return common.to_numpy(kw)


@pytest.mark.parametrize("name", SCENES)
def test_harness_is_tied_to_the_oracle_and_the_maximum_lies_between_mean_and_sum(name):
    kw, ref = smc.scene(name)
    for pol in smc.POLICIES:
        o = oracle.forward(count=True, weight_policy=ORACLE_POLICY[pol], **_np(kw))
        assert np.array_equal(ref["count"], o.count), pol
        assert np.array_equal(common.bits(ref["score_sum"][pol]), common.bits(o.score)), pol
        cnt, mx = ref["count"].astype(np.float64), ref["max"][pol]
        hit = ref["count"] > 0
        assert hit.any() and (~hit).any()
        # without hits both reductions are 0; with hits the maximum is one hit's weight: alpha >= 1/255, T >= 1e-4
        assert np.all(mx[~hit] == 0) and np.all(ref["sum"][pol][~hit] == 0) and np.all(mx[hit] > 0)
        # mean <= max <= min(sum, 0.99), the sum being known to its own quantisation (count x 2^-41) plus one fp32 ulp of the maximum
        total = ref["sum"][pol].astype(np.float64) * 2.0 ** -40            # exact: the integers are below 2^53
        tol = cnt * 2.0 ** -41 + np.spacing(mx).astype(np.float64)
        m64 = mx.astype(np.float64)
        assert np.all(total[hit] / cnt[hit] - tol[hit] <= m64[hit]), pol
        assert np.all(m64[hit] <= total[hit] + tol[hit]) and np.all(mx[hit] <= np.float32(0.99)), pol
        # Gaussians on both sides of the pruning threshold, among those that were hit: a threshold prune removes some and keeps some
        assert (mx[hit] < smc.THRESHOLD).any() and (mx >= smc.THRESHOLD).any(), (name, pol)
    # alpha T <= alpha hit by hit, hence for the maxima
    assert np.all(ref["max"]["alpha_t"] <= ref["max"]["alpha"])


def test_antialias_switch_changes_the_maxima_and_stays_tied_to_the_sums():
    kw, plain = smc.scene("saturating")
    _, aa = smc.scene("saturating", antialias=True)
    assert not np.array_equal(plain["max"]["alpha_t"], aa["max"]["alpha_t"]) and not np.array_equal(plain["count"], aa["count"])
    hit = aa["count"] > 0
    assert np.all(aa["max"]["alpha"][hit] > 0) and np.all(aa["max"]["alpha"][~hit] == 0)
    # the oracle on opacities compensated by the product's own rho (as tests/test_gpu_antialias.py builds its reference)
    import antialias_common
    k = _np(kw)
    k["opacities"] = (k["opacities"].reshape(-1) * antialias_common.rho32_harness(kw)).astype(np.float32)[:, None]
    for pol in smc.POLICIES:
        o = oracle.forward(count=True, weight_policy=ORACLE_POLICY[pol], **k)
        assert np.array_equal(aa["count"], o.count) and np.array_equal(common.bits(aa["score_sum"][pol]), common.bits(o.score)), pol


def test_plan_bit_selects_the_max_score_kernel_and_nothing_else():
    n = 0
    for count, fast, skip, serial, parallel, policy, flags in _cases():
        for N, cap in ((1000, 5000), (1000, 0), (0, 5000)):
            base, got = forward_plan(flags, count, policy, N, cap), forward_plan(flags | SCORE_MAX, count, policy, N, cap)
            per_hit = count and policy in (ALPHA, ALPHA_T)
            assert (got["score"] == SCORE_SLOTS_MAX) == bool(per_hit and N > 0), (count, hex(flags), policy, N, cap)
            for f in FIELDS:
                if f != "score" or got["score"] != SCORE_SLOTS_MAX:
                    assert got[f] == base[f], (f, count, hex(flags), policy, N, cap)
            if not count:       # a colour forward ignores the flag, as it ignores the policy
                assert got == base
            n += got["score"] == SCORE_SLOTS_MAX
    assert n == 2 * 2 * 16      # two policies, (N, cap) with N > 0, the 16 combinations of the four other flags


def test_extension_header_declares_the_flag_on_a_bit_the_frozen_header_leaves_free(monkeypatch):
    """include/lightgaussian_score.h holds LG_FLAG_SCORE_MAX and nothing else; lightgaussian.h, its 36 constants and the ABI version are as
    they were, and none of its flags has the bit."""
    import test_abi
    from lightgaussian_amd import _lib, rasterizer
    frozen = test_abi._header_constants()
    assert "LG_FLAG_SCORE_MAX" not in frozen and frozen["LG_ABI_VERSION"] == 7 == _lib.ABI_VERSION
    assert not any(v & SCORE_MAX for n, v in frozen.items() if n.startswith("LG_FLAG_")) and SCORE_MAX != 4096
    monkeypatch.setattr(test_abi, "HDR", os.path.join(common.ROOT, "include", "lightgaussian_score.h"))
    monkeypatch.setattr(test_abi, "HDR_DEBUG", os.devnull)
    assert test_abi._header_constants() == {"LG_FLAG_SCORE_MAX": SCORE_MAX} == {"LG_FLAG_SCORE_MAX": rasterizer.FLAG_SCORE_MAX}
    assert test_abi._header_prototypes() == {} and test_abi._header_structs() == {}      # no new entry point, no struct


def test_option_is_validated_and_refuses_equal_addend_policies_before_any_native_call(monkeypatch):
    from lightgaussian_amd import _lib, rasterizer
    assert rasterizer.resolve_options()["score_reduce"] == "sum"
    for bad in ("maximum", "", None, 1, True):
        with pytest.raises(ValueError):
            rasterizer.options(score_reduce=bad)
        with pytest.raises(ValueError):
            rasterizer.set_option("score_reduce", bad)
    assert rasterizer.resolve_options()["score_reduce"] == "sum"
    with rasterizer.options(score_reduce="max"):
        assert rasterizer.resolve_options()["score_reduce"] == "max"
    for pol in ("alpha", "alpha_t", _lib.WEIGHT_ALPHA_T):
        assert rasterizer.check_score_reduce("max", pol) == "max" and rasterizer.check_score_reduce("sum", pol) == "sum"
    for pol in ("one", "opacity", _lib.WEIGHT_ONE):
        assert rasterizer.check_score_reduce("sum", pol) == "sum"
        with pytest.raises(ValueError, match="alpha"):
            rasterizer.check_score_reduce("max", pol)
    # the sharded pass refuses before it renders anything: neither the library nor count_fn is reached
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("native library loaded"))
    g, cams = smc.shard_scene()
    fail = lambda *a, **k: pytest.fail("count_fn called")  # noqa: E731
    for pol in ("opacity", "one", None):
        with pytest.raises(ValueError, match="alpha"):
            lg_prune.prune_list_sharded(g, cams, syn.PipelineParams(), torch.zeros(3), count_fn=fail, weight_policy=pol, score_reduce="max")
    with pytest.raises(ValueError):
        lg_prune.prune_list_sharded(g, cams, syn.PipelineParams(), torch.zeros(3), count_fn=fail, weight_policy="alpha_t", score_reduce="most")


def test_runner_refuses_a_bad_score_reduce_before_the_script_runs(tmp_path):
    script = tmp_path / "trainer.py"
    script.write_text("import json\nfrom lightgaussian_amd import rasterizer\nprint(json.dumps({'ran': rasterizer.resolve_options()['score_reduce']}))\n")
    run = lambda *flags: subprocess.run([sys.executable, "-m", "lightgaussian_amd.run", "--no-patch", *flags, str(script)],  # noqa: E731
                                        capture_output=True, text=True, cwd=common.ROOT)
    ok = run("--weight-policy=alpha_t", "--score-reduce=max")
    assert ok.returncode == 0 and '"ran": "max"' in ok.stdout, ok.stderr[-2000:]
    ok = run("--score-reduce=max", "--weight-policy=alpha")         # the order of the two does not matter
    assert ok.returncode == 0 and '"ran": "max"' in ok.stdout, ok.stderr[-2000:]
    ok = run("--score-reduce=sum")
    assert ok.returncode == 0 and '"ran": "sum"' in ok.stdout, ok.stderr[-2000:]
    for flags in (("--score-reduce=maximum",), ("--score-reduce=max",), ("--score-reduce=max", "--weight-policy=opacity"),
                  ("--weight-policy=one", "--score-reduce=max")):
        bad = run(*flags)
        assert bad.returncode != 0 and "score-reduce" in bad.stderr and '"ran"' not in bad.stdout, flags


# ---- the fold over views: prune_list, prune_list_sharded ------------------------------------------------------------------------------
_VIEWS = {}


def _views():
    """Per-view harness results of the 9-view scene, once per process."""
    if not _VIEWS:
        g, cams = smc.shard_scene()
        _VIEWS["g"], _VIEWS["cams"] = g, cams
        _VIEWS["ref"] = [smc.score_max(common.scene_kwargs(g, cam, smc.SHARD_W, smc.SHARD_H, as_torch=True)) for cam in cams]
    return _VIEWS


def _count_fn(pol):
    v = _views()

    def fn(cam, pc, pipe, bg):
        from lightgaussian_amd import rasterizer
        assert rasterizer.resolve_options()["score_reduce"] == "max"        # the pass hands the option to its forwards
        r = v["ref"][[id(c) for c in v["cams"]].index(id(cam))]
        return {"gaussians_count": torch.from_numpy(r["count"].copy()), "important_score": torch.from_numpy(r["max"][pol].copy())}
    return fn


def _expected(pol):
    v = _views()
    return np.sum([r["count"] for r in v["ref"]], axis=0), np.max([r["max"][pol] for r in v["ref"]], axis=0)


@pytest.mark.parametrize("pol", smc.POLICIES)
def test_single_process_folds_views_with_a_maximum_and_adds_counts(pol):
    from lightgaussian_amd import rasterizer
    v = _views()
    cnt_ref, max_ref = _expected(pol)
    pipe, bg = syn.PipelineParams(), torch.zeros(3)
    with rasterizer.options(weight_policy=pol):
        cnt, imp = lg_prune.prune_list(v["g"], v["cams"], pipe, bg, count_fn=_count_fn(pol), score_reduce="max")
        with rasterizer.options(score_reduce="max"):            # None = the option in force
            cnt2, imp2 = lg_prune.prune_list(v["g"], v["cams"], pipe, bg, count_fn=_count_fn(pol))
    for c, s in ((cnt, imp), (cnt2, imp2)):
        assert np.array_equal(c.numpy(), cnt_ref) and np.array_equal(common.bits(s), common.bits(max_ref))
    for block in (1, 2, 4, 9, 24):
        cnt, imp = lg_prune.prune_list_sharded(v["g"], v["cams"], pipe, bg, count_fn=_count_fn(pol), block=block, weight_policy=pol, score_reduce="max")
        assert np.array_equal(cnt.numpy(), cnt_ref), block
        assert np.array_equal(common.bits(imp), common.bits(max_ref)), block
    # RadSplat's two thresholds.  (On this scene every Gaussian has alpha >= 0.01 somewhere: 0.01 splits the alpha_t scores only.)
    for thr in (smc.THRESHOLD, 0.25):
        mask = lg_prune.prune_mask_threshold(imp, thr)
        assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), max_ref < np.float32(thr))
        assert 0 < int(mask.sum()) < mask.numel() or (pol, thr) == ("alpha", smc.THRESHOLD)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, mode, block, pol, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        v = _views()
        stats = {}
        cnt, imp = lg_prune.prune_list_sharded(v["g"], v["cams"], syn.PipelineParams(), torch.zeros(3), mode=mode, count_fn=_count_fn(pol), block=block,
                                               weight_policy=pol, score_reduce="max", stats=stats)
        mask = lg_prune.prune_mask_threshold(imp, smc.THRESHOLD)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), cnt=cnt.numpy(), imp=imp.numpy(), mask=mask.numpy(), collectives=stats["collectives"])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,mode,block,pol", [(2, "ordered", 24, "alpha_t"), (3, "ordered", 2, "alpha_t"), (2, "allreduce", 1, "alpha"),
                                                 (3, "ordered", 4, "alpha")])
def test_sharded_max_is_bit_identical_on_every_rank_for_every_world_size(world, mode, block, pol, tmp_path):
    """block 2 at world 3: rounds of 6 views with a ragged last round; 24: one round in which ranks own 5 / 4 views.  Whatever `mode` says
    the exchange is one all_reduce(MAX) for the scores and one all_reduce(SUM) for the counts."""
    cnt_ref, max_ref = _expected(pol)
    mp.spawn(_worker, args=(world, _free_port(), mode, block, pol, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        o = np.load(tmp_path / f"r{r}.npz")
        assert np.array_equal(o["cnt"], cnt_ref)
        assert np.array_equal(o["imp"].view(np.uint32), max_ref.view(np.uint32))
        assert np.array_equal(o["mask"], max_ref < np.float32(smc.THRESHOLD))
        assert int(o["collectives"]) == 2


def test_threshold_mask_and_prune_below(monkeypatch):
    score = torch.tensor([0.0, 0.0099999, 0.01, 0.25, 0.5, 0.009])
    assert lg_prune.prune_mask_threshold(score, 0.01).tolist() == [True, True, False, False, False, True]      # strictly below goes; ties stay
    assert lg_prune.prune_mask_threshold(score.reshape(-1, 1), 0.25).tolist() == [True, True, True, False, False, True]
    # prune_below hands exactly that mask to prune_points (whose compaction needs the device: tests/test_gpu_score_max.py runs it on a
    # model with Adam state against plain indexing)
    seen = {}
    monkeypatch.setattr(lg_prune, "prune_points", lambda model, mask: seen.update(model=model, mask=mask.clone()))
    model = object()
    out = lg_prune.prune_below(model, score.reshape(-1, 1), 0.01)
    assert seen["model"] is model and torch.equal(seen["mask"], score < 0.01) and torch.equal(out, seen["mask"])
