"""-m gpu: no output may depend on what allocated memory held before the call.

Every output tensor and every scratch buffer of the library comes from torch.empty (torch.empty_like, Tensor.new_empty, _lib.scratch),
so the design rests on one invariant: every byte that is read, on the device or by the caller, was written by
this call first.  Fresh device pages are zero and the caching allocator hands a test the block its previous, identical call freed, so
a kernel that skips a row, or reads a word it never cleared, passes every other test.  Here each entry point runs once as it is and
once under each pattern of tests/poison_common.py (ZERO first, then the payload NaN, then 1.0f), with guard words around every
allocation, and EVERY tensor the caller can see must be bit-identical across the four runs; one comparison with the path's existing
oracle keeps four identically wrong results from passing.  Internal saved buffers (geom, binning, img) are not compared: their padding
is legitimately unspecified.

The one user-visible region that is documented as unspecified: the `render` image of a count render with skip_color_in_count
("the returned `render` tensor is uninitialised memory", rasterizer.set_option) -- it is left out of those comparisons and nowhere else.

The view: the 2000-Gaussian, 161 x 83 scene of camera_common under its `inside` camera (N no multiple of 64, a ragged image,
Gaussians between the camera plane and the near plane and behind the camera, radii of hundreds of pixels) with appended, in view
space: splats whose opacity lies below 1/255 (radii > 0, no instance emitted), a pile of opaque splats on one tile (a list of more than
three 64-entry segments, saturating pixels).  Every tile of that view is covered by at least nine screen-filling splats, so no
appended Gaussian can make a tile's list empty there: the empty tiles come from a second camera on the same model, far outside it
(`far`), and the training render runs under both.  preconditions() asserts all of it from the CPU oracle before any GPU call."""
import functools
import math

import numpy as np
import pytest
import torch

import camera_common
import common
import gpu_common
import poison_common as pz
from common import syn
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = camera_common.W, camera_common.H
BG = camera_common.BG
PILE, FAINT = 200, 6
PILE_PIXEL = (88.0, 40.0)            # inside tile (5, 2): x 80 .. 95, y 32 .. 47


def _view_xy(cam, px, py, z):
    """View-space (x, y) of the point that lands on pixel centre (px, py) at depth z."""
    ndcx, ndcy = (2.0 * px + 1.0) / W - 1.0, (2.0 * py + 1.0) / H - 1.0
    return ndcx * math.tan(cam.FoVx * 0.5) * z, ndcy * math.tan(cam.FoVy * 0.5) * z


@functools.lru_cache(maxsize=None)
def model():
    """(the Gaussians, {name: camera}): camera_common's scene + the appended populations."""
    cam = camera_common.camera("inside")
    rng = np.random.default_rng(12)
    extra = []
    for k in range(FAINT):                                         # sigmoid(-7) = 9.1e-4 < 1/255: visible, but no instance
        x, y = _view_xy(cam, 20.0 + 24.0 * k, 12.0 + 11.0 * k, 1.5)
        extra.append(((x, y, 1.5), (math.log(0.05),) * 3, -7.0))
    for k in range(PILE):                                          # sigmoid(3) = 0.95, ~30 px radius: each covers the pile's tile
        z = 1.0 + 2.0 * k / PILE
        x, y = _view_xy(cam, PILE_PIXEL[0] + rng.uniform(-3, 3), PILE_PIXEL[1] + rng.uniform(-3, 3), z)
        extra.append(((x, y, z), (math.log(0.07 * z),) * 3, 3.0))
    g = common.append_view_space(camera_common.gaussians(), cam, extra)
    far = syn.look_at_camera((9.0, -6.0, -10.0), (0.0, 0.0, 0.0), W, H, roll_deg=15.0, fovx_deg=60.0)
    return g, {"inside": cam, "far": far}


@functools.lru_cache(maxsize=None)
def view(name, deg=3):
    """The rasterizer kwargs of `name` (numpy), the oracle's count forward and the CPU build of the kernels' traversal."""
    g, cams = model()
    kw = common.scene_kwargs(g, cams[name], W, H, deg=deg, bg=BG)
    return dict(kw=kw, ref=oracle.forward(count=True, **kw), twin=common.harness_forward(kw, cull=True))


def _tile_cover(twin, vis):
    """Upper bound of every tile's list: the tight rectangles are all the kernels can emit."""
    cover = np.zeros(((H + 15) // 16, (W + 15) // 16), np.int64)
    for x0, y0, x1, y1 in twin["tight_rect"][vis]:
        cover[y0:y1, x0:x1] += 1
    return cover


@functools.lru_cache(maxsize=None)
def preconditions():
    """Conditions a-e on the inputs, from the CPU oracle; returns the row masks the tests use."""
    v, far = view("inside"), view("far")
    kw, ref, twin = v["kw"], v["ref"], v["twin"]
    N = kw["means3D"].shape[0]
    assert N == camera_common.CAMERA_SCENE["N"] + FAINT + PILE and N % 64 != 0 and W % 16 != 0 and H % 16 != 0
    vis = ref.radii > 0
    assert np.array_equal(twin["radii"], ref.radii)
    vm = np.asarray(kw["viewmatrix"], np.float32).reshape(4, 4)
    z = np.asarray(kw["means3D"], np.float32) @ vm[:3, 2] + vm[3, 2]
    # a. radii == 0 for each reason the kernels know.  Here, as in the reference, the lateral frustum cull IS the empty reference rectangle
    # (a centre so far off the image that its rectangle clamps to nothing); the product's own empty rectangle is the TIGHT one of a visible
    # Gaussian whose footprint reaches no pixel of any tile (population b's, and the conservative footprint cull's)
    near = (z > 0) & (z <= np.float32(0.2))
    behind = z <= 0
    lateral = (z > np.float32(0.2)) & ~vis
    tight_area = (twin["tight_rect"][:, 2] - twin["tight_rect"][:, 0]) * (twin["tight_rect"][:, 3] - twin["tight_rect"][:, 1])
    assert near.sum() >= 50 and behind.sum() >= 500 and not vis[near | behind].any()
    assert lateral.sum() >= 100
    assert (vis & (tight_area == 0)).sum() >= FAINT
    # b. visible, opacity below 1/255: never counted, no instance
    faint = vis & (np.asarray(kw["opacities"]).reshape(-1) < np.float32(1.0 / 255.0))
    assert faint.sum() == FAINT and not ref.count[faint].any() and not tight_area[faint].any()
    # c. an empty tile list: under `far`, a tile no tight rectangle reaches
    far_cover = _tile_cover(far["twin"], far["ref"].radii > 0)
    assert (far_cover == 0).sum() >= 4 and (far_cover > 0).sum() >= 4 and far["ref"].count.sum() > 1000
    assert _tile_cover(twin, vis).min() >= 1             # ... and why it cannot be had under `inside`
    # d. a list of at least 3 segments of 64: Gaussians whose centre lies inside the tile are on its list whatever the footprint cull does
    xy = ref.saved["xy"]
    solid = vis & (tight_area > 0)
    in_tile = solid & (xy[:, 0] >= 80) & (xy[:, 0] < 96) & (xy[:, 1] >= 32) & (xy[:, 1] < 48)
    assert in_tile.sum() >= 3 * 64 + 1, int(in_tile.sum())
    # e. a pixel that saturates: the walk stops where T (1 - alpha) would fall below 1e-4, so the pile's pixel ends with T in [1e-4, 1e-2)
    # and never reaches the deepest half of the pile (each of which covers it with alpha ~ 0.9) -- recolouring that half changes nothing there
    px, py = int(PILE_PIXEL[0]), int(PILE_PIXEL[1])
    assert ref.saved["final_T"].reshape(H, W)[py, px] < 1e-3
    recoloured = dict(kw, shs=kw["shs"].copy())
    recoloured["shs"][N - PILE // 2:, 0, :] += 2.0
    other = oracle.forward(**recoloured).color
    assert np.array_equal(common.bits(other[:, py, px]), common.bits(ref.color[:, py, px])) and not np.array_equal(common.bits(other), common.bits(ref.color))
    assert (ref.saved["final_T"] < 1e-3).sum() >= 16
    assert ref.count.sum() > 10000 and twin["num_instances"] > 2000
    return dict(N=N, culled=torch.from_numpy(~vis), faint=torch.from_numpy(faint), no_gradient=torch.from_numpy(~vis | faint))


def test_the_view_holds_every_population():
    facts = preconditions()
    assert int(facts["culled"].sum()) > 1500 and int(facts["faint"].sum()) == FAINT


def test_the_poison_reaches_the_buffers_the_kernels_write():
    """The tests below prove something only if the library's allocations really come back dirty.  The one output that is DOCUMENTED as
    uninitialised memory shows it: the `render` tensor of a count render with skip_color_in_count holds the pattern in every word (the
    kernels never touch it), and a render + backward allocates its outputs, its saved buffers, its scratch and its gradient buffers --
    the nine slots of _GradSet among them -- through the patched names."""
    from lightgaussian_amd.gaussian_renderer import render, count_render
    preconditions()
    cam = model()[1]["inside"].to(DEV)
    bg, pipe = torch.tensor(BG, device=DEV), syn.PipelineParams()
    for name, word in pz.PATTERNS:
        with pz.poisoned(word) as p:
            with torch.no_grad():
                img = count_render(cam, _frozen(), pipe, bg, options={"skip_color_in_count": True, "sync_free": False})["render"]
            forward_only = len(p.allocations)
            pc = _leaf_model()
            render(cam, pc, pipe, bg, options={"sync_free": False})["render"].sum().backward()
            torch.cuda.synchronize()
            sizes = [nbytes for _raw, nbytes in p.allocations[forward_only:]]
        assert bool((img.view(torch.int32) == int(np.uint32(word).view(np.int32))).all()), name
        N = pc._xyz.shape[0]
        assert forward_only >= 7                                               # geom, img, color, radii, count, score, binning
        for rows in (3, 3, 3, 45, 1, 3, 4):                                    # means2D, means3D, dc, rest, opacity, scales, rotations
            assert 4 * N * rows in sizes, (name, rows)
        assert 3 * H * W * 4 in sizes and 4 * N in sizes                       # the image, the radii


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _gimg(seed=3):
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed))


def _leaf_model(deg=3):
    g, _ = model()
    pc = syn.SyntheticGaussians(*[t.detach().clone().to(DEV).requires_grad_(True) for t in
                                  (g._xyz, g._features_dc, g._features_rest, g._scaling, g._rotation, g._opacity)], deg, g.max_sh_degree)
    return pc


RAW = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


def _raw_grads(pc):
    return {n: getattr(pc, n).grad for n in RAW}


def _four(fn, what):
    runs = pz.run_all(fn)
    pz.assert_identical(runs, what)
    return runs[0][1]


def _assert_zero_rows(grads, rows, what):
    rows = rows.to(DEV)
    for name, g in grads.items():
        if torch.is_tensor(g) and g.dim() >= 1 and g.shape[0] == rows.shape[0]:
            assert not g[rows].any(), f"{what}: rows of culled / never-hit Gaussians of {name} are not exact zeros"


def _image_close(img, ref_color, what, tol=1e-4):
    err = gpu_common.rel_err(img.detach().cpu().numpy(), ref_color)
    assert err <= tol, f"{what}: image rel err {err:.3g} against the oracle"


# ---- training render + backward -----------------------------------------------------------------------------------------------------
FUSED = {
    "default": {}, "far": {}, "degree0": {}, "canonical": {"fast_exp": False}, "antialiasing": {"antialiasing": True},
    "absgrad": {"absgrad": True}, "camera_grad": {"camera_grad": True}, "no_sh_jacobian": {"sh_jacobian": False},
    "k1_lds": {"k1_lds": True}, "narrow_key": {"narrow_key": True}, "sort_all_bits": {"sort_all_bits": True},
    "seg64_serial": {"segment_length": 64, "long_tiles": "serial"}, "seg64_parallel": {"segment_length": 64, "long_tiles": "parallel"},
    "exact_forward": {"sync_free": False},
}


@pytest.mark.parametrize("variant", FUSED)
def test_render_fused_raw_parameters(variant):
    """gaussian_renderer.render on the raw parameters (the fused path) + backward: image, radii, visibility, every parameter's .grad,
    viewspace_points.grad (and .absgrad), the camera gradients."""
    from lightgaussian_amd.gaussian_renderer import render
    facts = preconditions()
    name = "far" if variant == "far" else "inside"
    deg = 0 if variant == "degree0" else 3
    opts = FUSED[variant]
    cam = model()[1][name].to(DEV)
    gimg, bg, pipe = _gimg().to(DEV), torch.tensor(BG, device=DEV), syn.PipelineParams()

    def run():
        pc = _leaf_model(deg)
        view_cam = cam
        leaves = {}
        if opts.get("camera_grad"):
            view_cam = syn.MiniCam.__new__(syn.MiniCam)
            view_cam.__dict__.update(cam.__dict__)
            for n in ("world_view_transform", "full_proj_transform", "camera_center"):
                leaves[n] = getattr(cam, n).detach().clone().requires_grad_(True)
                setattr(view_cam, n, leaves[n])
        pkg = render(view_cam, pc, pipe, bg, options=opts)
        (pkg["render"] * gimg).sum().backward()
        out = dict(render=pkg["render"].detach(), radii=pkg["radii"], visible=pkg["visibility_filter"].clone(), grads=_raw_grads(pc),
                   viewspace=pkg["viewspace_points"].grad, camera={n: t.grad for n, t in leaves.items()})
        if opts.get("absgrad"):
            out["absgrad"] = pkg["viewspace_points"].absgrad
        return out

    out = _four(run, f"render fused {variant}")
    ref = view(name, deg)["ref"]
    assert np.array_equal(out["radii"].cpu().numpy(), ref.radii)
    if variant != "antialiasing":
        _image_close(out["render"], ref.color, variant, tol=2e-4)        # (the raw path evaluates the getters in the kernel: ~1e-7 on the inputs)
    if name == "inside":
        rows = facts["no_gradient"]
        _assert_zero_rows(dict(out["grads"], viewspace=out["viewspace"], absgrad=out.get("absgrad")), rows, variant)
        assert float(out["grads"]["_xyz"].abs().sum()) > 0
    if opts.get("camera_grad"):
        assert [tuple(t.shape) for t in out["camera"].values()] == [(4, 4), (4, 4), (3,)] and all(t.abs().sum() > 0 for t in out["camera"].values())


LITERAL = {
    "default": dict(), "degree0": dict(deg=0), "colors_precomp": dict(precolor=True), "cov3D_precomp": dict(precov=True),
    "canonical": dict(options={"fast_exp": False}), "antialiasing": dict(options={"antialiasing": True}),
    "absgrad": dict(options={"absgrad": True}), "camera_grad": dict(camera_grad=True), "no_sh_jacobian": dict(options={"sh_jacobian": False}),
    "k1_lds": dict(options={"k1_lds": True}), "narrow_key": dict(options={"narrow_key": True}), "sort_all_bits": dict(options={"sort_all_bits": True}),
    "seg64_serial": dict(options={"segment_length": 64, "long_tiles": "serial"}),
    "seg64_parallel": dict(options={"segment_length": 64, "long_tiles": "parallel"}),
    "far": dict(view="far"),
}


@pytest.mark.parametrize("variant", LITERAL)
def test_rasterizer_literal_path(variant):
    """GaussianRasterizer on activated inputs, through gpu_common.run_rasterizer: image, radii, the gradient of every input, means2D.grad
    (and .absgrad), all 16 + 16 + 3 camera-gradient entries."""
    facts = preconditions()
    spec = LITERAL[variant]
    name, deg = spec.get("view", "inside"), spec.get("deg", 3)
    g, cams = model()
    pre = torch.rand(g.num, 3, generator=torch.Generator().manual_seed(7)) if spec.get("precolor") else None
    kw = common.scene_kwargs(g, cams[name], W, H, deg=deg, precolor=pre, precov=bool(spec.get("precov")), bg=BG, as_torch=True)
    gimg = _gimg()

    def run():
        r = gpu_common.run_rasterizer(kw, gimg, spec.get("options"), camera_grad=bool(spec.get("camera_grad")))
        out = dict(image=r["image"].detach(), radii=r["radii"], grads=r["grads"], camera=r["camera"])
        if (spec.get("options") or {}).get("absgrad"):
            out["absgrad"] = r["means2D"].absgrad
        return out

    out = _four(run, f"rasterizer {variant}")
    ref = oracle.forward(**common.to_numpy(kw))
    assert np.array_equal(out["radii"].cpu().numpy(), ref.radii)
    if variant != "antialiasing":
        _image_close(out["image"], ref.color, variant)
    if name == "inside":
        _assert_zero_rows(dict(out["grads"], absgrad=out.get("absgrad")), facts["no_gradient"], variant)
        assert float(out["grads"]["means3D"].abs().sum()) > 0
    if spec.get("camera_grad"):
        assert sorted(out["camera"]) == sorted(("viewmatrix", "projmatrix", "campos")) and sum(v.size for v in out["camera"].values()) == 35


# ---- count_render -----------------------------------------------------------------------------------------------------------------
POLICY_ID = {"one": oracle.W_ONE, "opacity": oracle.W_OPACITY, "alpha": oracle.W_ALPHA, "alpha_t": oracle.W_ALPHA_T}


def _frozen():
    from lightgaussian_amd import prune
    g, _ = model()
    with torch.no_grad():
        return prune._FrozenGetters(g.to(DEV))


def _count_oracle(policy):
    """The oracle on what the kernels see: torch's getters evaluated ON THE DEVICE (their last bit differs from the CPU's)."""
    pc = _frozen()
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    kw = dict(view("inside")["kw"], means3D=c(pc.get_xyz), opacities=c(pc.get_opacity), shs=c(pc.get_features), scales=c(pc.get_scaling),
              rotations=c(pc.get_rotation))
    return oracle.forward(count=True, weight_policy=POLICY_ID[policy], **kw)


@pytest.mark.parametrize("skip_color", [False, True])
@pytest.mark.parametrize("policy", sorted(POLICY_ID))
def test_count_render(policy, skip_color):
    """Every weight policy with and without the image, on the exact and the bounded forward -- for the per-hit policies this is every
    fast / colour combination a count forward has (count forwards always use the canonical exp), i.e. the variant that MERGES in LDS and
    stores every slot once, and the variant that adds into slots a clear node must have zeroed (the keys_in hazard of ADVICE.md) --
    and with caller-owned score_out / count_sum, count_sum starting from a known non-zero value."""
    from lightgaussian_amd import rasterizer
    from lightgaussian_amd.gaussian_renderer import count_render
    preconditions()
    pc, cam = _frozen(), model()[1]["inside"].to(DEV)
    bg, pipe = torch.tensor(BG, device=DEV), syn.PipelineParams()
    N = pc.get_xyz.shape[0]
    keys = ("gaussians_count", "important_score", "radii") + (() if skip_color else ("render",))

    def run():
        out = {}
        with torch.no_grad():
            for mode in (False, "validated"):
                rasterizer._CAPACITY.clear()
                opts = {"weight_policy": policy, "skip_color_in_count": skip_color, "sync_free": mode}
                first = count_render(cam, pc, pipe, bg, options=opts)                      # exact (learns the capacity)
                second = count_render(cam, pc, pipe, bg, options=opts)                     # bounded under "validated"
                rows = torch.full((2, N + 5), -3.0, device=DEV)
                running = torch.full((N,), 7, dtype=torch.int32, device=DEV)
                owned = count_render(cam, pc, pipe, bg, options=dict(opts, score_out=rows[1, :N], count_sum=running))
                assert owned["important_score"].data_ptr() == rows[1].data_ptr()
                out[str(mode)] = dict(first={k: first[k] for k in keys}, second={k: second[k] for k in keys},
                                      owned={k: owned[k] for k in keys}, rows=rows, running=running)
        rasterizer._CAPACITY.clear()
        return out

    out = _four(run, f"count_render {policy} skip_color={skip_color}")
    ref = _count_oracle(policy)
    for mode, o in out.items():
        for which in ("first", "second", "owned"):
            assert np.array_equal(o[which]["gaussians_count"].cpu().numpy(), ref.count), (mode, which)
            assert np.array_equal(common.bits(o[which]["important_score"]), common.bits(ref.score)), (mode, which)
        assert torch.equal(o["running"], o["first"]["gaussians_count"] + 7)             # exactly the view's count was added
        assert bool((o["rows"][0] == -3.0).all()) and bool((o["rows"][1, N:] == -3.0).all())
        if not skip_color:
            assert np.array_equal(common.bits(o["first"]["render"]), common.bits(ref.color))


@pytest.mark.parametrize("wide_band", [False, True])
def test_count_render_parallel_long_tiles(wide_band):
    """The significance-only pass's parallel walk of long lists (lg_count_seg / _rewalk / _fixup) at segment_length 64."""
    from lightgaussian_amd.gaussian_renderer import count_render
    preconditions()
    pc, cam = _frozen(), model()[1]["inside"].to(DEV)
    bg, pipe = torch.tensor(BG, device=DEV), syn.PipelineParams()
    opts = {"weight_policy": "opacity", "skip_color_in_count": True, "count_long_tiles": "parallel", "count_wide_band": wide_band,
            "segment_length": 64, "sync_free": False}

    def run():
        with torch.no_grad():
            o = count_render(cam, pc, pipe, bg, options=opts)
        return {k: o[k] for k in ("gaussians_count", "important_score", "radii")}

    out = _four(run, f"count parallel wide_band={wide_band}")
    ref = _count_oracle("opacity")
    assert np.array_equal(out["gaussians_count"].cpu().numpy(), ref.count)
    assert np.array_equal(common.bits(out["important_score"]), common.bits(ref.score))


# ---- sync-free modes --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def _clean_capacity():
    from lightgaussian_amd import rasterizer
    rasterizer._CAPACITY.clear()
    rasterizer.pending_status()
    yield
    rasterizer.pending_status()
    rasterizer._CAPACITY.clear()


@pytest.mark.parametrize("mode", [False, "validated", True], ids=lambda m: f"sync_free_{m}")
def test_sync_free_modes_with_a_fitting_and_a_small_capacity(mode, _clean_capacity):
    """Forward + backward in each mode with the capacity the first view learnt, then with a capacity that is far too small: under True the
    abandoned view returns the same zeros / background and the same status words in every run, under "validated" it is repaired and equals
    the exact view."""
    from lightgaussian_amd import rasterizer
    from lightgaussian_amd.gaussian_renderer import render, count_render
    facts = preconditions()
    cam = model()[1]["inside"].to(DEV)
    gimg, bg, pipe = _gimg().to(DEV), torch.tensor(BG, device=DEV), syn.PipelineParams()
    key = (0, facts["N"], W, H)

    def step(opts):
        pc = _leaf_model()
        pkg = render(cam, pc, pipe, bg, options=opts)
        (pkg["render"] * gimg).sum().backward()
        with torch.no_grad():
            cnt = count_render(cam, pc, pipe, bg, options=opts)
        return dict(render=pkg["render"].detach(), radii=pkg["radii"], grads=_raw_grads(pc), viewspace=pkg["viewspace_points"].grad,
                    count=cnt["gaussians_count"], score=cnt["important_score"], count_image=cnt["render"])

    def run():
        rasterizer._CAPACITY.clear()
        out = {"learn": step({"sync_free": mode}), "fit": step({"sync_free": mode})}
        out["pending_fit"] = [bool(b) for b in rasterizer.pending_status()]
        if mode:
            assert rasterizer._CAPACITY[key] > 1000
            rasterizer._CAPACITY[key] = 600                               # far below the view's instance count
            status = torch.full((4,), -1, dtype=torch.int32, device=DEV)
            if mode is True:
                pc = _leaf_model()
                pkg = render(cam, pc, pipe, bg, options={"sync_free": True, "status_override": status})
                (pkg["render"] * gimg).sum().backward()
                with torch.no_grad():
                    cnt = count_render(cam, pc, pipe, bg, options={"sync_free": True})
                out["small"] = dict(render=pkg["render"].detach(), radii=pkg["radii"], grads=_raw_grads(pc), viewspace=pkg["viewspace_points"].grad,
                                    count=cnt["gaussians_count"], score=cnt["important_score"], count_image=cnt["render"], status=status)
            else:
                out["small"] = step({"sync_free": mode})
            out["pending_small"] = [bool(b) for b in rasterizer.pending_status()]
        rasterizer._CAPACITY.clear()
        return out

    out = _four(run, f"sync_free={mode}")
    ref = view("inside")["ref"]
    _image_close(out["fit"]["render"], ref.color, f"sync_free={mode}", tol=2e-4)
    assert np.array_equal(out["fit"]["count"].cpu().numpy(), _count_oracle("opacity").count)
    pz.assert_identical([("learn", out["learn"]), ("fit", out["fit"])], "exact against bounded")
    if mode == "validated":
        pz.assert_identical([("fit", out["fit"]), ("repaired", out["small"])], "validated repair")
        assert out["pending_small"] == []
    if mode is True:
        small = out["small"]
        assert out["pending_fit"] == [False] * 4 and out["pending_small"] == [True, True]
        assert not small["count"].any() and not small["score"].any() and all(not g.any() for g in small["grads"].values())
        assert torch.equal(small["radii"], out["fit"]["radii"])
        background = torch.tensor(BG, device=DEV)[:, None, None].expand(3, H, W)
        assert torch.equal(small["render"], background) and torch.equal(small["count_image"], background)
        assert int(small["status"][0]) & 1 and 600 < int(small["status"][3]) < (1 << 30)      # abandoned for its size; the device's own count


# ---- backward over views, chunked backward -------------------------------------------------------------------------------------------
def test_backward_over_views(_clean_capacity):
    from lightgaussian_amd import parallel, rasterizer
    preconditions()
    _g, cams = model()
    views = [cams["inside"].to(DEV), cams["far"].to(DEV), camera_common.camera("pitched_rolled").to(DEV)]
    targets = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(k)).to(DEV) for k in range(3)]
    bg, pipe = torch.tensor(BG, device=DEV), syn.PipelineParams()
    loss_fn = lambda img, gt: (img - gt).abs().mean()  # noqa: E731

    def run():
        rasterizer._CAPACITY.clear()
        pc = _leaf_model()
        losses = parallel.backward_over_views(pc, views, targets, pipe, bg, loss_fn, streams=3)
        return dict(losses=torch.stack([x.detach().reshape(()) if torch.is_tensor(x) else torch.tensor(float(x)) for x in losses]).cpu(),
                    grads=_raw_grads(pc))

    out = _four(run, "backward_over_views")
    # the oracle of this path: the same three views one after the other, plain render + backward
    from lightgaussian_amd.gaussian_renderer import render
    pc = _leaf_model()
    for v, t in zip(views, targets):
        loss_fn(render(v, pc, pipe, bg)["render"], t).backward()
    for n in RAW:
        want, got = getattr(pc, n).grad, out["grads"][n]
        assert float((want - got).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-12, n


def test_chunked_backward():
    """set_grad_chunk_hook(..., chunks=3): three K9 launches over Gaussian ranges; the rows handed to the hook and the final gradients."""
    from lightgaussian_amd import rasterizer
    facts = preconditions()
    g, cams = model()
    kw = common.scene_kwargs(g, cams["inside"], W, H, bg=BG, as_torch=True)
    gimg = _gimg()

    def run():
        seen = []
        rasterizer.set_grad_chunk_hook(lambda first, count, grads: seen.append((first, count, sorted(grads))), chunks=3)
        try:
            r = gpu_common.run_rasterizer(kw, gimg)
        finally:
            rasterizer.set_grad_chunk_hook(None)
        assert len(seen) == 3 and seen[0][0] == 0 and sum(c for _f, c, _n in seen) == facts["N"]
        return dict(image=r["image"].detach(), radii=r["radii"], grads=r["grads"], ranges=torch.tensor([(f, c) for f, c, _n in seen]))

    out = _four(run, "chunked backward")
    plain = gpu_common.run_rasterizer(kw, gimg)
    pz.assert_identical([("one launch", dict(image=plain["image"].detach(), grads=plain["grads"])),
                         ("three chunks", dict(image=out["image"], grads=out["grads"]))], "chunks against the single launch")
    _assert_zero_rows(out["grads"], facts["no_gradient"], "chunked")


# ---- feature maps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["c7", "c7_bg", "c17_seg64", "depth_geometry", "depth_geometry_bg_seg64"])
def test_render_features(case):
    from lightgaussian_amd.gaussian_renderer import render_features
    facts = preconditions()
    g, cams = model()
    cam = cams["inside"].to(DEV)
    pipe = syn.PipelineParams()
    N = facts["N"]
    gen = torch.Generator().manual_seed(23)
    depth = case.startswith("depth")
    C = 1 if depth else 17 if "c17" in case else 7
    F = torch.randn(N, C, generator=gen).to(DEV)
    bgf = torch.randn(C, generator=gen).to(DEV) if "bg" in case else None
    dout, dalpha = torch.randn(C, H, W, generator=gen).to(DEV), torch.randn(H, W, generator=gen).to(DEV)
    gimg = _gimg().to(DEV)
    opts = {"fast_exp": False}
    if "seg64" in case:
        opts["segment_length"] = 64

    def run():
        pc = _leaf_model()
        if depth:
            pkg = render_features(cam, pc, pipe, "depth", bg_features=bgf, options=opts, geometry_grad=True, bg_color=torch.tensor(BG, device=DEV))
            ((pkg["features"] * dout).sum() + (pkg["alpha"] * dalpha).sum() + (pkg["render"] * gimg).sum() + pkg["depth"].sum()).backward()
            return dict(features=pkg["features"].detach(), alpha=pkg["alpha"].detach(), render=pkg["render"].detach(), radii=pkg["radii"],
                        depth=pkg["depth"].detach(), grads=_raw_grads(pc), viewspace=pkg["viewspace_points"].grad)
        feats = F.clone().requires_grad_(True)
        pkg = render_features(cam, pc, pipe, feats, bg_features=bgf, options=opts, bg_color=torch.tensor(BG, device=DEV))
        (pkg["features"] * dout).sum().backward()
        return dict(features=pkg["features"].detach(), alpha=pkg["alpha"], render=pkg["render"], radii=pkg["radii"], d_features=feats.grad)

    out = _four(run, f"render_features {case}")
    ref = _count_oracle("opacity")
    assert np.array_equal(out["radii"].cpu().numpy(), ref.radii)
    assert np.array_equal(common.bits(out["render"]), common.bits(ref.color))            # canonical exp: the colour by-product is the oracle's
    if depth:
        _assert_zero_rows(dict(out["grads"], viewspace=out["viewspace"]), facts["no_gradient"], case)
        assert float(out["grads"]["_xyz"].abs().sum()) > 0
    else:
        assert not out["d_features"][facts["no_gradient"].to(DEV)].any() and float(out["d_features"].abs().sum()) > 0


# ---- compressed models --------------------------------------------------------------------------------------------------------------
def test_render_compressed_and_trainable():
    """The small hand-packed model of vq_finetune_common: empty codes, a code of exactly 256 rows and one of 257."""
    import vq_finetune_common as fc
    from lightgaussian_amd import vectree
    from lightgaussian_amd.gaussian_renderer import render, render_compressed
    packed = fc.packed_by_hand(3001, 2)
    cam = syn.orbit_camera(1, 8, fc.W, fc.H).to(DEV)
    bg, pipe = torch.tensor(BG, device=DEV), syn.PipelineParams()
    gimg = torch.randn(3, fc.H, fc.W, generator=torch.Generator().manual_seed(4)).to(DEV)

    def run():
        cg = vectree.CompressedGaussians.from_packed(packed, DEV)
        fwd = render_compressed(cam, cg, pipe, bg)
        tc = cg.trainable(fc.ALL_PARAMS)
        pkg = render(cam, tc, pipe, bg)
        (pkg["render"] * gimg).sum().backward()
        return dict(forward={k: fwd[k] for k in ("render", "radii", "visibility_filter")}, render=pkg["render"].detach(), radii=pkg["radii"],
                    grads={n: getattr(tc, "_" + n).grad for n in fc.ALL_PARAMS}, viewspace=pkg["viewspace_points"].grad)

    out = _four(run, "compressed")
    assert torch.equal(out["forward"]["render"], out["render"])                          # the documented promise: the same image bits
    cg = vectree.CompressedGaussians.from_packed(packed, DEV)
    with torch.no_grad():
        dense = render(cam, cg.to_dense(), pipe, bg, options=fc.UNFUSED)["render"]
    assert torch.equal(dense, out["render"])                                              # ... as render() of to_dense() with the getters unfused
    used = torch.zeros(out["grads"]["rows"].shape[0], dtype=torch.bool, device=DEV)
    used[cg._slot.long()] = True
    assert not used[list(fc.HAND_EMPTY)].any() and not out["grads"]["rows"][~used].any() and float(out["grads"]["rows"].abs().sum()) > 0


@pytest.mark.parametrize("n,d,K,seed", [(129, 3, 7, 4), (1000, 12, 100, 3)])
def test_vq_nearest_code(n, d, K, seed):
    from lightgaussian_amd import vq
    from oracle import vq_oracle
    rng = np.random.default_rng(seed)
    e = (rng.standard_normal((K, d)) * 0.3).astype(np.float32)
    x = (e[rng.integers(0, K, n)] + 0.1 * rng.standard_normal((n, d))).astype(np.float32)
    xt, et = torch.tensor(x, device=DEV), torch.tensor(e, device=DEV)
    out = _four(lambda: {"ind": vq.nearest_code(xt, et), "ind3": vq.nearest_code(xt[None], et[None])}, f"nearest_code {n} {d} {K}")
    ref, gap = vq_oracle.nearest_code(x, e)
    ind = out["ind"].cpu().numpy()
    bad = np.nonzero(ind != ref)[0]
    scale = float(np.abs(x).max() * np.sqrt(d)) + 1e-30
    assert all(gap[i] < 1e-5 * scale for i in bad) and len(bad) <= 2 and ind.min() >= 0 and ind.max() < K


def test_vq_ema_update_and_train_codebook():
    """Two steps of ema_update (weighted, with codes nobody is assigned to) and two iterations of train_codebook: the codebook and the
    cluster sizes are updated in place."""
    import vq_train_common as vt
    from lightgaussian_amd import vq
    n, d, K = 1000, 12, 100
    rng = np.random.default_rng(9)
    e0 = (rng.standard_normal((K, d)) * 0.3).astype(np.float32)
    e0[90:] += 50.0                                                                        # ten codes far from every row: they receive none
    x = (e0[rng.integers(0, 90, n)] + 0.1 * rng.standard_normal((n, d))).astype(np.float32)
    w = rng.random(n).astype(np.float32) + 0.1
    xt, wt = torch.tensor(x, device=DEV), torch.tensor(w, device=DEV)

    def run():
        embed, cs = torch.tensor(e0, device=DEV), torch.ones(K, device=DEV)
        first = vq.ema_update(xt, embed, cs, weight=wt)
        after_one = (embed.clone(), cs.clone())
        ind, quant = vq.ema_update(xt, embed, cs, weight=wt, return_quantized=True)
        embed2, cs2 = torch.tensor(e0, device=DEV), torch.ones(K, device=DEV)
        errors = vq.train_codebook(xt, wt, embed2, cs2, iterations=2, chunk=700, k_expire=3, generator=torch.Generator(DEV).manual_seed(5))
        return dict(first=first, after_one=after_one, ind=ind, quant=quant, embed=embed, cs=cs, embed2=embed2, cs2=cs2, errors=errors)

    out = _four(run, "ema_update / train_codebook")
    ind64, _best, gap = vt.nearest_f64(x, e0)
    bad = np.flatnonzero(out["first"].cpu().numpy() != ind64)
    assert len(bad) <= 2 and all(gap[i] < 1e-5 * float(np.abs(x).max() * np.sqrt(d)) for i in bad)      # (a disagreement is a near tie)
    e64, c64 = vt.ema_step_f64(x, w, e0, np.ones(K), out["first"].cpu().numpy())[:2]
    assert np.abs(out["after_one"][0].cpu().numpy() - e64).max() <= 1e-4 * np.abs(e64).max()
    assert np.abs(out["after_one"][1].cpu().numpy() - c64).max() <= 1e-4 * np.abs(c64).max()
    assert torch.isfinite(out["errors"]).all() and float(out["errors"][0]) > 0


# ---- the photometric loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("shape", [(3, 33, 31), (1, 35, 65)])
def test_l1_dssim_loss(shape, lazy):
    from lightgaussian_amd import loss_utils as LU
    from oracle import loss_oracle as LO
    rng = np.random.default_rng(31)
    x = rng.random(shape, dtype=np.float32)
    y = np.clip(x + 0.1 * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    lam = 0.2

    def run():
        xt, yt = torch.tensor(x, device=DEV, requires_grad=True), torch.tensor(y, device=DEV)
        prev = LU.set_lazy(lazy)
        try:
            if lazy:                                     # the reference's two calls and its formula, on LazyLoss scalars
                l1 = LU.l1_loss(xt, yt)
                loss = (1.0 - lam) * l1 + lam * (1.0 - LU.ssim(xt, yt))
            else:
                loss, l1 = LU.l1_dssim_loss(xt, yt, lam)
            loss.backward()
            return dict(loss=torch.tensor(loss.item()), l1=torch.tensor(l1.item()), grad=xt.grad)
        finally:
            LU.set_lazy(prev)

    out = _four(run, f"l1_dssim_loss {shape} lazy={lazy}")
    assert float(out["loss"]) == pytest.approx(LO.l1_dssim(x, y, lam), rel=1e-4) and float(out["l1"]) == pytest.approx(LO.l1_loss(x, y), rel=1e-4)
    ref = LO.l1_dssim_grad(x, y, lam)
    assert np.abs(out["grad"].cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()


# ---- prune ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_pow", [False, True])
@pytest.mark.parametrize("N,seed,zero_frac,ties,percent,v_pow", [(257, 3, 0.3, False, 0.66, 0.1), (5000, 5, 0, True, 0.3, 0.1)])
def test_prune_epilogue(N, seed, zero_frac, ties, percent, v_pow, fused_pow):
    import test_gpu_prune_epilogue as pe
    from lightgaussian_amd import prune
    assert (N, seed, zero_frac, ties, percent, v_pow) in pe.CASES
    scaling, imp = pe._case(N, seed, zero_frac, ties)
    st, it = torch.tensor(scaling, device=DEV), torch.tensor(imp, device=DEV)

    def run():
        v_list, mask, thr = prune.prune_epilogue(pe._G(st), it, v_pow, percent, fused_pow=fused_pow)
        return dict(v_list=v_list, mask=mask, thresholds=thr)

    out = _four(run, f"prune_epilogue N={N} fused_pow={fused_pow}")
    assert np.array_equal(out["mask"].cpu().numpy(), oracle.prune_mask(percent, out["v_list"].cpu().numpy()))
    if not fused_pow:
        tv = prune.calculate_v_imp_score(pe._G(st), it, v_pow)
        assert torch.equal(out["v_list"], tv) and torch.equal(out["mask"], prune.prune_mask(percent, tv).reshape(-1))


@pytest.mark.parametrize("N", [1, 1023, 1025])
def test_compact_tensors(N):
    from lightgaussian_amd import prune
    gen = torch.Generator().manual_seed(N)
    keep = (torch.rand(N, generator=gen) < 0.5).to(DEV)
    if N == 1:
        keep[:] = True
    ts = [torch.randn(*s, generator=gen).to(DEV) for s in [(N, 3), (N, 15, 3), (N, 1), (N, 4), (N,)]]
    ts += [torch.randint(0, 1000, (N,), generator=gen, dtype=torch.int32).to(DEV), torch.randint(0, 2, (N, 3), generator=gen, dtype=torch.uint8).to(DEV)]
    out = _four(lambda: {"kept": prune.compact_tensors(ts, keep), "none": prune.compact_tensors(ts[:2], torch.zeros_like(keep))}, f"compact N={N}")
    for t, o in zip(ts, out["kept"]):
        assert o.dtype == t.dtype and torch.equal(o, t[keep])
    assert all(o.shape[0] == 0 for o in out["none"])


def test_prune_points_with_adam_state():
    import test_gpu_compact as tc
    from lightgaussian_amd import prune
    N = 1025
    mask = (torch.rand(N, generator=torch.Generator().manual_seed(9)) < 0.66).to(DEV)

    def run():
        m = tc._Model(N, 3, steps=2)
        prune.prune_points(m, mask)
        return tc._state(m)

    out = _four(run, "prune_points")
    want = tc._Model(N, 3, steps=2)
    want.reference_prune_points(mask)
    pz.assert_identical([("reference", tc._state(want)), ("prune_points", out)], "prune_points against the reference's statements")


def test_prune_list_over_three_views():
    from lightgaussian_amd import prune
    preconditions()
    _g, cams = model()
    views = [cams["inside"].to(DEV), cams["far"].to(DEV), camera_common.camera("inside_wide").to(DEV)]
    bg, pipe = torch.tensor(BG, device=DEV), syn.PipelineParams()
    pc = _frozen()
    with torch.no_grad():
        dense = model()[0].to(DEV)

    def run():
        with torch.no_grad():
            cnt, imp = prune.prune_list(pc, list(views), pipe, bg)
            scnt, simp = prune.prune_list_sharded(dense, list(views), pipe, bg, streams=2, block=2)
        return dict(count=cnt, score=imp, sharded_count=scnt, sharded_score=simp)

    out = _four(run, "prune_list")
    assert torch.equal(out["count"], out["sharded_count"]) and torch.equal(out["score"], out["sharded_score"])
    ref = _count_oracle("opacity")
    assert bool((out["count"].cpu().numpy() >= ref.count).all()) and int(out["count"].sum()) > int(ref.count.sum())


# ---- densify, MCMC ------------------------------------------------------------------------------------------------------------------
def _model_state(m):
    import densify_common as dc
    out = {}
    for n in dc.NAMES:
        p = m.param(n)
        st = m.optimizer.state[p]
        out[n], out["m_" + n], out["v_" + n] = p.detach(), st["exp_avg"], st["exp_avg_sq"]
    out.update(accum=m.xyz_gradient_accum, denom=m.denom, max_radii2D=m.max_radii2D)
    return out


def test_densify_stats_and_densify_and_prune():
    import densify_common as dc
    from lightgaussian_amd import densify
    c = dc.case("mixed")
    n = c["in_xyz"].shape[0]
    noise = torch.from_numpy(c["noise"]).to(DEV)
    gen = torch.Generator().manual_seed(2)
    vgrad = (torch.randn(n, 3, generator=gen) * 1e-4).to(DEV)
    f = (torch.rand(n, generator=gen) < 0.5).to(DEV)
    radii = torch.randint(0, 60, (n,), generator=gen, dtype=torch.int32).to(DEV)

    def run():
        stats = dc.model_of(c, device=DEV)
        vp = torch.zeros(n, 3, device=DEV)
        vp.grad = vgrad.clone()
        densify.accumulate_stats(stats, vp, f, radii=radii)
        m = dc.model_of(c, device=DEV)
        rec = densify.densify_and_prune(m, noise=noise, backend="hip", **c["kwargs"])
        return dict(stats=dict(accum=stats.xyz_gradient_accum, denom=stats.denom, max_radii2D=stats.max_radii2D), model=_model_state(m),
                    record=torch.tensor([rec[k] for k in ("N_out", "n_keep", "n_clone", "n_s", "n_child")]))

    _four(run, "densify")
    m = dc.model_of(c, device=DEV)
    densify.densify_and_prune(m, noise=noise, backend="hip", **c["kwargs"])
    dc.check_golden(m, c, "mixed")


def test_mcmc_add_noise_relocate_grow():
    import densify_common as dc
    import mcmc_common as mc
    from lightgaussian_amd import mcmc
    n = 257
    cn = mc.noise_case(n, seed=60 + n)
    noise = torch.from_numpy(cn["noise"]).to(DEV)
    c = mc.case(n, deg=1, seed=200 + n + 1)
    dead = mc.dead_rows(c)
    dst, alive = torch.nonzero(dead).reshape(-1), torch.nonzero(~dead).reshape(-1)
    src = mc.hand_draws(alive[:: max(1, alive.numel() // 40)], dst.numel())
    n_new = int(1.05 * n) - n
    gsrc = mc.hand_draws(range(0, n, max(1, n // 40)), n_new)

    def run():
        a, b, g = dc.model_of(cn, device=DEV), dc.model_of(c, device=DEV), dc.model_of(c, device=DEV)
        mcmc.add_noise(a, 1e-5, noise_lr=5e5, noise=noise, backend="hip")
        r1 = mcmc.relocate(b, draws=src.to(DEV), backend="hip")
        r2 = mcmc.grow(g, draws=gsrc.to(DEV), backend="hip", cap_max=10 ** 6, factor=1.05)
        return dict(noise_xyz=a._xyz.detach(), relocate=_model_state(b), grow=_model_state(g),
                    records=torch.tensor([int(v) for r in (r1, r2) for k, v in sorted(r.items()) if k != "backend"]))

    out = _four(run, "mcmc")
    b = dc.model_of(c, device=DEV)
    mcmc.relocate(b, draws=src.to(DEV), backend="hip")
    mc.check_state(b, mc.expected_state(c, dst, src, n, 0.005), dst, src, "hip relocate", exact=True)
    g = dc.model_of(c, device=DEV)
    mcmc.grow(g, draws=gsrc.to(DEV), backend="hip", cap_max=10 ** 6, factor=1.05)
    gdst = torch.arange(n, n + n_new)
    mc.check_state(g, mc.expected_state(c, gdst, gsrc, n + n_new, 0.005), gdst, gsrc, "hip grow", exact=True)
    assert out["grow"]["xyz"].shape[0] == n + n_new


# ---- the 3D filter --------------------------------------------------------------------------------------------------------------------
def test_filter_3d():
    import filter3d_common as f3
    from lightgaussian_amd import filter3d
    N, V, (Wf, Hf) = 257, 3, f3.SIZES[0]
    means, rows = f3.points(N, V, Wf, Hf)
    table = filter3d.camera_table(f3.cameras(V, Wf, Hf))
    xyz = torch.from_numpy(means).to(DEV)
    r, o, f = (t.to(DEV) for t in f3.rows(N))
    gs, go = torch.randn(N, 3, generator=torch.Generator().manual_seed(1)).to(DEV), torch.randn(N, 1, generator=torch.Generator().manual_seed(2)).to(DEV)

    class Holder:
        pass

    def run():
        filt, seen = filter3d.compute_filter_3d(xyz, table, return_seen=True)
        rl, ol = r.clone().requires_grad_(True), o.clone().requires_grad_(True)
        s2, o2 = filter3d.apply_filter_3d(rl, ol, f)
        ((s2 * gs).sum() + (o2 * go).sum()).backward()
        m = Holder()
        m._scaling, m._opacity, m.filter_3D = r, o, f
        fs, fo = filter3d.fuse_filter_3d(m)
        act = filter3d.apply_filter_3d_activated(torch.exp(r), torch.sigmoid(o), f)
        return dict(filter=filt, seen=seen, scaling=s2.detach(), opacity=o2.detach(), d_scaling=rl.grad, d_opacity=ol.grad, fused=(fs, fo), activated=act)

    out = _four(run, "filter3d")
    want = f3.run_harness(means, rows)
    assert np.array_equal(out["seen"].cpu().numpy(), want["seen"]) and 0 < int(want["seen"].sum()) < N
    assert np.array_equal(common.bits(out["filter"].reshape(-1)), common.bits(want["filter"]))
    assert torch.equal(out["fused"][0], out["scaling"]) and torch.equal(out["fused"][1], out["opacity"])
    s64, o64 = f3.apply_formula(torch.exp(r.double().cpu()), torch.sigmoid(o.double().cpu()), f.double().cpu(), False)    # the activated domain
    for got, want in ((torch.exp(out["scaling"].double().cpu()), s64), (torch.sigmoid(out["opacity"].double().cpu()), o64),
                      (out["activated"][0].double().cpu(), s64), (out["activated"][1].double().cpu(), o64)):
        assert float(((got - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 1e-5


# ---- kNN ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 64, 1000])
@pytest.mark.parametrize("kind", ["duplicates", "outliers"])
def test_knn(kind, n):
    import zlib
    from oracle import knn_oracle as KO
    from simple_knn._C import distCUDA2
    from test_knn import CLOUDS
    rng = np.random.default_rng(zlib.crc32(f"{kind}:{n}".encode()))
    p = CLOUDS[kind](rng, max(n, 8)).astype(np.float32)
    pt = torch.tensor(p, device=DEV)
    out = _four(lambda: {"dist2": distCUDA2(pt)}, f"knn {kind} {n}")
    want = KO.dist_cuda2(p)
    got = out["dist2"].cpu().numpy()
    assert got.shape == want.shape and np.allclose(got, want, rtol=2e-6, atol=1e-12)
