"""-m gpu: what other tests and tools read off the autograd node of a render, stated once.

tests/test_gpu_sort.py, test_gpu_full_size.py, test_gpu_long_tiles.py, tools/gpu_fuzz.py and tools/reuse_probe.py rebuild a view from
`grad_fn.raster_settings / .num_rendered / .opts` and `grad_fn.saved_tensors` (positions first; radii, geom, binning, img last);
INTEGRATION.md and DESIGN.md name the Function classes.  One scene (N = 2500 at 144 x 96, as test_gpu_call_shapes._scene).
"""
import math

import numpy as np
import pytest
import torch

import common
import gpu_common
from common import syn
from lightgaussian_amd import _lib, rasterizer
from lightgaussian_amd.gaussian_renderer import render
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, W, H = 2500, 144, 96


@pytest.fixture(scope="module")
def scene():
    g = syn.make_gaussians(N, sh_degree=3, seed=21, log_scale_mean=math.log(0.03), opacity_mean=0.0, extent=(2, 1.2, 2), log_scale_std=0.5,
                           rest_std=0.15)
    return g, syn.orbit_camera(2, 7, W, H, radius=5.0)


def _literal(scene, options=None):
    """(colour, radii, positions, raster_settings) of a GaussianRasterizer call on leaves that require grad."""
    g, cam = scene
    kw = common.scene_kwargs(g, cam, W, H, deg=3, bg=(0.2, 0.1, 0.3), as_torch=True)
    t = {k: (v.detach().to(DEV).clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
    for n in ("viewmatrix", "projmatrix", "campos", "means3D", "opacities", "shs", "scales", "rotations"):
        t[n].requires_grad_(True)
    rs = GaussianRasterizationSettings(H, W, t["tanfovx"], t["tanfovy"], t["bg"], 1.0, t["viewmatrix"], t["projmatrix"], 3, t["campos"],
                                       False, False)
    color, radii = GaussianRasterizer(rs, options=options)(means3D=t["means3D"], means2D=torch.zeros(N, 3, device=DEV, requires_grad=True),
                                                           opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    return color, radii, t["means3D"], rs


def _fused(scene, options=None):
    g, cam = scene
    pc, c = g.to(DEV).requires_grad_(True), cam.to(DEV)
    for t in (c.world_view_transform, c.full_proj_transform, c.camera_center):
        t.requires_grad_(True)
    pkg = render(c, pc, syn.PipelineParams(), torch.tensor([0.2, 0.1, 0.3], device=DEV), options=dict(options or {}, fuse_getters=True))
    return pkg["render"], pkg["radii"], pc._xyz, None


@pytest.mark.parametrize("path, camera_grad, node", [
    (_literal, False, "_RasterizeGaussiansBackward"), (_literal, True, "_RasterizeGaussiansCameraBackward"),
    (_fused, False, "_RasterizeGaussiansRawBackward"), (_fused, True, "_RasterizeGaussiansRawCameraBackward")])
def test_node_type_attributes_and_saved_tensors(scene, path, camera_grad, node):
    color, radii, positions, rs = path(scene, {"camera_grad": camera_grad, "segment_length": 128, "tag": "per call only"})
    fn = color.grad_fn
    assert type(fn).__name__ == node
    if rs is not None:
        assert fn.raster_settings is rs
    assert (int(fn.raster_settings.image_height), int(fn.raster_settings.image_width)) == (H, W)
    assert isinstance(fn.num_rendered, int) and fn.num_rendered > 0
    assert set(fn.opts) == set(rasterizer._OPTIONS) and fn.opts["segment_length"] == 128 and fn.opts["camera_grad"] is camera_grad
    saved = fn.saved_tensors
    assert saved[0].data_ptr() == positions.data_ptr() and saved[0].shape == (N, 3)
    s_radii, geom, binning, img = saved[-4:]
    assert s_radii.data_ptr() == radii.data_ptr() and s_radii.dtype == torch.int32 and s_radii.shape == (N,)
    lib = _lib.load()
    assert geom.dtype == torch.uint8 and geom.numel() == lib.lg_geom_bytes(N)
    assert img.dtype == torch.uint8 and img.numel() == lib.lg_img_bytes(W, H)
    assert binning.dtype == torch.uint8 and binning.numel() == lib.lg_binning_bytes(fn.num_rendered, W, H, 128)


def test_the_backward_runs_with_the_options_on_the_node_at_backward_time(scene):
    """(test_gpu_long_tiles.py replaces grad_fn.opts on the fused path; here the literal one, with an option that leaves a trace)"""
    color, *_ = _literal(scene, {"profile": False})
    torch.cuda.synchronize()
    _lib.profile_reset()
    color.grad_fn.opts = dict(color.grad_fn.opts, profile=True)
    color.sum().backward()
    torch.cuda.synchronize()
    launches = {k: v[1] for k, v in _lib.profile_read().items() if v[1]}
    assert launches, "the backward did not see profile=True"
    _lib.profile_reset()
    color, *_ = _literal(scene, {"profile": False})
    color.sum().backward()
    torch.cuda.synchronize()
    assert not {k: v[1] for k, v in _lib.profile_read().items() if v[1]}


def test_backward_through_the_colour_of_a_count_render_is_the_canonical_backward(scene):
    """f_count=True returns (count, score, colour, radii): the colour's gradient arrives as grads[2], and a count render always
    uses the canonical arithmetic -- so its backward is, bit for bit, that of the plain render with fast_exp=False."""
    g, cam = scene
    kw = common.scene_kwargs(g, cam, W, H, deg=3, bg=(0.2, 0.1, 0.3), as_torch=True)
    gimg = np.random.RandomState(11).randn(3, H, W).astype(np.float32)
    counted = gpu_common.hip_forward_backward(kw, count=True, grad_image=gimg)
    with rasterizer.options(fast_exp=False):
        plain = gpu_common.hip_forward_backward(kw, grad_image=gimg)
    assert np.array_equal(counted["color"].view(np.uint32), plain["color"].view(np.uint32))
    assert set(counted["grads"]) == set(plain["grads"]) and len(plain["grads"]) == 6
    for name, grad in plain["grads"].items():
        assert np.abs(grad).max() > 0, name
        assert np.array_equal(counted["grads"][name].view(np.uint32), grad.view(np.uint32)), name
