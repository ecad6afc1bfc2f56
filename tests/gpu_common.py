"""GPU-side helpers: run the HIP rasterizer through the drop-in API and compare with the oracle."""
import torch

import common  # noqa: F401
import dense_twin
import tolerance
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
from oracle import oracle


def hip_forward_backward(kw_t, *, count=False, grad_image=None, debug=False):
    """kw_t: scene_kwargs(..., as_torch=True) on CPU.  Returns dict of numpy outputs (+grads)."""
    dev = torch.device("cuda:0")
    t = {k: (v.detach().to(dev).clone() if torch.is_tensor(v) else v) for k, v in kw_t.items()}
    names = dense_twin.PER_GAUSSIAN
    for n in names:
        if n in t and grad_image is not None:
            t[n].requires_grad_(True)
    N = t["means3D"].shape[0]
    means2D = torch.zeros((N, 3), device=dev, requires_grad=grad_image is not None)
    rs = GaussianRasterizationSettings(
        image_height=t["H"], image_width=t["W"], tanfovx=t["tanfovx"], tanfovy=t["tanfovy"], bg=t["bg"],
        scale_modifier=t.get("scale_modifier", 1.0), viewmatrix=t["viewmatrix"], projmatrix=t["projmatrix"],
        sh_degree=t["sh_degree"], campos=t["campos"], prefiltered=False, debug=debug, f_count=count)
    rast = GaussianRasterizer(raster_settings=rs)
    out = rast(means3D=t["means3D"], means2D=means2D, opacities=t["opacities"], shs=t.get("shs"),
               colors_precomp=t.get("colors_precomp"), scales=t.get("scales"), rotations=t.get("rotations"),
               cov3D_precomp=t.get("cov3D_precomp"))
    res = {}
    if count:
        cnt, score, color, radii = out
        res["count"] = cnt.cpu().numpy(); res["score"] = score.cpu().numpy()
    else:
        color, radii = out
    res["color"] = color.detach().cpu().numpy(); res["radii"] = radii.cpu().numpy()
    if grad_image is not None:
        (color * torch.as_tensor(grad_image, device=dev)).sum().backward()
        res["grads"] = {"means2D": means2D.grad.cpu().numpy()}
        for n in names:
            if n in t:
                res["grads"][n] = t[n].grad.cpu().numpy()
    torch.cuda.synchronize()
    return res


def run_rasterizer(kw, gimg, options=None, *, camera_grad=False, backwards=1, retain_graph=False, after_forward=None):
    """Forward + `backwards` backward passes of sum(image * gimg) through GaussianRasterizer (activated inputs).  kw: scene kwargs as CPU
    torch tensors; options: the rasterizer's (camera_grad is added to them); retain_graph: keep the graph after the last backward;
    after_forward(grad_fn, radii): called between the forward and the backward.  Returns a dict: image, radii, grads {name: tensor}
    (means2D among them), camera {name: array} or None, means2D (the leaf: .absgrad is read from it)."""
    dev = torch.device("cuda:0")
    t = {k: (v.detach().to(dev).clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
    names = [n for n in dense_twin.PER_GAUSSIAN if n in t]
    for n in names:
        t[n].requires_grad_(True)
    cam = {n: t[n].requires_grad_(camera_grad) for n in dense_twin.CAMERA}
    rs = GaussianRasterizationSettings(image_height=t["H"], image_width=t["W"], tanfovx=t["tanfovx"], tanfovy=t["tanfovy"], bg=t["bg"],
                                       scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], sh_degree=t["sh_degree"],
                                       campos=cam["campos"], prefiltered=False, debug=False, f_count=False)
    means2D = torch.zeros((t["means3D"].shape[0], 3), device=dev, requires_grad=True)
    color, radii = GaussianRasterizer(rs, options=dict(options or {}, camera_grad=camera_grad))(
        means3D=t["means3D"], means2D=means2D, opacities=t["opacities"], shs=t.get("shs"), colors_precomp=t.get("colors_precomp"),
        scales=t.get("scales"), rotations=t.get("rotations"), cov3D_precomp=t.get("cov3D_precomp"))
    if after_forward is not None:
        after_forward(color.grad_fn, radii)
    loss = (color * gimg.to(dev)).sum()
    for k in range(backwards):
        loss.backward(retain_graph=retain_graph or k + 1 < backwards)
    torch.cuda.synchronize()
    grads = {n: t[n].grad for n in names}
    grads["means2D"] = means2D.grad
    camera = None
    if camera_grad:
        for n, c in cam.items():
            assert c.grad is not None and c.grad.shape == c.shape and c.grad.dtype == torch.float32, n
        camera = {n: c.grad.detach().cpu().numpy().copy() for n, c in cam.items()}
    return dict(image=color, radii=radii, grads=grads, camera=camera, means2D=means2D)


TOL = tolerance.TOL  # north_star tolerance for floating-point outputs (relative to tensor max)
rel_err, elem_excess = tolerance.rel_err, tolerance.elem_excess


def assert_backward_parity(grads, g32, g64, *, well_conditioned=False, what=""):
    """The gradient rule of tests/test_gpu_parity.py::test_backward_parity.  grads: the HIP path's gradients by name; g32 / g64: the
    float32 / float64 oracle's backward on the same inputs: rule 3, the element-wise bound (on the well-conditioned scenes, where the
    float32 oracle itself meets it, without its slack) and -- on every scene, the saturating / screen-filling ones included, where the
    tensor-level bound is 8-1600x the element bound and no test would notice a 100x regression -- the quantiles of the element errors."""
    for name, g in grads.items():
        assert g64[name] is not None, name
        label = f"{what} grad {name}"
        tolerance.assert_rule3(g, g64[name], g32[name], label, ref="oracle", nonzero=False)
        tolerance.assert_elementwise(g, g64[name], g32[name], label, well_conditioned=well_conditioned)
        tolerance.assert_quantiles(g, g64[name], g32[name], label)
