"""GPU-side helpers: run the HIP rasterizer through the drop-in API and compare with the oracle."""
import math

import numpy as np
import torch

import common
from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
from oracle import oracle


def hip_forward_backward(kw_t, *, count=False, grad_image=None, debug=False):
    """kw_t: scene_kwargs(..., as_torch=True) on CPU.  Returns dict of numpy outputs (+grads)."""
    dev = torch.device("cuda:0")
    t = {k: (v.detach().to(dev).clone() if torch.is_tensor(v) else v) for k, v in kw_t.items()}
    names = ["means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"]
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


def rel_err(a, b):
    """max |a-b| relative to max |b| (tensor-level relative error used for the 1e-4 contract)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def elem_excess(a, b, rtol=1e-4, atol_frac=2e-5):
    """Element-wise check |a - b| <= rtol |b| + atol with atol = atol_frac * max|b| (an absolute floor for entries that are
    small only through cancellation).  Returns (worst ratio |a-b| / bound, flat index of the worst element): <= 1 passes."""
    a = np.asarray(a, np.float64).reshape(-1); b = np.asarray(b, np.float64).reshape(-1)
    bound = rtol * np.abs(b) + atol_frac * (np.abs(b).max() + 1e-300)
    ratio = np.abs(a - b) / bound
    i = int(ratio.argmax()) if ratio.size else 0
    return (float(ratio[i]) if ratio.size else 0.0), i


TOL = 1e-4  # north_star tolerance for floating-point outputs (relative to tensor max)


def assert_backward_parity(grads, g32, g64, *, well_conditioned=False, what=""):
    """The gradient rule of tests/test_gpu_parity.py::test_backward_parity.  grads: the HIP path's gradients by name; g32 / g64: the
    float32 / float64 oracle's backward on the same inputs.  Every figure is printed before it is asserted."""
    for name, g in grads.items():
        r = g64[name]
        assert r is not None, name
        floor = rel_err(g32[name], r)
        err = rel_err(g.reshape(r.shape), r)
        print(f"{what} grad {name}: rel err {err:.3e} (fp32 oracle floor {floor:.3e})")
        assert err <= max(TOL, 3.0 * floor), f"{what} grad {name}: rel err {err:.3e} (fp32 oracle floor {floor:.3e})"
        # element-wise: |a - b| <= 1e-4 |b| + 2e-5 max|b| on the well-conditioned scenes, where the float32
        # oracle itself meets that bound; elsewhere within 3x of the float32 oracle's own worst element
        ex, where = elem_excess(g.reshape(r.shape), r)
        ex32, _ = elem_excess(g32[name], r)
        print(f"{what} grad {name}: elem excess {ex:.3f} (fp32 oracle {ex32:.3f})")
        assert ex <= max(1.0, 3.0 * ex32), (f"{what} grad {name}: worst element {where} off by {ex:.2f}x the element-wise bound "
                                            f"(fp32 oracle: {ex32:.2f}x); hip {g.reshape(-1)[where]:.6e} ref {r.reshape(-1)[where]:.6e}")
        if well_conditioned:
            assert ex32 <= 1.0 and ex <= 1.0, f"{what} grad {name}: element-wise bound missed on a well-conditioned scene ({ex:.2f}x, fp32 oracle {ex32:.2f}x)"
        # every scene, the saturating / screen-filling ones included (r2 verdict: there the tensor-level bound is 8-1600x the
        # element bound, "no test would notice a 100x regression"): the DISTRIBUTION of the HIP path's element errors (in units of
        # the element bound, against the float64 oracle) must not be worse than 3x that of the float32 oracle -- at the median, at
        # the 99th and at the 99.9th percentile (floor: a tenth of the bound).  A single entry proves nothing on an ill-conditioned
        # scene (where float32 lands is luck); a broad loss of accuracy moves the quantiles.
        r64 = np.asarray(r, np.float64).reshape(-1); a64 = np.asarray(g, np.float64).reshape(-1); o32 = np.asarray(g32[name], np.float64).reshape(-1)
        bound = 1e-4 * np.abs(r64) + 2e-5 * (np.abs(r64).max() + 1e-300)
        rh, ro = np.abs(a64 - r64) / bound, np.abs(o32 - r64) / bound
        for q in (0.5, 0.99, 0.999):
            qh, qo = float(np.quantile(rh, q)), float(np.quantile(ro, q))
            print(f"{what} grad {name}: {q:.3f}-quantile of the element error {qh:.3f}x the bound (fp32 oracle {qo:.3f}x)")
            assert qh <= max(0.1, 3.0 * qo), f"{what} grad {name}: {q:.3f}-quantile of the element error is {qh:.3f}x the bound (float32 oracle: {qo:.3f}x)"
