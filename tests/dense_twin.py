"""The dense autograd twin (oracle/torch_dense.py::render_dense) as the tests call it (test infrastructure): the one place that spells
out its keywords, the keep mask, and the cached float64 / float32 gradient loop.

The twin is O(pixels x Gaussians): it is handed only the Gaussians in front of z_view = 0.19 (a superset of what the 0.2 near plane
lets through, by the float32 view transform; the others take no part in the image or in any gradient)."""
import numpy as np
import torch

from oracle import torch_dense

PER_GAUSSIAN = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")
CAMERA = ("viewmatrix", "projmatrix", "campos")
DTYPES = ((torch.float64, "float64"), (torch.float32, "float32"))


def front(kw):
    """[N] bool: in front of z_view = 0.19 by the float32 view transform."""
    vm32 = kw["viewmatrix"].float()
    return (kw["means3D"].float() @ vm32[:3, 2] + vm32[3, 2]) > 0.19


def leaves(kw, dd, grad=True):
    """kw's per-Gaussian tensors in dtype dd, as fresh leaves."""
    return {k: kw[k].to(dd).detach().clone().requires_grad_(grad) for k in PER_GAUSSIAN if k in kw}


def render(kw, dd, *, leaves=None, camera=None, means2D=None, antialias=False, front_only=True):
    """render_dense in dtype dd of kw (scene kwargs, CPU torch tensors).  leaves: {name: [N, .] tensor of dtype dd} in place of kw's
    per-Gaussian tensors; camera: (viewmatrix, projmatrix, campos) of dtype dd in place of kw's; means2D: [N, 3] (default zeros);
    antialias: opacities = sigma rho, rho of antialias_common from the same tensors and view matrix; front_only=False: all N Gaussians
    go to the twin.  Returns (color [3,H,W], radii [N], count [N]), radii and count zero for the Gaussians left out."""
    N = kw["means3D"].shape[0]
    keep = front(kw) if front_only else torch.ones(N, dtype=torch.bool)
    t = {k: kw[k].to(dd) for k in PER_GAUSSIAN if k in kw}
    t.update(leaves or {})
    vm, pm, cp = camera if camera is not None else (kw[n].to(dd) for n in CAMERA)
    if antialias:
        import antialias_common
        t["opacities"] = antialias_common.compensated_opacities(t, vm, kw)
    m2 = torch.zeros(N, 3, dtype=dd) if means2D is None else means2D
    color, rad, cnt = torch_dense.render_dense(means2D=m2[keep], W=kw["W"], H=kw["H"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"],
                                               bg=kw["bg"].to(dd), viewmatrix=vm, projmatrix=pm, campos=cp, sh_degree=kw["sh_degree"],
                                               **{k: v[keep] for k, v in t.items()})
    radii, count = torch.zeros(N, dtype=rad.dtype), torch.zeros(N, dtype=cnt.dtype)
    radii[keep], count[keep] = rad, cnt
    return color, radii, count


_REF = {}


def gradients(key, kw, gimg, *, camera=False, antialias=False, per_gaussian=True):
    """{"float64": {tensor name: gradient}, "float32": {...}} (numpy float64 arrays) of sum(image * gimg) by the twin, with respect to the
    per-Gaussian inputs of kw (per_gaussian) and to viewmatrix / projmatrix / campos (camera; zeros where autograd hands none back).
    key: anything hashable naming (scene, combination, image gradient).  Computed once per (key, switches)."""
    key = (key, camera, antialias, per_gaussian)
    if key in _REF:
        return _REF[key]
    out = {}
    for dd, name in DTYPES:
        lv = leaves(kw, dd) if per_gaussian else {}
        cam = tuple(kw[n].to(dd).detach().clone().requires_grad_() for n in CAMERA) if camera else None
        (render(kw, dd, leaves=lv, camera=cam, antialias=antialias)[0] * gimg.to(dd)).sum().backward()
        out[name] = {k: v.grad.numpy().astype(np.float64) for k, v in lv.items()}
        if camera:
            out[name].update({n: (np.zeros(tuple(c.shape)) if c.grad is None else c.grad.numpy().astype(np.float64)) for n, c in zip(CAMERA, cam)})
    _REF[key] = out
    return out
