"""A camera whose pose is a trainable correction of a base camera: what render(..., options={"camera_grad": True}) differentiates into.

    cam = PoseCamera(base_camera).to(device)
    opt = torch.optim.Adam(cam.parameters(), lr=1e-3)
    loss = l1_loss(render(cam, gaussians, pipe, bg, options={"camera_grad": True})["render"], target)
    loss.backward(); opt.step()

The library's matrices are row-vector ones (scene/cameras.py:70-85: world_view_transform = getWorld2View2(R, T).transpose(0, 1),
p_view = [p, 1] @ world_view_transform).  With Delta = exp(xi^) in SE(3) acting on view-space COLUMN vectors, p_view' = Delta p_view,
the corrected row-vector matrix is  world_view_transform = base @ Delta^T.
"""
import torch
import torch.nn as nn


def se3_generator(xi):
    """xi = (omega, tau) [6] -> the 4 x 4 generator [[omega^, tau], [0, 0]] (column-vector convention)."""
    z = xi.new_zeros(())
    wx, wy, wz, tx, ty, tz = xi.unbind(0)
    return torch.stack([torch.stack([z, -wz, wy, tx]), torch.stack([wz, z, -wx, ty]), torch.stack([-wy, wx, z, tz]),
                        torch.stack([z, z, z, z])])


def pose_matrices(xi, base_wvt, proj):
    """(world_view_transform, full_proj_transform, camera_center) of the base view matrix corrected by xi; differentiable in xi."""
    delta = torch.matrix_exp(se3_generator(xi))
    wvt = base_wvt @ delta.transpose(0, 1)
    return wvt, wvt @ proj, torch.linalg.inv(wvt)[3, :3]


class PoseCamera(nn.Module):
    """base_camera with a trainable se(3) correction `xi` (rotation vector omega, translation tau; zero-initialised: at zero the three
    matrices equal the base camera's).  Same attribute surface as the cameras render() reads: image_width, image_height, FoVx, FoVy,
    world_view_transform, full_proj_transform, camera_center -- the last three are computed from `xi` on access, under autograd.
    The projection P is recovered once from the base camera (its projection_matrix attribute when it has one, else
    inverse(world_view_transform) @ full_proj_transform)."""

    def __init__(self, base_camera):
        super().__init__()
        wvt = base_camera.world_view_transform.detach().to(torch.float32)
        self.register_buffer("base_world_view_transform", wvt.clone())
        proj = getattr(base_camera, "projection_matrix", None)
        if proj is None:
            proj = torch.linalg.inv(wvt.double()) @ base_camera.full_proj_transform.detach().to(wvt.device).double()
        self.register_buffer("projection_matrix", proj.detach().to(device=wvt.device, dtype=torch.float32).clone())
        self.xi = nn.Parameter(torch.zeros(6, dtype=torch.float32, device=wvt.device))
        self.image_width, self.image_height = int(base_camera.image_width), int(base_camera.image_height)
        self.FoVx, self.FoVy = float(base_camera.FoVx), float(base_camera.FoVy)
        self.znear, self.zfar = getattr(base_camera, "znear", 0.01), getattr(base_camera, "zfar", 100.0)

    def matrices(self):
        return pose_matrices(self.xi, self.base_world_view_transform, self.projection_matrix)

    @property
    def world_view_transform(self):
        return self.matrices()[0]

    @property
    def full_proj_transform(self):
        return self.matrices()[1]

    @property
    def camera_center(self):
        return self.matrices()[2]
