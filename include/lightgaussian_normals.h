/* lightgaussian_normals.h -- extension of the C ABI of liblightgaussian_hip.so (include/lightgaussian.h, same LG_ABI_VERSION): normals
 * of the Gaussians, normals of a rendered depth map, and the fused depth-normal consistency loss (2DGS, GOF, PGSR, RaDe-GS) for float32
 * device tensors.  Error codes, lg_last_error(), LG_FLAG_PROFILE and the stream argument are lightgaussian.h's.  DESIGN.md section
 * 10.11 holds the contract and its reasons; lightgaussian_amd/csrc/lg_math.h writes every operation out in order.
 *
 * --- per Gaussian and view: lg_normal_rows / lg_normal_rows_bwd, ONE launch each, no read-back ------------------------------
 * Inputs: xyz [N,3], scaling [N,3], rotation [N,4] as (r, x, y, z), viewmatrix = world_view_transform, 16 floats ON THE DEVICE, used as
 * lg_view.viewmatrix is: p_v[c] = sum_a xyz[a] vm[4 a + c] + vm[12 + c].  rows [N,4] = (view-space normal, view-space z):
 *     q^ = q / max(|q|, 1e-12)          the forward's own normalisation of raw rotations (F.normalize); a zero quaternion gives q^ = 0,
 *                                       R = identity; a non-finite one gives a non-finite row -- as the forward treats them
 *     k = argmin_k scaling[k]           ties to the lowest index.  Raw log-scales, activated scales and 3D-filtered scales have the same
 *                                       argmin, so any of them may be passed; no filter and no scale modifier enters
 *     n_w = column k of R(q^)           n_v[c] = sum_a n_w[a] vm[4 a + c]
 *     s = -1 when n_v . p_v > 0, else +1       the normal faces the camera; an exactly perpendicular one keeps its sign
 *     rows = (s n_v, p_v.z)
 * lg_normal_rows_bwd takes dL_drows [N,4]:  dL_dxyz[a] = g[3] vm[4 a + 2];  dL_drotation through column k of R(q / |q|) including the
 * normalisation, k and s held constant; scaling receives nothing (it has no argument for it).
 * N == 0 is LG_OK without a launch.  N < 2^30.  A tensor set in which every pointer is 16-byte aligned moves whole 16-byte words.
 *
 * --- per pixel: lg_depth_normals / lg_depth_normals_bwd -----------------------------------------------------------------------
 * depth [H,W] -> normals [3,H,W], 2DGS's depth_to_normal with the rasterizer's pixel centres:
 *     P(x, y) = depth(x, y) (((2 x + 1) / W - 1) tanfovx, ((2 y + 1) / H - 1) tanfovy, 1)
 *     c = (P(x, y + 1) - P(x, y - 1)) x (P(x + 1, y) - P(x - 1, y))          N_d = c / max(|c|, 1e-12)
 * A fronto-parallel plane gives (0, 0, -1).  Pixels of the first and last row and column are zero, and so is a pixel whose c or whose own
 * depth is not finite; both kinds pass no gradient.  lg_depth_normals_bwd: dL_dnormals [3,H,W] -> dL_ddepth [H,W], every pixel written.
 *
 * --- the consistency loss: lg_normal_loss / lg_normal_loss_bwd ----------------------------------------------------------------
 *     loss[0] = (1 / (H W)) sum_p (1 - w_p N_r(p) . N_d(p))          w = alpha, or alpha * weight when weight is not NULL
 * normal_map = N_r [3,H,W], the blended unnormalised normals; alpha, weight [H,W] are constants of the loss.  depth_normals (may be
 * NULL) receives N_d.  scratch: lg_normal_loss_scratch_bytes(H, W) bytes, 4-byte aligned, one partial sum per wave; sums run in a fixed
 * order (no float atomics, no memset): bit-identical from run to run and across streams.  lg_normal_loss_bwd reads the upstream scalar
 * dL_dloss[0] from DEVICE memory and writes dL_dnormal_map = -g w N_d / (H W) [3,H,W] and dL_ddepth [H,W] (through N_d); it needs no
 * state of the forward.
 * flags: LG_FLAG_PROFILE records "normal_rows", "normal_rows_bwd", "depth_normals", "depth_normals_bwd", "normal_loss",
 * "normal_loss_reduce", "normal_loss_bwd", one entry per launch.
 * LG_ERR_INVALID_ARGUMENT, before any device call, the message naming the argument: N outside [0, 2^30); H or W outside [1, 32768]; a
 * null pointer (weight and depth_normals excepted); a pointer off 4 bytes; a NaN tanfovx / tanfovy. */
#ifndef LIGHTGAUSSIAN_NORMALS_H
#define LIGHTGAUSSIAN_NORMALS_H

#include "lightgaussian.h"

#ifdef __cplusplus
extern "C" {
#endif

int lg_normal_rows(int32_t N, const float* xyz, const float* scaling, const float* rotation, const float* viewmatrix, float* rows,
                   uint32_t flags, void* stream);
int lg_normal_rows_bwd(int32_t N, const float* xyz, const float* scaling, const float* rotation, const float* viewmatrix,
                       const float* dL_drows, float* dL_dxyz, float* dL_drotation, uint32_t flags, void* stream);
int lg_depth_normals(int32_t H, int32_t W, const float* depth, float tanfovx, float tanfovy, float* normals, uint32_t flags, void* stream);
int lg_depth_normals_bwd(int32_t H, int32_t W, const float* depth, float tanfovx, float tanfovy, const float* dL_dnormals,
                         float* dL_ddepth, uint32_t flags, void* stream);
size_t lg_normal_loss_scratch_bytes(int32_t H, int32_t W);
int lg_normal_loss(int32_t H, int32_t W, const float* normal_map, const float* depth, const float* alpha, const float* weight,
                   float tanfovx, float tanfovy, float* loss, float* depth_normals, void* scratch, uint32_t flags, void* stream);
int lg_normal_loss_bwd(int32_t H, int32_t W, const float* normal_map, const float* depth, const float* alpha, const float* weight,
                       float tanfovx, float tanfovy, const float* dL_dloss, float* dL_dnormal_map, float* dL_ddepth, uint32_t flags,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGAUSSIAN_NORMALS_H */
