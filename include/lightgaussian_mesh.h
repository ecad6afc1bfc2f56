/* lightgaussian_mesh.h -- extension of the C ABI of liblightgaussian_hip.so (include/lightgaussian.h, same LG_ABI_VERSION): fusion of
 * rendered depth maps into a truncated signed distance volume (TSDF) and extraction of a triangle mesh from it by marching tetrahedra,
 * the surface 2DGS, GOF, PGSR and RaDe-GS publish.  Error codes, lg_last_error(), LG_FLAG_PROFILE and the stream argument are
 * lightgaussian.h's.  DESIGN.md section 10.13 holds the contract and its reasons; lightgaussian_amd/csrc/lg_math.h writes every
 * operation out in order.  All tensors are float32 device memory unless said otherwise.
 *
 * --- the volume: lg_tsdf_volume ----------------------------------------------------------------------------------------------
 * nx x ny x nz points; point (x, y, z) lies at origin + voxel_size (x, y, z) in world space.  Storage is x-fastest: tsdf [nz,ny,nx]
 * (initial value 1), weight [nz,ny,nx] (initial value 0), color [nz,ny,nx,3] or NULL (no colour is kept).  trunc > 0 is the truncation
 * distance in world units.  Every dimension >= 1 and nx ny nz < 2^29.
 *
 * --- lg_tsdf_integrate: n views into the volume, in view order ------------------------------------------------------------------
 * views is a HOST array of n_views lg_tsdf_view holding device pointers: viewmatrix = world_view_transform, 16 floats ON THE DEVICE,
 * used as lg_view.viewmatrix is (p_v[c] = sum_a p[a] vm[4 a + c] + vm[12 + c]); depth [H,W] = view-space z, 0 = nothing there; color
 * [3,H,W] (required when the volume keeps colour, ignored otherwise); alpha [H,W] or NULL with alpha_min; depth_max (0: none); z_min.
 * One point under one view, in float32:
 *     p_v = point vm                                      skip when !(p_v.z > z_min)
 *     fx = (p_v.x / (p_v.z tanfovx) + 1) (0.5 W)          px = floor(fx)        (fy, py likewise with tanfovy, H)
 *                                                         skip when px is outside [0, W) or py outside [0, H)
 *     d = depth[py, px]                                   skip when !(d > 0), d is not finite, depth_max > 0 and d > depth_max, or alpha
 *                                                         is given and alpha[py, px] < alpha_min
 *     sdf = d - p_v.z                                     skip when sdf < -trunc
 *     t = min(1, sdf / trunc)        w' = w + 1        tsdf = (tsdf w + t) / w'        color_c = (color_c w + image_c[py, px]) / w'
 *     weight = w'
 * (px, py) is the pixel that contains the projection, with the rasterizer's pixel centres.  A skipped point keeps its three values bit
 * for bit.  The library splits the views into launches of 8; one call with n views gives the bits of n calls with one view each.
 * n_views == 0 is LG_OK without a launch.
 *
 * --- lg_mesh_count / lg_mesh_emit: marching tetrahedra with indexed vertices -------------------------------------------------------
 * Axis bits x = 1, y = 2, z = 4.  A point is observed when weight >= min_weight and inside when tsdf < iso.
 *     edge slots   point p owns the seven edges to p + offset(m), m = 1, 2, 4, 3, 5, 6, 7 (slot k = 0 .. 6), that stay inside the grid
 *     vertices     an edge carries a vertex iff both ends are observed and exactly one is inside: at p0 + t (p1 - p0), t = f0 / (f0 - f1),
 *                  f = tsdf - iso, mapped to world space; its colour is the same interpolation of the colour volume.  Vertex ids count
 *                  the carrying edges in order of (point linear index, slot)
 *     cells        the cube at p < (nx - 1, ny - 1, nz - 1); valid when its eight corners are observed
 *     tetrahedra   six per cell, one per permutation (a, b, c) of the axes in lexicographic order, with the local corners 0, 1<<a,
 *                  1<<a | 1<<b, 7; the edge between local corners i < j is the slot of mask_j ^ mask_i at the point of corner i
 *     triangles    by the inside mask of the four local corners: one corner apart: the edges from it to the other three in ascending
 *                  order; two and two (a < b inside, c < d outside): the quad (a,c), (a,d), (b,d), (b,c) as (q0,q1,q2), (q0,q2,q3); wound
 *                  so that the normals point toward larger tsdf (free space)
 *     faces        ordered by valid cell in linear order, then tetrahedron, then triangle
 * lg_mesh_count leaves the number of vertices and faces in counts (DEVICE int64[2]) and, in scratch (lg_mesh_scratch_bytes(nx, ny, nz)
 * bytes, 256-byte aligned), what lg_mesh_emit needs; the caller reads counts, allocates vertices [Nv,3], colors [Nv,3] (or NULL) and faces
 * [Nf,3] (int32) and calls lg_mesh_emit with the same volume, iso and min_weight.  lg_mesh_emit waits for the stream, holds n_vertices and
 * n_faces against the counts in scratch (LG_ERR_INVALID_ARGUMENT when they differ, or are 2^31 or more) and writes every element of the
 * outputs with plain stores.  Values and order are deterministic.  A grid thinner than two points along an axis has no faces.
 * flags: LG_FLAG_PROFILE records "tsdf_integrate" (per launch), "mesh_count", "mesh_scan", "mesh_emit".
 * LG_ERR_INVALID_ARGUMENT, before any device call, the message naming the argument: a null pointer (volume->color, view color / alpha
 * and colors excepted) or one off 4 bytes (counts: 8); a dimension < 1 or nx ny nz >= 2^29; trunc, voxel_size or min_weight not positive
 * and finite; a non-finite origin or iso; a NaN tanfovx / tanfovy, z_min, depth_max or alpha_min; W or H outside [1, 32768]; n_views < 0;
 * a view without color for a volume that keeps colour; colors for a volume that keeps none. */
#ifndef LIGHTGAUSSIAN_MESH_H
#define LIGHTGAUSSIAN_MESH_H

#include "lightgaussian.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_tsdf_volume {
    int32_t nx, ny, nz;
    float origin[3];
    float voxel_size;
    float trunc;
    float* tsdf;
    float* weight;
    float* color;
} lg_tsdf_volume;

typedef struct lg_tsdf_view {
    int32_t W, H;
    float tanfovx, tanfovy;
    const float* viewmatrix;
    const float* depth;
    const float* color;
    const float* alpha;
    float alpha_min;
    float depth_max;
    float z_min;
} lg_tsdf_view;

int lg_tsdf_integrate(const lg_tsdf_volume* volume, int32_t n_views, const lg_tsdf_view* views, uint32_t flags, void* stream);
size_t lg_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int lg_mesh_count(const lg_tsdf_volume* volume, float iso, float min_weight, void* scratch, int64_t* counts, uint32_t flags, void* stream);
int lg_mesh_emit(const lg_tsdf_volume* volume, float iso, float min_weight, void* scratch, int64_t n_vertices, int64_t n_faces, float* vertices,
                 float* colors, int32_t* faces, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGAUSSIAN_MESH_H */
