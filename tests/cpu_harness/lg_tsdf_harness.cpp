// CPU build of the product's TSDF and marching-tetrahedra arithmetic (lightgaussian_amd/csrc/lg_math.h, the functions lg_tsdf.h's kernels
// call), for tests/test_mesh_host.py and tests/test_gpu_mesh.py.  Compiled with -ffp-contract=off -mfma: the bits are the device's.
// The loops visit every point, edge slot and cell on their own, in the order of the contract; the prefix sums
// the kernels take with scans are running counters here.
#include <vector>

#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

// views: wh [n][2] = (W, H), cam [n][5] = (tanfovx, tanfovy, depth_max, z_min, alpha_min), vms [n][16], and per view the pointers of depth
// [H,W], color [3,H,W] or NULL, alpha [H,W] or NULL.  decided [n][P] (or NULL): 1 where the view updated the point.
void h_tsdf_integrate(int nx, int ny, int nz, const float* origin, float voxel, float trunc, float* tsdf, float* weight, float* color, int n_views,
                      const int* wh, const float* cam, const float* vms, const float* const* depth, const float* const* image, const float* const* alpha,
                      uint8_t* decided)
{
    const size_t P = (size_t)nx * ny * nz;
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++) {
                const size_t p = lg_mesh_index(nx, ny, x, y, z);
                const float px = lg_tsdf_coord(origin[0], voxel, x), py = lg_tsdf_coord(origin[1], voxel, y), pz = lg_tsdf_coord(origin[2], voxel, z);
                for (int v = 0; v < n_views; v++) {
                    const LgTsdfCam c = { wh[2 * v], wh[2 * v + 1], cam[5 * v], cam[5 * v + 1], cam[5 * v + 2], cam[5 * v + 3], cam[5 * v + 4] };
                    const bool hit = lg_tsdf_update(vms + 16 * v, c, depth[v], color ? image[v] : nullptr, alpha[v], trunc, px, py, pz, tsdf[p], weight[p],
                                                    color ? color + 3 * p : nullptr);
                    if (decided) decided[(size_t)v * P + p] = hit ? 1 : 0;
                }
            }
}

// counts[0] = vertices, counts[1] = faces
void h_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float iso, float min_weight, int64_t* counts)
{
    counts[0] = counts[1] = 0;
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++) {
                counts[0] += lg_mesh_popc8(lg_mesh_edge_mask(tsdf, weight, nx, ny, nz, x, y, z, iso, min_weight));
                uint32_t inside8;
                if (x < nx - 1 && y < ny - 1 && z < nz - 1 && lg_mesh_cell_corners(tsdf, weight, nx, ny, x, y, z, iso, min_weight, inside8))
                    counts[1] += lg_mesh_cell_count(inside8);
            }
}

// vertices [Nv,3], colors [Nv,3] or NULL, faces [Nf,3], cell_of_face [Nf] (or NULL): the linear index of the cell a face came from;
// used [6][16] (or NULL): how many valid cells met the table entry (tetrahedron, inside mask).  The counts are h_mesh_count's.
void h_mesh_extract(int nx, int ny, int nz, const float* origin, float voxel, const float* tsdf, const float* weight, const float* color, float iso,
                    float min_weight, float* vertices, float* colors, int32_t* faces, int64_t* cell_of_face, int64_t* used)
{
    const size_t P = (size_t)nx * ny * nz;
    std::vector<uint32_t> vprefix(P);
    std::vector<uint8_t> vmask(P);
    uint32_t nv = 0;
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++) {
                const size_t p = lg_mesh_index(nx, ny, x, y, z);
                const uint32_t m = lg_mesh_edge_mask(tsdf, weight, nx, ny, nz, x, y, z, iso, min_weight);
                vprefix[p] = nv; vmask[p] = (uint8_t)m;
                for (uint32_t k = 0; k < LG_MESH_SLOTS; k++)
                    if ((m >> k) & 1u) {
                        lg_mesh_vertex(tsdf, color, nx, ny, x, y, z, k, iso, origin, voxel, vertices + 3 * (size_t)nv, colors ? colors + 3 * (size_t)nv : nullptr);
                        nv++;
                    }
            }
    size_t nf = 0;
    for (int z = 0; z < nz - 1; z++)
        for (int y = 0; y < ny - 1; y++)
            for (int x = 0; x < nx - 1; x++) {
                uint32_t inside8;
                if (!lg_mesh_cell_corners(tsdf, weight, nx, ny, x, y, z, iso, min_weight, inside8)) continue;
                if (used)
                    for (uint32_t t = 0; t < 6u; t++) used[16 * t + lg_mesh_tet_inside(t, inside8)]++;
                const uint32_t n = lg_mesh_cell_faces(nx, ny, x, y, z, inside8, vprefix.data(), vmask.data(), faces + 3 * nf, 12);
                if (cell_of_face)
                    for (uint32_t j = 0; j < n; j++) cell_of_face[nf + j] = (int64_t)lg_mesh_index(nx, ny, x, y, z);
                nf += n;
            }
}

}
