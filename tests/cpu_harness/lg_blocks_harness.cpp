// CPU build of the product's block-sparse TSDF arithmetic (lightgaussian_amd/csrc/lg_math.h, the functions lg_blocks.h's kernels call), for
// tests/test_blocks_host.py and tests/test_gpu_blocks.py.  Compiled with -ffp-contract=off -mfma: the bits are the device's.
// The loops visit every pixel, block, point, edge slot and cell on their own, in the order of the contract; the
// sorted union the kernels take with a radix sort is a std::set here, the neighbour table a std::map, the prefix sums running counters.
#include <map>
#include <set>
#include <vector>

#include "../../lightgaussian_amd/csrc/lg_math.h"

// the halo of block b: values of `src` [n][512] through the neighbour ranks, `fill` for a missing block
template <typename T>
static void halo_of(int b, const int* nbr, const T* src, T fill, T* out)
{
    for (int h = 0; h < LG_BLK_HALO_POINTS; h++) {
        uint32_t m; int local;
        lg_blk_halo_source(h, m, local);
        const int r = nbr[8 * b + m];
        out[h] = r >= 0 ? src[(size_t)r * LG_BLK_POINTS + local] : fill;
    }
}

extern "C" {

// views as in lg_tsdf_harness.cpp: wh [n][2], cam [n][5] = (tanfovx, tanfovy, depth_max, z_min, alpha_min), vms [n][16], depth and alpha (or
// NULL) per view.  The keys the views touch, ascending, go to keys (room for `room`); pixels (or NULL) receives per pixel, views back to
// back, (status, lo x, lo y, lo z, n x, n y, n z).  stats = (touched keys, skipped pixels).  Returns the number of touched keys.
int64_t h_blocks_touch(const float* origin, float voxel, float trunc, int n_views, const int* wh, const float* cam, const float* vms, const float* const* depth,
                       const float* const* alpha, int64_t room, int64_t* keys, int32_t* pixels, int64_t* stats)
{
    std::set<int64_t> seen;
    int64_t skipped = 0;
    size_t at = 0;
    for (int v = 0; v < n_views; v++) {
        const LgTsdfCam c = { wh[2 * v], wh[2 * v + 1], cam[5 * v], cam[5 * v + 1], cam[5 * v + 2], cam[5 * v + 3], cam[5 * v + 4] };
        for (int iy = 0; iy < c.H; iy++)
            for (int ix = 0; ix < c.W; ix++, at++) {
                const size_t pix = (size_t)iy * c.W + ix;
                LgBlkBox box = { { 0, 0, 0 }, { 0, 0, 0 } };
                const int status = lg_blk_touch(vms + 16 * v, c, origin, voxel, trunc, ix, iy, depth[v][pix], alpha[v] != nullptr, alpha[v] ? alpha[v][pix] : 0.0f, box);
                if (pixels) {
                    int32_t* o = pixels + 7 * at;
                    o[0] = status;
                    for (int a = 0; a < 3; a++) { o[1 + a] = box.lo[a]; o[4 + a] = box.n[a]; }
                }
                if (status == 2) skipped++;
                if (status != 1) continue;
                for (int z = 0; z < box.n[2]; z++)
                    for (int y = 0; y < box.n[1]; y++)
                        for (int x = 0; x < box.n[0]; x++) seen.insert(lg_blk_key(box.lo[0] + x, box.lo[1] + y, box.lo[2] + z));
            }
    }
    int64_t k = 0;
    for (int64_t key : seen)
        if (k < room) keys[k++] = key; else k++;
    stats[0] = (int64_t)seen.size(); stats[1] = skipped;
    return (int64_t)seen.size();
}

// every point of every block under every view, in order; tsdf, weight [n][512], color [n][512][3] or NULL
void h_blocks_integrate(int n, const int64_t* keys, const float* origin, float voxel, float trunc, float* tsdf, float* weight, float* color, int n_views,
                        const int* wh, const float* cam, const float* vms, const float* const* depth, const float* const* image, const float* const* alpha)
{
    for (int b = 0; b < n; b++) {
        int bx, by, bz;
        lg_blk_coords(keys[b], bx, by, bz);
        for (int z = 0; z < LG_BLK; z++)
            for (int y = 0; y < LG_BLK; y++)
                for (int x = 0; x < LG_BLK; x++) {
                    const size_t p = (size_t)b * LG_BLK_POINTS + lg_blk_local(x, y, z);
                    const float px = lg_tsdf_coord(origin[0], voxel, bx * LG_BLK + x), py = lg_tsdf_coord(origin[1], voxel, by * LG_BLK + y),
                                pz = lg_tsdf_coord(origin[2], voxel, bz * LG_BLK + z);
                    for (int v = 0; v < n_views; v++) {
                        const LgTsdfCam c = { wh[2 * v], wh[2 * v + 1], cam[5 * v], cam[5 * v + 1], cam[5 * v + 2], cam[5 * v + 3], cam[5 * v + 4] };
                        lg_tsdf_update(vms + 16 * v, c, depth[v], color ? image[v] : nullptr, alpha[v], trunc, px, py, pz, tsdf[p], weight[p], color ? color + 3 * p : nullptr);
                    }
                }
    }
}

// counts = (vertices, faces); with vertices != NULL also the mesh: vertices [Nv,3], colors [Nv,3] or NULL, faces [Nf,3], cell_of_face [Nf] (or
// NULL) = rank 512 + local index of the cell, used [6][16] (or NULL) as in lg_tsdf_harness.cpp; nbr_out [n][8] (or NULL): the neighbour table.
void h_blocks_mesh(int n, const int64_t* keys, const float* origin, float voxel, const float* tsdf, const float* weight, const float* color, float iso,
                   float min_weight, int64_t* counts, float* vertices, float* colors, int32_t* faces, int64_t* cell_of_face, int64_t* used, int32_t* nbr_out)
{
    std::map<int64_t, int> rank;
    for (int b = 0; b < n; b++) rank[keys[b]] = b;
    std::vector<int> nbr((size_t)n * 8 + 1);
    for (int b = 0; b < n; b++) {
        int bx, by, bz;
        lg_blk_coords(keys[b], bx, by, bz);
        for (int m = 0; m < 8; m++) {
            const int x = bx + (m & 1), y = by + ((m >> 1) & 1), z = bz + ((m >> 2) & 1);
            int r = -1;
            if (x < LG_BLK_BIAS && y < LG_BLK_BIAS && z < LG_BLK_BIAS) {
                auto it = rank.find(lg_blk_key(x, y, z));
                if (it != rank.end()) r = it->second;
            }
            nbr[8 * b + m] = r;
            if (nbr_out) nbr_out[8 * b + m] = r;
        }
    }
    const size_t P = (size_t)n * LG_BLK_POINTS;
    std::vector<uint32_t> vprefix(P + 1);
    std::vector<uint8_t> vmask(P + 1);
    float ht[LG_BLK_HALO_POINTS], hw[LG_BLK_HALO_POINTS];
    uint32_t nv = 0;
    int64_t nf = 0;
    for (int b = 0; b < n; b++) {
        halo_of<float>(b, nbr.data(), tsdf, 1.0f, ht);
        halo_of<float>(b, nbr.data(), weight, 0.0f, hw);
        int bx, by, bz;
        lg_blk_coords(keys[b], bx, by, bz);
        for (int z = 0; z < LG_BLK; z++)
            for (int y = 0; y < LG_BLK; y++)
                for (int x = 0; x < LG_BLK; x++) {
                    const size_t p = (size_t)b * LG_BLK_POINTS + lg_blk_local(x, y, z);
                    const uint32_t m = lg_mesh_edge_mask(ht, hw, LG_BLK_HALO, LG_BLK_HALO, LG_BLK_HALO, x, y, z, iso, min_weight);
                    vprefix[p] = nv; vmask[p] = (uint8_t)m;
                    for (uint32_t k = 0; k < LG_MESH_SLOTS; k++)
                        if ((m >> k) & 1u) {
                            if (vertices) {
                                const uint32_t sm = lg_mesh_slot_mask(k);
                                const int h1 = lg_blk_halo_index(x + (int)(sm & 1u), y + (int)((sm >> 1) & 1u), z + (int)((sm >> 2) & 1u));
                                uint32_t qm; int ql;
                                lg_blk_halo_source(h1, qm, ql);
                                const float* c0 = (color && colors) ? color + 3 * p : nullptr;
                                const float* c1 = c0 ? color + 3 * ((size_t)nbr[8 * b + qm] * LG_BLK_POINTS + ql) : nullptr;
                                lg_blk_vertex(ht[lg_blk_halo_index(x, y, z)], ht[h1], c0, c1, bx * LG_BLK + x, by * LG_BLK + y, bz * LG_BLK + z, k, iso, origin, voxel,
                                              vertices + 3 * (size_t)nv, colors ? colors + 3 * (size_t)nv : nullptr);
                            }
                            nv++;
                        }
                    uint32_t inside8;
                    if (lg_mesh_cell_corners(ht, hw, LG_BLK_HALO, LG_BLK_HALO, x, y, z, iso, min_weight, inside8)) nf += lg_mesh_cell_count(inside8);
                }
    }
    counts[0] = nv; counts[1] = nf;
    if (!vertices) return;
    uint32_t hp[LG_BLK_HALO_POINTS];
    uint8_t hm[LG_BLK_HALO_POINTS];
    size_t f = 0;
    for (int b = 0; b < n; b++) {
        halo_of<float>(b, nbr.data(), tsdf, 1.0f, ht);
        halo_of<float>(b, nbr.data(), weight, 0.0f, hw);
        halo_of<uint32_t>(b, nbr.data(), vprefix.data(), 0u, hp);
        halo_of<uint8_t>(b, nbr.data(), vmask.data(), (uint8_t)0, hm);
        for (int z = 0; z < LG_BLK; z++)
            for (int y = 0; y < LG_BLK; y++)
                for (int x = 0; x < LG_BLK; x++) {
                    uint32_t inside8;
                    if (!lg_mesh_cell_corners(ht, hw, LG_BLK_HALO, LG_BLK_HALO, x, y, z, iso, min_weight, inside8)) continue;
                    if (used)
                        for (uint32_t t = 0; t < 6u; t++) used[16 * t + lg_mesh_tet_inside(t, inside8)]++;
                    const uint32_t k = lg_mesh_cell_faces(LG_BLK_HALO, LG_BLK_HALO, x, y, z, inside8, hp, hm, faces + 3 * f, 12);
                    if (cell_of_face)
                        for (uint32_t j = 0; j < k; j++) cell_of_face[f + j] = (int64_t)b * LG_BLK_POINTS + lg_blk_local(x, y, z);
                    f += k;
                }
    }
}

}
