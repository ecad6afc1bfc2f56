// lg_blocks.h -- a block-sparse TSDF volume for unbounded scenes: allocation of 8 x 8 x 8 blocks from depth maps, integration and
// marching tetrahedra across block borders (include/lightgaussian_blocks.h).  The blocks are kept in sorted-key
// order: no hash table, no atomics, no memset; every result is bit-identical from run to run and independent of allocation history.
//
//   lg_blk_touch_kernel <EMIT>   one lane per pixel, one wave per tile of 8 x 8 pixels, up to 8 views per launch.  lg_blk_touch gives a lane
//                                its box of at most 4 x 4 x 4 blocks; the wave then removes equal keys among its lanes before anything
//                                reaches memory: the first lane with blocks left names its lowest one, every lane that holds that block
//                                strikes it from its 64-bit to-do mask, one turn per distinct key.  EMIT = false counts the turns (and the
//                                skipped pixels) per wave; after lg_mesh_scan_kernel over the waves EMIT = true takes the same turns and
//                                lane 0 stores the key of turn j at prefix + j
//   lg_blk_pad_kernel            -1 into the candidates past the ones emitted: lg_blocks_merge drops negative keys
//   lg_blk_concat_kernel         old keys and added keys side by side, then lg_sort_keys on all 64 bits (a negative key sorts last)
//   lg_blk_unique_kernel <EMIT>  count / scan / emit of the keys that differ from their predecessor: the new key list
//   lg_blk_regrid_kernel         one workgroup per NEW block: binary search of its key among the old ones, then 16-byte loads and stores
//                                of the old values, or of the fresh ones; every element of the new pool is written
//   lg_blk_nbr_kernel            nbr [n,8]: the rank of the block at + offset(m), or -1 (binary search)
//   lg_blk_integrate_kernel <COLOR>  one workgroup of two waves per block; a lane carries lg_tsdf.h's run of four x-consecutive points
//                                (LgTsdfRun; rows of 32 contiguous bytes, always the dwordx4 path) in registers through up to 8 views
//                                (lg_tsdf_fetch, lg_tsdf_apply_view), loads once and stores once, and stores nothing for an untouched
//                                run; a view whose z_min plane the whole block lies behind is skipped by the workgroup
//   lg_blk_mesh_count_kernel     one workgroup per block: the 9 x 9 x 9 halo of tsdf and weight staged in LDS through nbr (5.8 KB), lg_math.h's
//                                rule functions on it as on a dense 9^3 grid, per-point edge-mask and face-count bytes, per-block totals
//                                (lg_mesh_put_totals)
//   lg_mesh_scan_kernel (lg_tsdf.h) over the block totals, then lg_mesh_prefix_kernel<2, true> (lg_tsdf.h): per point both exclusive prefixes
//   lg_blk_mesh_emit_kernel      the halo again, with the halo of vprefix and vmask: vertices at prefix + rank (lg_mesh_put_vertex), faces at
//                                the cell's face prefix with the vertex ids of the neighbour blocks' points read from the halo: plain stores
// Every rank read from nbr or found by a search is held against n before it indexes a pool.
// What this volume has in common with the dense one -- the lattice struct, a lane's run, one view applied to a run, the scratch of the
// mesh calls, the scan tails, the prefix kernel, the vertex store -- lives in lg_tsdf.h; this header holds what the blocks add.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "../../include/lightgaussian_blocks.h"
#include "lg_host.h"
#include "lg_wave.h"
#include "lg_tsdf.h"

#define LG_BLK_MAX_BLOCKS (1 << 20)         // n 512 < 2^29
#define LG_BLK_TOUCH_TILE 8                 // a wave covers 8 x 8 pixels
#define LG_BLK_TOUCH_MAX_PIXELS (1ll << 26) // per lg_blocks_touch call: at most 64 keys per pixel count in 32 bits
#define LG_BLK_THREADS 128                  // integrate, regrid: one run of four points per lane
#define LG_BLK_MESH_THREADS 256             // mesh kernels: two points per lane

struct LgBlkTouchView { const float* vm; const float* depth; const float* alpha; LgTsdfCam cam; uint32_t wave_end, tiles_x; };
struct LgBlkTouchBatch { LgBlkTouchView v[LG_TSDF_BATCH]; };

static inline uint32_t lg_blk_touch_waves(int W, int H)
{
    return (uint32_t)((W + LG_BLK_TOUCH_TILE - 1) / LG_BLK_TOUCH_TILE) * (uint32_t)((H + LG_BLK_TOUCH_TILE - 1) / LG_BLK_TOUCH_TILE);
}

// rank of `key` among keys [n] (strictly ascending), or -1
__device__ __forceinline__ int lg_blk_find(const int64_t* __restrict__ keys, int n, int64_t key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (int)(((uint32_t)lo + (uint32_t)hi) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < n && keys[lo] == key) ? lo : -1;
}

// wave_n [2][total_waves]: channel 0 the candidates of a wave (EMIT: their exclusive prefix), channel 1 its skipped pixels
template <bool EMIT>
__global__ void __launch_bounds__(256)
lg_blk_touch_kernel(LgTsdfLattice g, int n_views, LgBlkTouchBatch b, uint32_t batch_waves, uint32_t wave_base, uint32_t total_waves, uint32_t* __restrict__ wave_n,
                    int64_t capacity, int64_t* __restrict__ cand)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= batch_waves) return;
    int v = 0;
    while (v < n_views - 1 && w >= b.v[v].wave_end) v++;
    const LgBlkTouchView& a = b.v[v];
    const uint32_t tile = w - (v ? b.v[v - 1].wave_end : 0u);
    const int ix = (int)((tile % a.tiles_x) * LG_BLK_TOUCH_TILE + (lane & 7u)), iy = (int)((tile / a.tiles_x) * LG_BLK_TOUCH_TILE + (lane >> 3));
    const bool inside = ix < a.cam.W && iy < a.cam.H;
    const size_t pix = inside ? (size_t)iy * (size_t)a.cam.W + (size_t)ix : 0;
    const float d = inside ? a.depth[pix] : 0.0f;
    const float alpha = (inside && a.alpha) ? a.alpha[pix] : 0.0f;
    float vm[16];
    lg_tsdf_view_matrix(a.vm, vm);
    LgBlkBox box = { { 0, 0, 0 }, { 0, 0, 0 } };
    const int status = inside ? lg_blk_touch(vm, a.cam, g.o, g.voxel, g.trunc, ix, iy, d, a.alpha != nullptr, alpha, box) : 0;
    // bit (dz 4 + dy) 4 + dx of the to-do mask: block lo + (dx, dy, dz) of the lane's box
    uint64_t todo = 0;
    if (status == 1) {
        const uint64_t row = (1ull << box.n[0]) - 1ull;
        uint64_t plane = 0;
        for (int y = 0; y < box.n[1]; y++) plane |= row << (4 * y);
        for (int z = 0; z < box.n[2]; z++) todo |= plane << (16 * z);
    }
    const size_t slot = (size_t)wave_base + w;
    const int64_t base = EMIT ? (int64_t)wave_n[slot] : 0;
    uint32_t count = 0;
    uint64_t active = __ballot(todo != 0);
    while (active) {
        const int leader = __builtin_ctzll(active);
        const int bit = todo ? __builtin_ctzll(todo) : 0;
        const int X = __shfl(box.lo[0] + (bit & 3), leader, 64), Y = __shfl(box.lo[1] + ((bit >> 2) & 3), leader, 64), Z = __shfl(box.lo[2] + (bit >> 4), leader, 64);
        if (EMIT && lane == 0 && base + (int64_t)count < capacity) cand[base + (int64_t)count] = lg_blk_key(X, Y, Z);
        count++;
        const uint32_t dx = (uint32_t)(X - box.lo[0]), dy = (uint32_t)(Y - box.lo[1]), dz = (uint32_t)(Z - box.lo[2]);
        if (dx < 4u && dy < 4u && dz < 4u) todo &= ~(1ull << ((dz * 4u + dy) * 4u + dx));
        active = __ballot(todo != 0);
    }
    if (!EMIT && lane == 0) {
        wave_n[slot] = count;
        wave_n[(size_t)total_waves + slot] = (uint32_t)__popcll(__ballot(status == 2));
    }
}

// total: the candidates the views produced (lg_mesh_scan_kernel's copy)
__global__ void __launch_bounds__(256) lg_blk_pad_kernel(const int64_t* __restrict__ total, int64_t capacity, int64_t* __restrict__ cand)
{
    const int64_t first = min(total[0], capacity);
    for (int64_t i = first + (int64_t)blockIdx.x * 256 + threadIdx.x; i < capacity; i += (int64_t)gridDim.x * 256) cand[i] = -1;
}

__global__ void __launch_bounds__(256)
lg_blk_concat_kernel(size_t n_old, const int64_t* __restrict__ old_keys, size_t n_add, const int64_t* __restrict__ add_keys, uint64_t* __restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_old + n_add; i += (size_t)gridDim.x * 256)
        out[i] = (uint64_t)(i < n_old ? old_keys[i] : add_keys[i - n_old]);
}

// sorted [n] ascending as unsigned words; a key is kept when it is not negative and differs from its predecessor.  1024 keys per workgroup.
// EMIT also turns the count into -1 when the sort left its error word set.
template <bool EMIT>
__global__ void __launch_bounds__(256)
lg_blk_unique_kernel(size_t n, const uint64_t* __restrict__ sorted, uint32_t* __restrict__ blk, int64_t* __restrict__ merged, const uint32_t* __restrict__ sort_err,
                     int64_t* __restrict__ count)
{
    __shared__ uint32_t ws[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t i0 = (size_t)blockIdx.x * 1024 + (size_t)threadIdx.x * 4;
    bool keep[4];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = i0 + k;
        keep[k] = i < n && (int64_t)sorted[i] >= 0 && (i == 0 || sorted[i] != sorted[i - 1]);
        mine += keep[k] ? 1u : 0u;
    }
    const uint32_t inc = lg_wave_scan_incl(mine, lane);
    lg_block_scan_put(ws, wave, lane, inc);
    __syncthreads();
    uint32_t total;
    const uint32_t woff = lg_block_scan_get<4>(ws, wave, total);
    if (!EMIT) {
        if (threadIdx.x == 0) blk[blockIdx.x] = total;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && sort_err[0]) count[0] = -1;         // the sort gave up (lg_sort.h's poll budget): the list is void
    size_t at = (size_t)blk[blockIdx.x] + woff + inc - mine;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (keep[k]) merged[at++] = (int64_t)sorted[i0 + k];
}

template <bool COLOR>
__global__ void __launch_bounds__(LG_BLK_THREADS)
lg_blk_regrid_kernel(int n_old, const int64_t* __restrict__ old_keys, const int64_t* __restrict__ new_keys, const float* __restrict__ old_tsdf,
                     const float* __restrict__ old_weight, const float* __restrict__ old_color, float* __restrict__ tsdf, float* __restrict__ weight,
                     float* __restrict__ color)
{
    const int r = lg_blk_find(old_keys, n_old, new_keys[blockIdx.x]);
    const bool found = (uint32_t)r < (uint32_t)n_old;
    const size_t to = (size_t)blockIdx.x * (LG_BLK_POINTS / 4) + threadIdx.x, from = (size_t)(found ? r : 0) * (LG_BLK_POINTS / 4) + threadIdx.x;
    ((lg_f4*)tsdf)[to] = found ? ((const lg_f4*)old_tsdf)[from] : lg_f4{ 1.0f, 1.0f, 1.0f, 1.0f };
    ((lg_f4*)weight)[to] = found ? ((const lg_f4*)old_weight)[from] : lg_f4{ 0.0f, 0.0f, 0.0f, 0.0f };
    if (COLOR) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const size_t o = (size_t)j * LG_BLK_THREADS;
            ((lg_f4*)color)[3 * (size_t)blockIdx.x * LG_BLK_THREADS + o + threadIdx.x] =
                found ? ((const lg_f4*)old_color)[3 * (size_t)r * LG_BLK_THREADS + o + threadIdx.x] : lg_f4{ 0.0f, 0.0f, 0.0f, 0.0f };
        }
    }
}

__global__ void __launch_bounds__(256) lg_blk_nbr_kernel(int n, const int64_t* __restrict__ keys, int32_t* __restrict__ nbr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * 8) return;
    const int b = (int)(i >> 3);
    const uint32_t m = (uint32_t)(i & 7);
    int bx, by, bz;
    lg_blk_coords(keys[b], bx, by, bz);
    bx += (int)(m & 1u); by += (int)((m >> 1) & 1u); bz += (int)((m >> 2) & 1u);
    int r = -1;
    if (m == 0u) r = b;
    else if (bx < LG_BLK_BIAS && by < LG_BLK_BIAS && bz < LG_BLK_BIAS) r = lg_blk_find(keys, n, lg_blk_key(bx, by, bz));
    nbr[i] = r;
}

// One workgroup per block, lane = run: x0 = 4 (lane & 1), y = (lane >> 1) & 7, z = lane >> 4; the pools are 16-byte aligned, so is every run.
template <bool COLOR>
__global__ void __launch_bounds__(LG_BLK_THREADS)
lg_blk_integrate_kernel(LgTsdfLattice g, const int64_t* __restrict__ keys, int n_views, LgTsdfBatch b, float* __restrict__ tsdf, float* __restrict__ weight,
                        float* __restrict__ color)
{
    int bx, by, bz;
    lg_blk_coords(keys[blockIdx.x], bx, by, bz);
    const uint32_t r = threadIdx.x;
    const int x0 = bx * LG_BLK + (int)(r & 1u) * 4, y = by * LG_BLK + (int)((r >> 1) & 7u), z = bz * LG_BLK + (int)(r >> 4);
    const size_t p0 = (size_t)blockIdx.x * LG_BLK_POINTS + (size_t)r * 4;

    // Whole-block cull, the same for every lane.  z of a point is affine in its coordinates, and lg_tsdf_coord is monotonic in the index:
    // over the block z <= z(lowest corner) + sum_a max(0, vm[4 a + 2] extent_a) in real arithmetic.  The float z that lg_tsdf_project
    // compares with z_min, this bound's own terms and the corner's z are each within a few ulp of `scale` = sum_a |vm[4 a + 2]| max |coordinate|
    // + |vm[14]| of their real values (under 1e-6 scale in all); 1e-5 scale is added before a view is dropped, and a NaN keeps it.
    const float lo[3] = { lg_tsdf_coord(g.o[0], g.voxel, bx * LG_BLK), lg_tsdf_coord(g.o[1], g.voxel, by * LG_BLK), lg_tsdf_coord(g.o[2], g.voxel, bz * LG_BLK) };
    const float hi[3] = { lg_tsdf_coord(g.o[0], g.voxel, bx * LG_BLK + 7), lg_tsdf_coord(g.o[1], g.voxel, by * LG_BLK + 7), lg_tsdf_coord(g.o[2], g.voxel, bz * LG_BLK + 7) };
    uint32_t reach = 0;
    for (int v = 0; v < n_views; v++) {
        const float* vm = b.v[v].vm;
        float zmax = vm[14], scale = fabsf(vm[14]);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float m = vm[4 * a + 2];
            zmax += m * lo[a] + fmaxf(0.0f, m * (hi[a] - lo[a]));
            scale += fabsf(m) * fmaxf(fabsf(lo[a]), fabsf(hi[a]));
        }
        if (!(zmax + 1e-5f * scale <= b.v[v].cam.z_min)) reach |= 1u << v;
    }
    if (reach == 0u) return;

    LgTsdfRun<COLOR> run;
    run.load(tsdf, weight, color, p0, true, 4);
    const float py = lg_tsdf_coord(g.o[1], g.voxel, y), pz = lg_tsdf_coord(g.o[2], g.voxel, z);
    float px[4];
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] = lg_tsdf_coord(g.o[0], g.voxel, x0 + k);
    bool touched = false;
    for (int v = 0; v < n_views; v++) {
        if (!((reach >> v) & 1u)) continue;
        LgTsdfFetch cur;
        lg_tsdf_fetch(b.v[v], 4, px, py, pz, cur);
        touched |= lg_tsdf_apply_view<COLOR>(&b.v[v], g.trunc, cur, run);
    }
    if (touched) run.store(tsdf, weight, color, p0, true, 4);
}

// ---- marching tetrahedra across block borders -------------------------------------------------------------------------------------
// the halo of tsdf and weight of block `blk` into LDS: a point of a missing neighbour is fresh (tsdf 1, weight 0: unobserved under any
// positive min_weight)
__device__ __forceinline__ void lg_blk_stage_field(uint32_t blk, uint32_t n, const int32_t* __restrict__ nbr, const float* __restrict__ tsdf,
                                                   const float* __restrict__ weight, float* ht, float* hw)
{
    for (int h = (int)threadIdx.x; h < LG_BLK_HALO_POINTS; h += LG_BLK_MESH_THREADS) {
        uint32_t m; int local;
        lg_blk_halo_source(h, m, local);
        const uint32_t r = (uint32_t)nbr[(size_t)blk * 8 + m];
        const bool there = r < n;
        ht[h] = there ? tsdf[(size_t)r * LG_BLK_POINTS + local] : 1.0f;
        hw[h] = there ? weight[(size_t)r * LG_BLK_POINTS + local] : 0.0f;
    }
}

__global__ void __launch_bounds__(LG_BLK_MESH_THREADS)
lg_blk_mesh_count_kernel(uint32_t n, float iso, float min_weight, const int32_t* __restrict__ nbr, const float* __restrict__ tsdf, const float* __restrict__ weight,
                         uint8_t* __restrict__ vmask, uint8_t* __restrict__ fcount, uint32_t* __restrict__ blk_v, uint32_t* __restrict__ blk_f)
{
    __shared__ float ht[LG_BLK_HALO_POINTS], hw[LG_BLK_HALO_POINTS];
    lg_blk_stage_field(blockIdx.x, n, nbr, tsdf, weight, ht, hw);
    __syncthreads();
    uint32_t nv = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int p = (int)threadIdx.x * 2 + k, x = p & 7, y = (p >> 3) & 7, z = p >> 6;
        const uint32_t m = lg_mesh_edge_mask(ht, hw, LG_BLK_HALO, LG_BLK_HALO, LG_BLK_HALO, x, y, z, iso, min_weight);
        uint32_t faces = 0, inside8;
        if (lg_mesh_cell_corners(ht, hw, LG_BLK_HALO, LG_BLK_HALO, x, y, z, iso, min_weight, inside8)) faces = lg_mesh_cell_count(inside8);
        vmask[(size_t)blockIdx.x * LG_BLK_POINTS + p] = (uint8_t)m; fcount[(size_t)blockIdx.x * LG_BLK_POINTS + p] = (uint8_t)faces;
        nv += lg_mesh_popc8(m); nf += faces;
    }
    lg_mesh_put_totals(nv, nf, blk_v, blk_f);
}

// n_vertices, n_faces: the sizes of the outputs (the host has held them against the counts); a store past them is dropped
__global__ void __launch_bounds__(LG_BLK_MESH_THREADS)
lg_blk_mesh_emit_kernel(uint32_t n, LgTsdfLattice g, float iso, float min_weight, const int64_t* __restrict__ keys, const int32_t* __restrict__ nbr,
                        const float* __restrict__ tsdf, const float* __restrict__ weight, const float* __restrict__ color, const uint32_t* __restrict__ vprefix,
                        const uint32_t* __restrict__ fprefix, const uint8_t* __restrict__ vmask, const uint8_t* __restrict__ fcount, int64_t n_vertices,
                        int64_t n_faces, float* __restrict__ vertices, float* __restrict__ colors, int32_t* __restrict__ faces)
{
    __shared__ float ht[LG_BLK_HALO_POINTS], hw[LG_BLK_HALO_POINTS];
    __shared__ uint32_t hp[LG_BLK_HALO_POINTS];
    __shared__ uint8_t hm[LG_BLK_HALO_POINTS + 3];
    lg_blk_stage_field(blockIdx.x, n, nbr, tsdf, weight, ht, hw);
    for (int h = (int)threadIdx.x; h < LG_BLK_HALO_POINTS; h += LG_BLK_MESH_THREADS) {
        uint32_t m; int local;
        lg_blk_halo_source(h, m, local);
        const uint32_t r = (uint32_t)nbr[(size_t)blockIdx.x * 8 + m];
        const bool there = r < n;
        hp[h] = there ? vprefix[(size_t)r * LG_BLK_POINTS + local] : 0u;
        hm[h] = there ? vmask[(size_t)r * LG_BLK_POINTS + local] : (uint8_t)0;
    }
    __syncthreads();
    int bx, by, bz;
    lg_blk_coords(keys[blockIdx.x], bx, by, bz);
#pragma unroll
    for (int k2 = 0; k2 < 2; k2++) {
        const int p = (int)threadIdx.x * 2 + k2, x = p & 7, y = (p >> 3) & 7, z = p >> 6;
        const int h0 = lg_blk_halo_index(x, y, z);
        const uint32_t m = hm[h0];
        if (m) {
            size_t id = hp[h0];
            const size_t gp = (size_t)blockIdx.x * LG_BLK_POINTS + p;
            for (uint32_t k = 0; k < LG_MESH_SLOTS; k++)
                if ((m >> k) & 1u) {
                    const uint32_t sm = lg_mesh_slot_mask(k);
                    const int x1 = x + (int)(sm & 1u), y1 = y + (int)((sm >> 1) & 1u), z1 = z + (int)((sm >> 2) & 1u);
                    const int h1 = lg_blk_halo_index(x1, y1, z1);
                    float pos[3], rgb[3] = { 0.0f, 0.0f, 0.0f };
                    const float* c0 = nullptr; const float* c1 = nullptr;
                    if (colors) {
                        uint32_t qm; int ql;
                        lg_blk_halo_source(h1, qm, ql);
                        const uint32_t rq = (uint32_t)nbr[(size_t)blockIdx.x * 8 + qm];        // (the edge carries: its far end is observed, so its block exists)
                        c0 = color + 3 * gp;
                        c1 = rq < n ? color + 3 * ((size_t)rq * LG_BLK_POINTS + ql) : c0;
                    }
                    lg_mesh_edge_vertex(ht[h0], ht[h1], c0, c1, bx * LG_BLK + x, by * LG_BLK + y, bz * LG_BLK + z, k, iso, g.o, g.voxel, pos, rgb);
                    lg_mesh_put_vertex(id, n_vertices, pos, rgb, vertices, colors);
                    id++;
                }
        }
        const size_t gp = (size_t)blockIdx.x * LG_BLK_POINTS + p;
        if (fcount[gp]) {
            uint32_t inside8;
            lg_mesh_cell_corners(ht, hw, LG_BLK_HALO, LG_BLK_HALO, x, y, z, iso, min_weight, inside8);
            const size_t first = fprefix[gp];
            if ((int64_t)first < n_faces) lg_mesh_cell_faces(LG_BLK_HALO, LG_BLK_HALO, x, y, z, inside8, hp, hm, faces + 3 * first, n_faces - (int64_t)first);
        }
    }
}
