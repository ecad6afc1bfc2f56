// lg_tsdf.h -- TSDF fusion of rendered depth maps into a dense volume and marching tetrahedra over it (DESIGN section 10.13;
// include/lightgaussian_mesh.h).  Replaces the CPU route of the Gaussian-splatting surface papers (open3d's ScalableTSDFVolume
// integrate per view, extract_triangle_mesh) for a bounded scene.
//
//   lg_tsdf_integrate_kernel <COLOR>
//       one lane per RUN of four x-consecutive points of one grid row; one wave per brick of 16 x 4 x 4 points (lane = run, y, z), the
//       four waves of a workgroup side by side in x, so that the gathers of a wave fall into a small patch of each image and the rows a
//       workgroup stores are 256 contiguous bytes.  Up to LG_TSDF_BATCH views per launch, by value in the kernel arguments.  The lane
//       loads tsdf, weight (and colour) of its run once -- one dwordx4 each (three for colour) where the run is whole and 16-byte aligned,
//       dwords otherwise (lg_rows.h's two paths; LgTsdfRun) --, carries them in registers through the views IN ORDER and stores them
//       once, and not at all when no view touched the run.  Per view and point: lg_tsdf_project, the depth gather, lg_tsdf_sample; alpha
//       and colour are gathered by the points that pass (a thin band about the surface), then lg_tsdf_apply (lg_tsdf_apply_view) --
//       lg_math.h's text throughout.  The four depth gathers of view v + 1 are in flight while view v is applied (lg_tsdf_fetch).  A
//       pass moves 8 + 8 bytes per point (20 + 20 with colour) whatever the number of views.
//   lg_mesh_count_kernel      per point its edge mask (which of its seven edge slots carry a vertex) and the faces of its cell, as bytes;
//                             per workgroup of 1024 points both totals
//   lg_mesh_scan_kernel       exclusive scan of the workgroup totals, one workgroup per channel (vertices, faces), the grand totals as int64
//   lg_mesh_prefix_kernel <N, WHOLE>  per point the exclusive prefix of both counts: workgroup offset + the scan inside the workgroup; N
//                             points per lane (4 here; 2, and no tests against P, for the blocks of lg_blocks.h)
//   lg_mesh_emit_kernel       per point its vertices (position, colour) at prefix + rank, per valid cell its faces at its face prefix:
//                             plain stores, no atomics; every element of the outputs is written once
// The scans are lg_wave_scan_incl + lg_block_scan_put / _get (lg_wave.h), the three phases of lg_compact.h.
// No atomics, no memset; results are bit-identical from run to run.
//
// This header is also the home of what the block-sparse volume (lg_blocks.h) shares with this one, each written once: LgTsdfLattice
// (origin, voxel, trunc), lg_tsdf_view_matrix, LgTsdfFetch / lg_tsdf_fetch, LgTsdfRun (a lane's run: load, store, both paths),
// lg_tsdf_apply_view (one view applied to a run), LgMeshScratch / carve_mesh, lg_mesh_put_totals (the tail of a count kernel),
// lg_mesh_scan_kernel, lg_mesh_prefix_kernel and lg_mesh_put_vertex (the bounded store of an emit kernel).  The integrate, count and
// emit KERNELS stay two each: the bricks differ (16 x 4 x 4 points per wave and the next view prefetched here; one 8^3 block per two
// waves and a whole-block z_min cull there), and the block mesh kernels stage a 9^3 halo in LDS where these index the grid.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "../../include/lightgaussian_mesh.h"
#include "lg_host.h"
#include "lg_wave.h"
#include "lg_rows.h"

#define LG_TSDF_THREADS 256
#define LG_TSDF_BATCH 8                     // views per launch
#define LG_TSDF_MAX_POINTS (1 << 29)        // nx ny nz < 2^29: seven edge slots per point count in 32 bits
#define LG_TSDF_MAX_DIM 32768               // W, H of a view
#define LG_MESH_POINTS 1024                 // points per workgroup of the mesh kernels (256 threads x 4)

// the lattice every kernel of this header and of lg_blocks.h places its points on: point i at lg_tsdf_coord(o, voxel, i) per axis; the band
struct LgTsdfLattice { float o[3]; float voxel, trunc; };
struct LgMeshDims { int nx, ny, nz; };
struct LgTsdfViewArg { const float* vm; const float* depth; const float* color; const float* alpha; LgTsdfCam cam; };
struct LgTsdfBatch { LgTsdfViewArg v[LG_TSDF_BATCH]; };

#define LG_TSDF_BRICK_X 64                  // points a workgroup covers in x (4 waves x 4 runs x 4 points), and in y and in z
#define LG_TSDF_BRICK_YZ 4
static inline size_t lg_tsdf_bricks(int nx, int ny, int nz)
{
    return (size_t)((nx + LG_TSDF_BRICK_X - 1) / LG_TSDF_BRICK_X) * (size_t)((ny + LG_TSDF_BRICK_YZ - 1) / LG_TSDF_BRICK_YZ) *
           (size_t)((nz + LG_TSDF_BRICK_YZ - 1) / LG_TSDF_BRICK_YZ);
}

// the 16 floats of a view matrix into registers
__device__ __forceinline__ void lg_tsdf_view_matrix(const float* src, float (&vm)[16])
{
#pragma unroll
    for (int k = 0; k < 16; k++) vm[k] = src[k];
}

// what a lane holds of one view: per point of its run whether it projects into the image, its view-space z, its pixel and the depth there
struct LgTsdfFetch { bool ok[4]; float z[4], d[4]; uint32_t pix[4]; };
__device__ __forceinline__ void lg_tsdf_fetch(const LgTsdfViewArg& a, int live, const float (&px)[4], float py, float pz, LgTsdfFetch& o)
{
    float vm[16];
    lg_tsdf_view_matrix(a.vm, vm);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int ix = 0, iy = 0;
        o.z[k] = 0.0f;
        o.ok[k] = k < live && lg_tsdf_project(vm, a.cam, px[k], py, pz, ix, iy, o.z[k]);
        o.pix[k] = o.ok[k] ? (uint32_t)iy * (uint32_t)a.cam.W + (uint32_t)ix : 0u;       // (W H <= 2^30)
    }
#pragma unroll
    for (int k = 0; k < 4; k++) o.d[k] = a.depth[o.pix[k]];      // unconditional: a point outside the image reads pixel 0 and drops it
}

// A lane's run of four x-consecutive points, p0 the linear index of the first: tsdf, weight (and colour) in registers between one load
// and one store.  whole: the run has four points and p0 is a multiple of 4 under 16-byte aligned arrays, so it moves as dwordx4 (three
// for colour); otherwise the first `live` points move as dwords (lg_rows.h's two paths).  A caller whose runs are all whole passes
// (true, 4) and keeps the dwordx4 path alone.
template <bool COLOR>
struct LgTsdfRun {
    float f[4], w[4], c[4][3];

    __device__ __forceinline__ void load(const float* tsdf, const float* weight, const float* color, size_t p0, bool whole, int live)
    {
        if (whole) {
            const lg_f4 tf = *(const lg_f4*)(tsdf + p0), tw = *(const lg_f4*)(weight + p0);
#pragma unroll
            for (int k = 0; k < 4; k++) { f[k] = tf[k]; w[k] = tw[k]; }
            if (COLOR) {
                lg_f4 tc[3];
#pragma unroll
                for (int j = 0; j < 3; j++) tc[j] = *(const lg_f4*)(color + 3 * p0 + 4 * j);
#pragma unroll
                for (int e = 0; e < 12; e++) c[e / 3][e % 3] = tc[e / 4][e % 4];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < live) {
                    f[k] = tsdf[p0 + k]; w[k] = weight[p0 + k];
                    if (COLOR) {
#pragma unroll
                        for (int a = 0; a < 3; a++) c[k][a] = color[3 * (p0 + k) + a];
                    }
                }
        }
    }
    __device__ __forceinline__ void store(float* tsdf, float* weight, float* color, size_t p0, bool whole, int live) const
    {
        if (whole) {
            *(lg_f4*)(tsdf + p0) = lg_f4{ f[0], f[1], f[2], f[3] };
            *(lg_f4*)(weight + p0) = lg_f4{ w[0], w[1], w[2], w[3] };
            if (COLOR) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    lg_f4 t;
#pragma unroll
                    for (int e = 0; e < 4; e++) t[e] = c[(4 * j + e) / 3][(4 * j + e) % 3];
                    *(lg_f4*)(color + 3 * p0 + 4 * j) = t;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < live) {
                    tsdf[p0 + k] = f[k]; weight[p0 + k] = w[k];
                    if (COLOR) {
#pragma unroll
                        for (int a = 0; a < 3; a++) color[3 * (p0 + k) + a] = c[k][a];
                    }
                }
        }
    }
};

// One view applied to a run whose fetch is `cur`: alpha and colour are gathered by the points that pass lg_tsdf_sample, then
// lg_tsdf_apply.  Returns whether a point of the run was updated.  The view comes as a pointer on purpose: a reference parameter
// tells the compiler that all of *view may be read ahead of the `if`, and the alpha / colour pointers it then loads early cost the
// dense colour kernel three VGPRs (67, one wave per SIMD less) and the block one one.
template <bool COLOR>
__device__ __forceinline__ bool lg_tsdf_apply_view(const LgTsdfViewArg* view, float trunc, const LgTsdfFetch& cur, LgTsdfRun<COLOR>& run)
{
    const LgTsdfViewArg& a = *view;
    const size_t plane = (size_t)a.cam.H * (size_t)a.cam.W;
    bool touched = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float t;
        if (cur.ok[k] && lg_tsdf_sample(a.cam, trunc, cur.d[k], cur.z[k], t)) {
            LgTsdfPixel p = { cur.d[k], a.alpha ? a.alpha[cur.pix[k]] : 0.0f, { 0.0f, 0.0f, 0.0f } };
            if (COLOR) { p.rgb[0] = a.color[cur.pix[k]]; p.rgb[1] = a.color[plane + cur.pix[k]]; p.rgb[2] = a.color[2 * plane + cur.pix[k]]; }
            touched |= lg_tsdf_apply(a.cam, trunc, p, a.alpha != nullptr, cur.z[k], run.f[k], run.w[k], COLOR ? run.c[k] : nullptr);
        }
    }
    return touched;
}

// vec: tsdf, weight (and color) are 16-byte aligned, so a whole run whose first point has a linear index that is a multiple of 4 moves as dwordx4
template <bool COLOR>
__global__ void __launch_bounds__(LG_TSDF_THREADS)
lg_tsdf_integrate_kernel(LgMeshDims d, LgTsdfLattice g, int vec, int n_views, LgTsdfBatch b, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color)
{
    const uint32_t nbx = (uint32_t)(d.nx + LG_TSDF_BRICK_X - 1) / LG_TSDF_BRICK_X, nby = (uint32_t)(d.ny + LG_TSDF_BRICK_YZ - 1) / LG_TSDF_BRICK_YZ;
    const uint32_t bx = blockIdx.x % nbx, byz = blockIdx.x / nbx, by = byz % nby, bz = byz / nby;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int x0 = (int)(bx * LG_TSDF_BRICK_X + wave * 16u + (lane & 3u) * 4u);
    const int y = (int)(by * LG_TSDF_BRICK_YZ + ((lane >> 2) & 3u)), z = (int)(bz * LG_TSDF_BRICK_YZ + (lane >> 4));
    if (x0 >= d.nx || y >= d.ny || z >= d.nz) return;
    const int live = min(4, d.nx - x0);
    const size_t p0 = ((size_t)z * (size_t)d.ny + (size_t)y) * (size_t)d.nx + (size_t)x0;
    const bool whole = vec && live == 4 && (p0 & 3) == 0;

    LgTsdfRun<COLOR> run;
    run.load(tsdf, weight, color, p0, whole, live);
    const float py = lg_tsdf_coord(g.o[1], g.voxel, y), pz = lg_tsdf_coord(g.o[2], g.voxel, z);
    float px[4];
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] = lg_tsdf_coord(g.o[0], g.voxel, x0 + k);
    bool touched = false;
    LgTsdfFetch cur, nxt;
    lg_tsdf_fetch(b.v[0], live, px, py, pz, cur);
    for (int v = 0; v < n_views; v++) {
        lg_tsdf_fetch(b.v[min(v + 1, n_views - 1)], live, px, py, pz, nxt);        // (the last turn fetches its own view again: nobody reads it)
        touched |= lg_tsdf_apply_view<COLOR>(&b.v[v], g.trunc, cur, run);
        cur = nxt;
    }
    if (touched) run.store(tsdf, weight, color, p0, whole, live);
}

// ---- marching tetrahedra ----------------------------------------------------------------------------------------------------------
// scratch of lg_mesh_count / lg_mesh_emit and of lg_blocks_mesh_count / lg_blocks_mesh_emit (P = 512 n there)
struct LgMeshScratch {
    int64_t* counts;        // [2] vertices, faces: what the count call found (the emit call holds its arguments against them)
    int32_t* nbr;           // [n][8] of a block volume (lg_blk_nbr_kernel); empty for the dense volume
    uint32_t* vprefix;      // [P] vertex id of the first carrying slot of the point
    uint32_t* fprefix;      // [P] index of the first face of the point's cell
    uint32_t* blk;          // [2][groups] workgroup totals, then their exclusive scans, per channel: ceil(P / 1024) groups, or n
    uint8_t* vmask;         // [P] lg_mesh_edge_mask
    uint8_t* fcount;        // [P] faces of the point's cell (0 .. 12; 0 for a point without a valid cell)
    size_t total;
};
static inline size_t lg_mesh_blocks(size_t P) { return (P + LG_MESH_POINTS - 1) / LG_MESH_POINTS; }
// groups: workgroups of the count kernel; nbr_blocks: blocks with a row of nbr (0: the dense volume, whose nbr takes no bytes)
static LgMeshScratch carve_mesh(void* base, size_t P, size_t groups, size_t nbr_blocks)
{
    LgMeshScratch s; size_t off = 0; char* p = (char*)base;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    s.counts = (int64_t*)take(16);
    s.nbr = (int32_t*)take(nbr_blocks * 8 * 4);
    s.vprefix = (uint32_t*)take(P * 4);
    s.fprefix = (uint32_t*)take(P * 4);
    s.blk = (uint32_t*)take(2 * groups * 4);
    s.vmask = (uint8_t*)take(P);
    s.fcount = (uint8_t*)take(P);
    s.total = off;
    return s;
}

// A lane's vertices and faces into the totals of its workgroup of 256 lanes: blk_v, blk_f [blockIdx.x].  Every lane calls it.
__device__ __forceinline__ void lg_mesh_put_totals(uint32_t nv, uint32_t nf, uint32_t* __restrict__ blk_v, uint32_t* __restrict__ blk_f)
{
    __shared__ uint32_t ws[2][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t iv = lg_wave_scan_incl(nv, lane), jf = lg_wave_scan_incl(nf, lane);
    lg_block_scan_put(ws[0], wave, lane, iv);
    lg_block_scan_put(ws[1], wave, lane, jf);
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_v[blockIdx.x] = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
        blk_f[blockIdx.x] = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
    }
}

__device__ __forceinline__ void lg_mesh_xyz(const LgMeshDims& d, size_t p, int& x, int& y, int& z)
{
    const size_t row = p / (size_t)d.nx;
    x = (int)(p - row * (size_t)d.nx); y = (int)(row % (size_t)d.ny); z = (int)(row / (size_t)d.ny);
}

__global__ void __launch_bounds__(256)
lg_mesh_count_kernel(LgMeshDims d, size_t P, float iso, float min_weight, const float* __restrict__ tsdf, const float* __restrict__ weight,
                     uint8_t* __restrict__ vmask, uint8_t* __restrict__ fcount, uint32_t* __restrict__ blk_v, uint32_t* __restrict__ blk_f)
{
    const size_t p0 = (size_t)blockIdx.x * LG_MESH_POINTS + (size_t)threadIdx.x * 4;
    uint32_t nv = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t p = p0 + k;
        if (p < P) {
            int x, y, z;
            lg_mesh_xyz(d, p, x, y, z);
            const uint32_t m = lg_mesh_edge_mask(tsdf, weight, d.nx, d.ny, d.nz, x, y, z, iso, min_weight);
            uint32_t faces = 0, inside8;
            if (x < d.nx - 1 && y < d.ny - 1 && z < d.nz - 1 && lg_mesh_cell_corners(tsdf, weight, d.nx, d.ny, x, y, z, iso, min_weight, inside8))
                faces = lg_mesh_cell_count(inside8);
            vmask[p] = (uint8_t)m; fcount[p] = (uint8_t)faces;
            nv += lg_mesh_popc8(m); nf += faces;
        }
    }
    lg_mesh_put_totals(nv, nf, blk_v, blk_f);
}

// workgroup c scans channel c (0 vertices, 1 faces) of the workgroup totals in place; the grand totals go to counts[c] and copy[c] as int64
__global__ void __launch_bounds__(1024)
lg_mesh_scan_kernel(size_t n, uint32_t* __restrict__ blk, int64_t* __restrict__ counts, int64_t* __restrict__ copy)
{
    __shared__ uint32_t wsum[16];
    uint32_t* __restrict__ io = blk + (size_t)blockIdx.x * n;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t carry = 0;
    for (size_t base = 0; base < n; base += 1024) {
        const size_t i = base + tid;
        const uint32_t v = i < n ? io[i] : 0u;
        const uint32_t x = lg_wave_scan_incl(v, lane);
        lg_block_scan_put(wsum, wave, lane, x);
        __syncthreads();
        uint32_t tot;
        const uint32_t woff = lg_block_scan_get<16>(wsum, wave, tot);
        if (i < n) io[i] = (uint32_t)carry + woff + x - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) { counts[blockIdx.x] = (int64_t)carry; copy[blockIdx.x] = (int64_t)carry; }
}

// N points per lane, 256 N per workgroup: the workgroups of the count kernel whose totals blk_v, blk_f hold (4: the dense volume's 1024
// points; 2: one block of 512).  WHOLE: P is a multiple of 256 N, as every block volume's is, and no point is held against P: a lane's
// bytes and prefixes then move as one load and one store each (with the tests the block volume's extraction ran 2 to 3 % longer).
template <int N, bool WHOLE>
__global__ void __launch_bounds__(256)
lg_mesh_prefix_kernel(size_t P, const uint8_t* __restrict__ vmask, const uint8_t* __restrict__ fcount, const uint32_t* __restrict__ blk_v,
                      const uint32_t* __restrict__ blk_f, uint32_t* __restrict__ vprefix, uint32_t* __restrict__ fprefix)
{
    __shared__ uint32_t ws[2][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t p0 = (size_t)blockIdx.x * (256 * N) + (size_t)threadIdx.x * N;
    uint32_t cv[N], cf[N], nv = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
        cv[k] = (WHOLE || p0 + k < P) ? lg_mesh_popc8(vmask[p0 + k]) : 0u;
        cf[k] = (WHOLE || p0 + k < P) ? (uint32_t)fcount[p0 + k] : 0u;
        nv += cv[k]; nf += cf[k];
    }
    const uint32_t iv = lg_wave_scan_incl(nv, lane), jf = lg_wave_scan_incl(nf, lane);
    lg_block_scan_put(ws[0], wave, lane, iv);
    lg_block_scan_put(ws[1], wave, lane, jf);
    __syncthreads();
    uint32_t tv, tf;
    uint32_t pv = blk_v[blockIdx.x] + lg_block_scan_get<4>(ws[0], wave, tv) + iv - nv;
    uint32_t pf = blk_f[blockIdx.x] + lg_block_scan_get<4>(ws[1], wave, tf) + jf - nf;
#pragma unroll
    for (int k = 0; k < N; k++)
        if (WHOLE || p0 + k < P) { vprefix[p0 + k] = pv; fprefix[p0 + k] = pf; pv += cv[k]; pf += cf[k]; }
}

// vertex `id` into the outputs of an emit kernel: position, and colour where colors is given; an id past n_vertices is dropped
__device__ __forceinline__ void lg_mesh_put_vertex(size_t id, int64_t n_vertices, const float (&pos)[3], const float (&rgb)[3], float* vertices, float* colors)
{
    if ((int64_t)id < n_vertices) {
#pragma unroll
        for (int a = 0; a < 3; a++) vertices[3 * id + a] = pos[a];
        if (colors) {
#pragma unroll
            for (int a = 0; a < 3; a++) colors[3 * id + a] = rgb[a];
        }
    }
}

// n_vertices, n_faces: the sizes of the outputs (the host has held them against the counts); a store past them is dropped
__global__ void __launch_bounds__(256)
lg_mesh_emit_kernel(LgMeshDims d, size_t P, LgTsdfLattice org, float iso, float min_weight, const float* __restrict__ tsdf, const float* __restrict__ weight,
                    const float* __restrict__ color, const uint32_t* __restrict__ vprefix, const uint32_t* __restrict__ fprefix,
                    const uint8_t* __restrict__ vmask, const uint8_t* __restrict__ fcount, int64_t n_vertices, int64_t n_faces,
                    float* __restrict__ vertices, float* __restrict__ colors, int32_t* __restrict__ faces)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    int x, y, z;
    lg_mesh_xyz(d, p, x, y, z);
    const uint32_t m = vmask[p];
    if (m) {
        size_t id = vprefix[p];
        for (uint32_t k = 0; k < LG_MESH_SLOTS; k++)
            if ((m >> k) & 1u) {
                float pos[3], rgb[3] = { 0.0f, 0.0f, 0.0f };
                lg_mesh_vertex(tsdf, colors ? color : nullptr, d.nx, d.ny, x, y, z, k, iso, org.o, org.voxel, pos, rgb);
                lg_mesh_put_vertex(id, n_vertices, pos, rgb, vertices, colors);
                id++;
            }
    }
    const uint32_t nf = fcount[p];
    if (nf) {
        uint32_t inside8;
        lg_mesh_cell_corners(tsdf, weight, d.nx, d.ny, x, y, z, iso, min_weight, inside8);
        const size_t first = fprefix[p];
        if ((int64_t)first < n_faces) lg_mesh_cell_faces(d.nx, d.ny, x, y, z, inside8, vprefix, vmask, faces + 3 * first, n_faces - (int64_t)first);
    }
}
