// lg_wave.h -- wave64 primitives: lane id, prefix popcount, DPP reductions, inclusive wave scan, butterfly all-reduces, two-part workgroup scan, LDS hand-over
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// ------------------------------------------------------------------------------------------------
// wave64 helpers
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t prefix_popc(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// DPP wave reduction: after the call lane 63 holds the sum over all 64 lanes.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v)
{
    int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, ROW_MASK == 0xf);
    return v + __int_as_float(moved);
}
__device__ __forceinline__ float wave_sum_to_lane63(float v)
{
    v = dpp_add<0x111, 0xf>(v); // row_shr:1
    v = dpp_add<0x112, 0xf>(v); // row_shr:2
    v = dpp_add<0x114, 0xf>(v); // row_shr:4
    v = dpp_add<0x118, 0xf>(v); // row_shr:8   -> lane 15 of every row holds the row total
    v = dpp_add<0x142, 0xa>(v); // row_bcast:15 into rows 1,3
    v = dpp_add<0x143, 0xc>(v); // row_bcast:31 into rows 2,3 -> lane 63 = total
    return v;
}


// integer add across lanes through DPP (one v_add_u32_dpp): every lane receives v + v[partner]
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_add_u32(uint32_t v)
{
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

// unsigned maximum across lanes through DPP: every lane receives max(v, v[partner])
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max_u32(uint32_t v)
{
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true));
}

// inclusive prefix sum over the 64 lanes of a wave (6 shuffle steps; every lane takes part)
__device__ __forceinline__ uint32_t lg_wave_scan_incl(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(v, s, 64);
        if ((int)lane >= s) v += o;
    }
    return v;
}

// butterfly all-reduces: every lane receives the maximum / or over the 64 lanes.  (There is no sum: at its two sites, lg_compact_count
// and lg_preprocess, a helper changed the kernel's register figures or instruction text, so they keep their loops.)
__device__ __forceinline__ uint32_t lg_wave_all_max(uint32_t v)
{
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, sh));
    return v;
}
__device__ __forceinline__ float lg_wave_all_max(float v)
{
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v = fmaxf(v, __shfl_xor(v, sh, 64));
    return v;
}
__device__ __forceinline__ uint32_t lg_wave_all_or(uint32_t v)
{
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v |= (uint32_t)__shfl_xor((int)v, sh);
    return v;
}

// Workgroup exclusive scan on top of lg_wave_scan_incl, in two parts with the CALLER's __syncthreads() between them (callers ride
// other words on that barrier, or scan several channels behind one): put = lane 63 leaves its wave's total (`inc` = the wave's
// inclusive scan), get = sum of the totals of the waves below + the grand total.  The exclusive prefix of a thread is
// get() + inc - its own value.  (The four-wave sites -- lg_ts_base_get, lg_compact_dest, lg_densify_map, lg_onesweep_pass -- sum the
// totals below with a loop over w < wave instead: get's select form changes their kernels' register figures.  Sites that spell
// get's loop out say why where they stand.)
__device__ __forceinline__ void lg_block_scan_put(uint32_t* wsum, uint32_t wave, uint32_t lane, uint32_t inc)
{
    if (lane == 63u) wsum[wave] = inc;
}
template <int WAVES>
__device__ __forceinline__ uint32_t lg_block_scan_get(const uint32_t* wsum, uint32_t wave, uint32_t& total)
{
    uint32_t woff = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t t = wsum[w];
        woff += (w < (int)wave) ? t : 0u;
        total += t;
    }
    return woff;
}

// LDS hand-over inside ONE wave: what its lanes wrote to LDS before the call is what every lane reads after it.  Release fence, wave
// barrier, acquire fence, all at wavefront scope: no s_barrier is issued -- the trio only keeps the compiler (and the LDS counter waits it
// places) from moving an LDS access across.  Sites with another scope or without the acquire say so where they stand.
__device__ __forceinline__ void lg_wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
