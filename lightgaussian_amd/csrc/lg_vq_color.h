// lg_vq_color.h -- per-Gaussian view-dependent colours straight from a VecTree-compressed model (lg_vq_colors).
// The compressed model (vectree/vectree.py:100-155 writes it, vectree/utils.py:5-65 reads it back) keeps the SH coefficients of
// a Gaussian either as a log2(K)-bit index into an fp16 codebook or as an fp16 row of its own.  lightgaussian_amd/vectree.py
// keeps both kinds in ONE device table -- the K codebook rows, then the non-VQ rows, every row padded to a multiple of 16 bytes
// -- and a uint32 slot[N] naming each Gaussian's row.  This kernel turns (camera, that table) into the [N,3] colours that K1
// takes as colors_precomp: the [N, 3 M] float32 SH tensor of the dequantised model (580 MB at 3 M Gaussians, degree 3) never exists.
//
//   one lane per Gaussian:  xyz (12 B) and slot (4 B), the row with 16-byte loads (only the chunks that hold an active
//   coefficient: `need`, a wave-uniform bit mask the host derives from M and the active degree), fp16 -> float (exact),
//   permuted from the file's channel-major order  f_dc_0..2, f_rest_{c (M-1) + j}  to the [M][3] order of lg_sh_to_rgb, then
//   THE SAME lg_sh_to_rgb (lg_math.h) K1 evaluates on the float32 table: with the library-wide -ffp-contract=off the colours are
//   those of the dense path bit for bit.  rgb leaves clamped at 0 with per-lane stores: the three dword stores of a wave cover
//   768 contiguous bytes between them, and staging them through LDS into 16-byte stores (K1's record idiom) measured the same
//   (EXPERIMENTS.md, "lg_vq_colors"), so the simpler form stays.
//
//   Byte model per Gaussian at active degree D:  read 12 (xyz) + 4 (slot) + 2 * 3 * (D + 1)^2 (fp16 coefficients), write 12.
//   Degree 3: 124 B, degree 2: 82 B.  The codebook part of the table is at most 8192 * 96 B = 786 KB and is expected to stay in
//   L2 (4 MB per XCD), so the model counts every row read although 60 % of them never reach HBM; it is larger than LDS (160 KB)
//   and is not staged there.  16-byte granularity reads a little more than the model: a degree-2 row of 54 B is fetched as 64.
// A slot is trusted (the table's row count is not an argument): lightgaussian_amd/vectree.py builds slot[] itself.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "lg_math.h"
#include "lg_preprocess.h"   // LG_PP

typedef _Float16 lg_h8 __attribute__((ext_vector_type(8)));

// position of coefficient m of channel c in a stored row of 3 M halfs (the PLY order f_dc_0..2, f_rest_*, channel-major)
static constexpr int lg_vq_row_index(int M, int m, int c) { return m == 0 ? c : 3 + c * (M - 1) + (m - 1); }

// bit q set: the 16-byte chunk q of a row (halfs 8 q .. 8 q + 7) holds a coefficient of degree <= D
static inline uint32_t lg_vq_need_mask(int M, int D)
{
    uint32_t need = 0;
    const int Ma = (D + 1) * (D + 1);
    for (int m = 0; m < Ma; m++)
        for (int c = 0; c < 3; c++) need |= 1u << (lg_vq_row_index(M, m, c) >> 3);
    return need;
}

template <int M>
__global__ void __launch_bounds__(LG_PP)
lg_vq_colors_kernel(int N, int D, uint32_t need, const float* __restrict__ means3D, const float* __restrict__ campos,
                    const uint32_t* __restrict__ slot, const unsigned char* __restrict__ rows, uint32_t row_stride,
                    float* __restrict__ out_rgb)
{
    constexpr int NH = 3 * M;                 // halfs per row
    constexpr int NQ = (NH + 7) / 8;          // 16-byte chunks per row
    const int i = blockIdx.x * LG_PP + (int)threadIdx.x;
    if (i >= N) return;
    const float px = means3D[3 * (size_t)i], py = means3D[3 * (size_t)i + 1], pz = means3D[3 * (size_t)i + 2];
    const float cp[3] = { campos[0], campos[1], campos[2] };
    const lg_h8* row = reinterpret_cast<const lg_h8*>(rows + (size_t)slot[i] * row_stride);
    _Float16 h[NQ * 8];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        lg_h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (need & (1u << q)) v = row[q];
#pragma unroll
        for (int k = 0; k < 8; k++) h[8 * q + k] = v[k];
    }
    const int Ma = (D + 1) * (D + 1);
    float sh[3 * M];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
        for (int c = 0; c < 3; c++) sh[3 * m + c] = m < Ma ? (float)h[lg_vq_row_index(M, m, c)] : 0.0f;
    float rgb[3];
    uint32_t cb;
    lg_sh_to_rgb(D, sh, px, py, pz, cp, rgb, cb);
    out_rgb[3 * (size_t)i] = rgb[0]; out_rgb[3 * (size_t)i + 1] = rgb[1]; out_rgb[3 * (size_t)i + 2] = rgb[2];
}
