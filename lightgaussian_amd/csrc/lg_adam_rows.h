// lg_adam_rows.h -- row index of an element of a span, for lg_adam_rows_kernel (lg_adam.h; DESIGN section 10.1, "visible rows").
// A tensor [rows, ...] is stepped in spans of LG_ADAM_SPAN elements; a row of row_len = numel / rows elements starts anywhere in a
// span (4096 is no multiple of 45).  The kernel needs the row of every element it touches without a 64-bit division per lane:
//     once per workgroup (uniform)   first = base / row_len, rem = base - first * row_len        base = span index * LG_ADAM_SPAN
//     per element k of the span      row   = first + lg_adam_local_row(rem + k, rcp, thr)      rem + k < row_len + LG_ADAM_SPAN, 32 bits
// lg_adam_local_row(x, rcp, thr) = x / d for every x < d + LG_ADAM_SPAN, without a branch: ((x * rcp) >> 32) + (x >= thr ? 1 : 0)
//     1 < d < LG_ADAM_SPAN   rcp = floor(2^32 / d) + 1, thr = 2^32 - 1 (never reached): exact, since x < 2 LG_ADAM_SPAN = 2^13 and
//                            rcp * d - 2^32 <= d make x * rcp / 2^32 exceed x / d by less than 2^-19 < 1 / d
//     d >= LG_ADAM_SPAN      rcp = 0, thr = d: the quotient is 0 or 1
//     d == 1                 rcp = 2^32 - 1, thr = 1: (x * (2^32 - 1)) >> 32 = x - 1 for x >= 1 and 0 for x = 0
// Plain C, host and device: tests/cpu_harness/lg_adam_rows_harness.cpp checks it against integer division.
#pragma once
#include <stdint.h>

#include "../../include/lightgaussian.h"

#if defined(__HIPCC__)
#define LG_ADAM_HD __host__ __device__ __forceinline__
#else
#define LG_ADAM_HD static inline
#endif

#define LG_ADAM_MAX_ROW_LEN 0x7FFFFFFF      /* rem + k stays below 2^32 */

LG_ADAM_HD uint32_t lg_adam_row_rcp(uint32_t row_len)
{
    if (row_len == 1u) return 0xFFFFFFFFu;
    return row_len < (uint32_t)LG_ADAM_SPAN ? (uint32_t)(0x100000000ull / row_len) + 1u : 0u;
}
LG_ADAM_HD uint32_t lg_adam_row_thr(uint32_t row_len)
{
    return row_len == 1u ? 1u : row_len < (uint32_t)LG_ADAM_SPAN ? 0xFFFFFFFFu : row_len;
}

// first row of the span that starts at element `base` (>= 0), and where in that row the span starts
LG_ADAM_HD int64_t lg_adam_first_row(int64_t base, uint32_t row_len, uint32_t* rem)
{
    const int64_t first = base / (int64_t)row_len;
    *rem = (uint32_t)(base - first * (int64_t)row_len);
    return first;
}

LG_ADAM_HD uint32_t lg_adam_local_row(uint32_t x, uint32_t rcp, uint32_t thr)
{
    return (uint32_t)(((uint64_t)x * rcp) >> 32) + (x >= thr ? 1u : 0u);
}
