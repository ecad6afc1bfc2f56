// CPU harness around the PRODUCT's row-index helpers of lg_adam_rows_kernel (lightgaussian_amd/csrc/lg_adam_rows.h), for
// tests/test_adam_rows_host.py.  Test infrastructure, compiled with g++; no GPU.
#include "../../lightgaussian_amd/csrc/lg_adam_rows.h"

extern "C" {

int h_adam_span(void) { return LG_ADAM_SPAN; }

// every x the kernel can form for this row_len (x = rem + k, rem < row_len, k < LG_ADAM_SPAN), or, with lo < hi, only x in [lo, hi):
// the number of x whose quotient differs from x / row_len; *first_bad = the first such x
int64_t h_adam_local_rows(uint32_t row_len, uint64_t lo, uint64_t hi, uint64_t* first_bad)
{
    const uint32_t rcp = lg_adam_row_rcp(row_len), thr = lg_adam_row_thr(row_len);
    const uint64_t end = (uint64_t)row_len + LG_ADAM_SPAN;
    if (lo >= hi) { lo = 0; hi = end; }
    if (hi > end) hi = end;
    int64_t bad = 0;
    for (uint64_t x = lo; x < hi; x++) {
        if (lg_adam_local_row((uint32_t)x, rcp, thr) != (uint32_t)(x / row_len)) {
            if (bad == 0) *first_bad = x;
            bad++;
        }
    }
    return bad;
}

// the span that starts at span * LG_ADAM_SPAN: its first row and the offset inside it; then the row of element k of the span
int64_t h_adam_first_row(int64_t span, uint32_t row_len, uint32_t* rem) { return lg_adam_first_row(span * (int64_t)LG_ADAM_SPAN, row_len, rem); }

int64_t h_adam_row_of(int64_t span, uint32_t k, uint32_t row_len)
{
    uint32_t rem;
    const int64_t first = lg_adam_first_row(span * (int64_t)LG_ADAM_SPAN, row_len, &rem);
    return first + lg_adam_local_row(rem + k, lg_adam_row_rcp(row_len), lg_adam_row_thr(row_len));
}
}
