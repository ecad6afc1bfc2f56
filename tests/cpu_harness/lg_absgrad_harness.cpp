// CPU harness around the absolute mean-gradient arithmetic of lightgaussian_amd/csrc/lg_math.h (LG_FLAG_ABSGRAD): lg_abs_pair, the two
// partial sums K7's ABS variants add per (pixel, Gaussian) pair, and lg_abs_rows_to_grad, which lg_absgrad_rows applies once per Gaussian.
// Test infrastructure: compiled with g++ (-ffp-contract=off); tests/test_absgrad_host.py compares the outputs with float64.
#include <cmath>
#include <cstdint>
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

// one pair each, accumulated from zero: out [n][2] = (|t (2 ha dx + nb dy)|, |t (2 hc dy + nb dx)|)
void h_abs_pair(int n, const float* t, const float* dx, const float* dy, const float* ha, const float* nb, const float* hc, float* out)
{
    for (int i = 0; i < n; i++) {
        float ax = 0.0f, ay = 0.0f;
        lg_abs_pair(t[i], dx[i], dy[i], ha[i], nb[i], hc[i], ax, ay);
        out[2 * i] = ax; out[2 * i + 1] = ay;
    }
}

// k pairs of ONE Gaussian accumulated in order: out [2]
void h_abs_pair_sum(int k, const float* t, const float* dx, const float* dy, float ha, float nb, float hc, float* out)
{
    float ax = 0.0f, ay = 0.0f;
    for (int i = 0; i < k; i++) lg_abs_pair(t[i], dx[i], dy[i], ha, nb, hc, ax, ay);
    out[0] = ax; out[1] = ay;
}

// out [n][3] = lg_abs_rows_to_grad(sx, sy, op, W, H)
void h_abs_rows_to_grad(int n, const float* sx, const float* sy, const float* op, int W, int H, float* out)
{
    for (int i = 0; i < n; i++) lg_abs_rows_to_grad(sx[i], sy[i], op[i], W, H, out + 3 * i);
}

// the SIGNED gradient of the same single pair as K7's moments and K9's lg_rows_to_grads give it: out [n][2] = acc[0], acc[1] (pixel units)
void h_pair_signed(int n, const float* t, const float* dx, const float* dy, const float* ha, const float* nb, const float* hc,
                   const float* op, float* out)
{
    for (int i = 0; i < n; i++) {
        const float tdx = t[i] * dx[i], tdy = t[i] * dy[i];
        const float m[9] = { tdx, tdy, tdx * dx[i], tdx * dy[i], tdy * dy[i], t[i], 0.0f, 0.0f, 0.0f };
        float acc[9];
        lg_rows_to_grads(m, ha[i], nb[i], hc[i], op[i], acc);
        out[2 * i] = acc[0]; out[2 * i + 1] = acc[1];
    }
}

}
