// CPU build of the product's normals arithmetic (lightgaussian_amd/csrc/lg_math.h, the functions lg_normals.h's kernels call), for
// tests/test_normals_host.py and tests/test_gpu_normals.py.  Compiled with -ffp-contract=off -mfma: the bits are the device's.
// The image loops visit every pixel on its own and gather its four neighbours exactly as the kernels do.
#include "../../lightgaussian_amd/csrc/lg_math.h"

static inline float at(const float* d, int x, int y, int W, int H)        // clamped like the kernels' loads: such a value is never used
{
    x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x); y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
    return d[(size_t)y * W + x];
}
struct Rays { float rx, rxm, rxp, ry, rym, ryp; };
static inline Rays rays(int x, int y, int W, int H, float tx, float ty)
{
    return { lg_pixel_ray(x, W, tx), lg_pixel_ray(x - 1, W, tx), lg_pixel_ray(x + 1, W, tx), lg_pixel_ray(y, H, ty), lg_pixel_ray(y - 1, H, ty),
             lg_pixel_ray(y + 1, H, ty) };
}
static inline void pixel(const float* d, int x, int y, int W, int H, float tx, float ty, LgDepthNormal& o, Rays& r)
{
    r = rays(x, y, W, H, tx, ty);
    lg_depth_normal(at(d, x, y, W, H), at(d, x, y - 1, W, H), at(d, x, y + 1, W, H), at(d, x - 1, y, W, H), at(d, x + 1, y, W, H), r.rx, r.rxm, r.rxp, r.ry, r.rym, r.ryp, o);
    if (!(x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2)) { o.ok = false; o.n[0] = o.n[1] = o.n[2] = 0.0f; }
}

extern "C" {

void h_normal_rows(int N, const float* xyz, const float* scaling, const float* rotation, const float* vm, float* rows, int* axis, float* sign)
{
    for (int i = 0; i < N; i++) {
        lg_normal_row(vm, xyz + 3 * i, scaling + 3 * i, rotation + 4 * i, rows + 4 * i);
        LgNormalRow o;
        lg_normal_view(vm, xyz + 3 * i, scaling + 3 * i, rotation + 4 * i, o);
        if (axis) axis[i] = o.k;
        if (sign) sign[i] = o.s;
    }
}

void h_normal_rows_bwd(int N, const float* xyz, const float* scaling, const float* rotation, const float* vm, const float* g, float* d_xyz, float* d_rot)
{
    for (int i = 0; i < N; i++) lg_normal_row_bwd(vm, xyz + 3 * i, scaling + 3 * i, rotation + 4 * i, g + 4 * i, d_xyz + 3 * i, d_rot + 4 * i);
}

void h_depth_normals(int H, int W, const float* depth, float tx, float ty, float* nd)
{
    const size_t plane = (size_t)H * W;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            LgDepthNormal o; Rays r;
            pixel(depth, x, y, W, H, tx, ty, o, r);
            for (int k = 0; k < 3; k++) nd[k * plane + (size_t)y * W + x] = o.n[k];
        }
}

// taps of pixel q for the upstream G(q): g is dL/dN_d [3,H,W] (nr == NULL) or formed from the loss (nr, alpha, weight, scale)
static LgNormalTaps taps(int H, int W, const float* depth, float tx, float ty, int x, int y, const float* g, const float* nr, const float* alpha,
                         const float* weight, float scale)
{
    LgNormalTaps t = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (x < 0 || x >= W || y < 0 || y >= H) return t;
    const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
    LgDepthNormal o; Rays r;
    pixel(depth, x, y, W, H, tx, ty, o, r);
    float G[3];
    if (nr) {
        float w = alpha[p];
        if (weight) w = w * weight[p];
        const float coef = -(scale * w);
        for (int k = 0; k < 3; k++) G[k] = coef * nr[k * plane + p];
    } else {
        for (int k = 0; k < 3; k++) G[k] = g[k * plane + p];
    }
    lg_depth_normal_bwd(o, G, r.rx, r.rxm, r.rxp, r.ry, r.rym, r.ryp, t);
    return t;
}

void h_depth_normals_bwd(int H, int W, const float* depth, float tx, float ty, const float* g, float* d_depth)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            d_depth[(size_t)y * W + x] = lg_depth_grad(taps(H, W, depth, tx, ty, x, y - 1, g, nullptr, nullptr, nullptr, 0.0f).down,
                                                       taps(H, W, depth, tx, ty, x, y + 1, g, nullptr, nullptr, nullptr, 0.0f).up,
                                                       taps(H, W, depth, tx, ty, x - 1, y, g, nullptr, nullptr, nullptr, 0.0f).right,
                                                       taps(H, W, depth, tx, ty, x + 1, y, g, nullptr, nullptr, nullptr, 0.0f).left);
}

// the loss in double over the float32 per-pixel terms (the device's partial sums are float32: the scalar is compared by tolerance)
double h_normal_loss(int H, int W, const float* nr, const float* depth, const float* alpha, const float* weight, float tx, float ty)
{
    const size_t plane = (size_t)H * W;
    double sum = 0.0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            LgDepthNormal o; Rays r;
            pixel(depth, x, y, W, H, tx, ty, o, r);
            float w = alpha[p];
            if (weight) w = w * weight[p];
            const float n[3] = { nr[p], nr[plane + p], nr[2 * plane + p] };
            sum += (double)lg_normal_term(w, n, o.n);
        }
    return sum / ((double)H * W);
}

void h_normal_loss_bwd(int H, int W, const float* nr, const float* depth, const float* alpha, const float* weight, float tx, float ty, float g_loss,
                       float* d_nr, float* d_depth)
{
    const size_t plane = (size_t)H * W;
    const float scale = g_loss * (float)(1.0 / ((double)H * W));
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            LgDepthNormal o; Rays r;
            pixel(depth, x, y, W, H, tx, ty, o, r);
            float w = alpha[p];
            if (weight) w = w * weight[p];
            const float coef = -(scale * w);
            for (int k = 0; k < 3; k++) d_nr[k * plane + p] = coef * o.n[k];
            d_depth[p] = lg_depth_grad(taps(H, W, depth, tx, ty, x, y - 1, nullptr, nr, alpha, weight, scale).down,
                                       taps(H, W, depth, tx, ty, x, y + 1, nullptr, nr, alpha, weight, scale).up,
                                       taps(H, W, depth, tx, ty, x - 1, y, nullptr, nr, alpha, weight, scale).right,
                                       taps(H, W, depth, tx, ty, x + 1, y, nullptr, nr, alpha, weight, scale).left);
        }
}

}
