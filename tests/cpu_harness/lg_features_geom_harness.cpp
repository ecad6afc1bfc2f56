// CPU harness around lg_feature_bwd_step (lightgaussian_amd/csrc/lg_math.h), the per-pixel step of lg_features_bwd_geom.
// Test infrastructure: compiled with g++ (-ffp-contract=off).  It projects the Gaussians with the product's lg_project, builds the
// per-tile lists (tight rectangles, depth order, ties by id), runs lg_feature_step front to back per pixel (final T, last
// contributing list position) and then lg_feature_bwd_step back to front, as the kernel does.  The six moments are summed per Gaussian
// in float64 and chained to the inputs with the product's own lg_rows_to_grads, lg_backward_geom and lg_backward_cov3d, the way
// lg_math_harness.cpp::h_backward_geom does, so that tests/test_features_geom_host.py can compare the geometry gradient of a loss on
// the feature image and on alpha with the oracle's without a GPU.
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

// one step on caller-held state; m: 6 floats (accumulated into).  Returns 1 when the entry contributed.
int h_feature_bwd_step(int live, float power, float G, float alpha, float dx, float dy, float q, float Tfb, float* T, float* S, float* m, float* w)
{
    return lg_feature_bwd_step<true>(live != 0, power, G, alpha, dx, dy, q, Tfb, *T, *S, m, *w) ? 1 : 0;
}

// features [N][C], bg [C] or NULL, dL_dout [C][H][W] or NULL, dL_dalpha [H][W] or NULL.  Outputs (zeroed here): dmeans2D [N][3],
// dmeans3D [N][3], dopacity [N], dscales [N][3], drots [N][4]; out [C][H][W] and alpha_out [H][W] (the forward, for the caller's checks);
// radii [N].  early[0] = number of pixels whose walk ended (T (1 - alpha) < 1e-4) before the end of their tile's list.
// Returns the number of (tile, Gaussian) instances.
long long h_features_geom(int N, int C, int W, int H, const float* means3D, const float* opacities, const float* scales, const float* rotations,
                          const float* vm, const float* pm, float tanfovx, float tanfovy, const float* features, const float* bg,
                          const float* dL_dout, const float* dL_dalpha, float* out, float* alpha_out, int* radii, float* dmeans2D,
                          float* dmeans3D, float* dopacity, float* dscales, float* drots, long long* early)
{
    struct Splat { LgSplat s; float op; float cov[6]; int vis; };
    std::vector<Splat> sp(N);
    const int gx = (W + LG_TILE - 1) / LG_TILE, gy = (H + LG_TILE - 1) / LG_TILE;
    for (int i = 0; i < N; i++) {
        sp[i].vis = 0; radii[i] = 0;
        lg_cov3d(scales + 3 * i, 1.0f, rotations + 4 * i, sp[i].cov);
        sp[i].op = opacities[i];
        if (!lg_project(vm, pm, means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2], sp[i].cov, sp[i].op, W, H, tanfovx, tanfovy, sp[i].s)) continue;
        sp[i].vis = 1; radii[i] = sp[i].s.radius;
    }
    struct Inst { uint64_t key; uint32_t id; };
    std::vector<Inst> inst;
    for (int i = 0; i < N; i++) {
        if (!sp[i].vis) continue;
        const LgSplat& s = sp[i].s;
        for (int y = s.ty0; y < s.ty1; y++)
            for (int x = s.tx0; x < s.tx1; x++) inst.push_back({((uint64_t)(y * gx + x) << 32) | lg_f2bits(s.depth), (uint32_t)i});
    }
    std::stable_sort(inst.begin(), inst.end(), [](const Inst& a, const Inst& b) { return a.key < b.key; });
    std::vector<uint32_t> lo(gx * gy, 0), hi(gx * gy, 0);
    for (size_t k = 0; k < inst.size(); k++) {
        const uint32_t t = (uint32_t)(inst[k].key >> 32);
        if (k == 0 || t != (uint32_t)(inst[k - 1].key >> 32)) lo[t] = (uint32_t)k;
        hi[t] = (uint32_t)k + 1;
    }
    std::vector<double> mom((size_t)N * 6, 0.0);
    std::vector<float> F(C), g(C);
    const size_t HW = (size_t)H * W;
    long long n_early = 0;
    for (int pyi = 0; pyi < H; pyi++)
        for (int pxi = 0; pxi < W; pxi++) {
            const int t = (pyi / LG_TILE) * gx + pxi / LG_TILE;
            const size_t pid = (size_t)pyi * W + pxi;
            // forward: what the colour forward leaves per pixel (final T, position of the last contributor), and the maps
            float T = 1.0f, A = 0.0f;
            uint32_t last = 0;
            std::fill(F.begin(), F.end(), 0.0f);
            for (uint32_t k = lo[t]; k < hi[t]; k++) {
                const Splat& h = sp[inst[k].id];
                float dx, dy, w = 0.0f;
                const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                const int res = lg_feature_step(power, lg_alpha_exact(h.op, power), T, w);
                if (res == 2) { if (k + 1 < hi[t]) n_early++; break; }
                if (res == 0) continue;
                last = k - lo[t] + 1;
                A = fmaf(1.0f, w, A);
                const float* f = features + (size_t)inst[k].id * C;
                for (int c = 0; c < C; c++) F[c] = fmaf(f[c], w, F[c]);
            }
            for (int c = 0; c < C; c++) out[c * HW + pid] = bg ? fmaf(T, bg[c], F[c]) : F[c];
            alpha_out[pid] = A;
            // backward: back to front from the last contributor
            float bgdot = 0.0f;
            for (int c = 0; c < C; c++) {
                g[c] = dL_dout ? dL_dout[c * HW + pid] : 0.0f;
                if (bg) bgdot = fmaf(bg[c], g[c], bgdot);
            }
            const float gA = dL_dalpha ? dL_dalpha[pid] : 0.0f;
            const float Tfb = T * bgdot;
            float S = 0.0f;
            for (uint32_t k = hi[t]; k-- > lo[t];) {
                const Splat& h = sp[inst[k].id];
                float dx, dy, w = 0.0f;
                const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                const float G = lg_exp(fminf(power, 0.0f));
                const float alpha = lg_alpha_exact(h.op, power);
                float q = gA;
                const float* f = features + (size_t)inst[k].id * C;
                for (int c = 0; c < C; c++) q = fmaf(f[c], g[c], q);
                float m[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                if (!lg_feature_bwd_step<true>(k - lo[t] + 1 <= last, power, G, alpha, dx, dy, q, Tfb, T, S, m, w)) continue;
                for (int v = 0; v < 6; v++) mom[(size_t)inst[k].id * 6 + v] += (double)m[v];
            }
        }
    if (early) early[0] = n_early;
    for (int i = 0; i < N; i++) {
        for (int k = 0; k < 3; k++) { dmeans2D[3 * i + k] = 0; dmeans3D[3 * i + k] = 0; dscales[3 * i + k] = 0; }
        for (int k = 0; k < 4; k++) drots[4 * i + k] = 0;
        dopacity[i] = 0;
        if (!(radii[i] > 0)) continue;
        float m9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, acc[9];
        for (int v = 0; v < 6; v++) m9[v] = (float)mom[(size_t)i * 6 + v];
        const LgSplat& s = sp[i].s;
        lg_rows_to_grads(m9, s.ha, s.nb, s.hc, sp[i].op, acc);
        LgGradOut go;
        lg_backward_geom(vm, pm, means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2], sp[i].cov, acc, W, H, tanfovx, tanfovy, go);
        lg_backward_cov3d(scales + 3 * i, 1.0f, rotations + 4 * i, go.cov3D, dscales + 3 * i, drots + 4 * i);
        dmeans2D[3 * i] = go.mean2D[0]; dmeans2D[3 * i + 1] = go.mean2D[1];
        for (int k = 0; k < 3; k++) dmeans3D[3 * i + k] = go.mean3D[k];
        dopacity[i] = acc[5];
    }
    return (long long)inst.size();
}
}
