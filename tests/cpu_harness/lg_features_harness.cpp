// CPU harness around lg_feature_step (lightgaussian_amd/csrc/lg_math.h), the per-pixel step of lg_blend_features.
// Test infrastructure: compiled with g++ (-ffp-contract=off).  It projects the Gaussians with the product's lg_project, builds the
// per-tile lists (tight rectangles, depth order, ties by id) and blends C feature channels per pixel front to back exactly as
// lg_features_fwd does -- lg_pair_power, lg_alpha_exact, lg_feature_step, F_c = fmaf(f_c, w, F_c), alpha as a channel of ones,
// out_c = fmaf(T, bg_c, F_c) -- so that tests/test_features_host.py can pin whole images against the oracle without a GPU.
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

int h_feature_step(float power, float alpha, float* T, float* w) { return lg_feature_step(power, alpha, *T, *w); }

// features [N][C], bg [C] or NULL, out [C][H][W], alpha [H][W], radii [N]; dL_dout [C][H][W] and dF [N][C] (double, zeroed here) or NULL:
// dF[j][c] = sum over pixels of w dL_dout, the gradient lg_blend_features_backward computes.  Returns the number of (tile, Gaussian) instances.
long long h_blend_features(int N, int C, int W, int H, const float* means3D, const float* opacities, const float* scales, const float* rotations,
                           const float* vm, const float* pm, float tanfovx, float tanfovy, const float* features, const float* bg, float* out,
                           float* alpha_out, int* radii, const float* dL_dout, double* dF)
{
    if (dF) std::fill(dF, dF + (size_t)N * C, 0.0);
    struct Splat { LgSplat s; float op; int vis; };
    std::vector<Splat> sp(N);
    const int gx = (W + LG_TILE - 1) / LG_TILE, gy = (H + LG_TILE - 1) / LG_TILE;
    for (int i = 0; i < N; i++) {
        sp[i].vis = 0; radii[i] = 0;
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        float cov[6];
        lg_cov3d(scales + 3 * i, 1.0f, rotations + 4 * i, cov);
        sp[i].op = opacities[i];
        if (!lg_project(vm, pm, px, py, pz, cov, sp[i].op, W, H, tanfovx, tanfovy, sp[i].s)) continue;
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
    std::vector<float> F(C);
    const size_t HW = (size_t)H * W;
    for (int pyi = 0; pyi < H; pyi++)
        for (int pxi = 0; pxi < W; pxi++) {
            const int t = (pyi / LG_TILE) * gx + pxi / LG_TILE;
            float T = 1.0f, A = 0.0f;
            std::fill(F.begin(), F.end(), 0.0f);
            for (uint32_t k = lo[t]; k < hi[t]; k++) {
                const Splat& h = sp[inst[k].id];
                float dx, dy, w = 0.0f;
                const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                const int res = lg_feature_step(power, lg_alpha_exact(h.op, power), T, w);
                if (res == 2) break;
                if (res == 0) continue;
                A = fmaf(1.0f, w, A);
                const float* f = features + (size_t)inst[k].id * C;
                for (int c = 0; c < C; c++) F[c] = fmaf(f[c], w, F[c]);
                if (dF)
                    for (int c = 0; c < C; c++) dF[(size_t)inst[k].id * C + c] += (double)w * dL_dout[c * HW + (size_t)pyi * W + pxi];
            }
            const size_t pid = (size_t)pyi * W + pxi;
            for (int c = 0; c < C; c++) out[c * HW + pid] = bg ? fmaf(T, bg[c], F[c]) : F[c];
            alpha_out[pid] = A;
        }
    return (long long)inst.size();
}
}
