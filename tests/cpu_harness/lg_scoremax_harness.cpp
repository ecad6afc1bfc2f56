// CPU harness of the per-hit significance weights and their two reductions (lightgaussian_amd/csrc/lg_math.h): the reference of
// LG_FLAG_SCORE_MAX, for which oracle/ has no counterpart.  Test infrastructure: compiled with g++ (-ffp-contract=off).  As
// lg_features_harness.cpp it projects the Gaussians with the product's lg_project (lg_project_t<true> with the antialias switch: the
// compensated opacity of the blend record), builds the per-tile lists ordered by (tile, depth bits, id) and walks every pixel front to
// back with lg_pair_power / lg_alpha_exact / lg_feature_step.  Per Gaussian it returns the hit count, the LARGEST alpha and the largest
// alpha T of any hit (plain fp32 values of single hits: nothing is rounded), and the Q24.40 integer sums of the same per-hit values --
// the quantity the oracle's W_ALPHA / W_ALPHA_T scores are lg_fix40_score of, which is how tests/test_scoremax_host.py ties the
// per-hit values maximised here to the oracle's.
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

float h_fix40_to_score(uint64_t q) { return lg_fix40_score(q); }

// count [N], max_alpha [N], max_alpha_t [N], sum_alpha [N], sum_alpha_t [N] (Q24.40), radii [N].  Returns the number of (tile, Gaussian) instances.
long long h_score_max(int N, int W, int H, int antialias, const float* means3D, const float* opacities, const float* scales, const float* rotations,
                      const float* vm, const float* pm, float tanfovx, float tanfovy, int* count, float* max_alpha, float* max_alpha_t,
                      uint64_t* sum_alpha, uint64_t* sum_alpha_t, int* radii)
{
    struct Splat { LgSplat s; float op; int vis; };
    std::vector<Splat> sp(N);
    const int gx = (W + LG_TILE - 1) / LG_TILE, gy = (H + LG_TILE - 1) / LG_TILE;
    for (int i = 0; i < N; i++) {
        sp[i].vis = 0; radii[i] = 0; count[i] = 0;
        max_alpha[i] = max_alpha_t[i] = 0.0f;
        sum_alpha[i] = sum_alpha_t[i] = 0;
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        float cov[6];
        lg_cov3d(scales + 3 * i, 1.0f, rotations + 4 * i, cov);
        sp[i].op = opacities[i];
        bool vis;
        if (antialias) vis = lg_project_t<true>(vm, pm, px, py, pz, cov, opacities[i], W, H, tanfovx, tanfovy, sp[i].s, sp[i].op);
        else vis = lg_project(vm, pm, px, py, pz, cov, opacities[i], W, H, tanfovx, tanfovy, sp[i].s);
        if (!vis) continue;
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
    std::vector<uint32_t> lo((size_t)gx * gy, 0), hi((size_t)gx * gy, 0);
    for (size_t k = 0; k < inst.size(); k++) {
        const uint32_t t = (uint32_t)(inst[k].key >> 32);
        if (k == 0 || t != (uint32_t)(inst[k - 1].key >> 32)) lo[t] = (uint32_t)k;
        hi[t] = (uint32_t)k + 1;
    }
    for (int pyi = 0; pyi < H; pyi++)
        for (int pxi = 0; pxi < W; pxi++) {
            const int t = (pyi / LG_TILE) * gx + pxi / LG_TILE;
            float T = 1.0f;
            for (uint32_t k = lo[t]; k < hi[t]; k++) {
                const uint32_t id = inst[k].id;
                const Splat& h = sp[id];
                float dx, dy, w = 0.0f;
                const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                const float alpha = lg_alpha_exact(h.op, power);
                const int res = lg_feature_step(power, alpha, T, w);      // w = alpha T (T before the hit)
                if (res == 2) break;
                if (res == 0) continue;
                count[id]++;
                max_alpha[id] = std::max(max_alpha[id], alpha);
                max_alpha_t[id] = std::max(max_alpha_t[id], w);
                sum_alpha[id] += lg_fix40_quant(alpha);
                sum_alpha_t[id] += lg_fix40_quant(w);
            }
        }
    return (long long)inst.size();
}
}
