// CPU harness around the sensitivity pieces of lightgaussian_amd/csrc/lg_math.h (lg_sensitivity_step, lg_sensitivity_moments_to_M,
// lg_sensitivity_AtMA, lg_sensitivity_logdet), the arithmetic of lg_sensitivity.h's kernels.  Test infrastructure: compiled with g++
// (-ffp-contract=off).
//   h_sens_ray      one pixel under n entries given as blend records: lg_feature_step front to back, lg_sensitivity_step back to front;
//                   the twelve moments of every entry
//   h_sens_block    H[21] += A^T M A of one Gaussian from its summed moments, as lg_sensitivity_accum builds it
//   h_sens_logdet   lg_sensitivity_logdet
//   h_sens_view     a whole view the way the kernels walk it: lg_project, the per-tile lists (tight rectangles, depth order, ties by id),
//                   per pixel the forward and the back-to-front replay, a Gaussian's moments summed in float64, then h_sens_block
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

// rec [n][9]: x, y, ha, nb, hc, opacity, r, g, b.  mom [n][12] (zeros for entries that did not contribute).  Returns the number of
// contributors; *T_final = the transmittance behind the last one.
int h_sens_ray(int n, const float* rec, float pxf, float pyf, const float* bg, float* mom, float* T_final)
{
    float T = 1.0f;
    int last = 0, cnt = 0;
    for (int k = 0; k < n; k++) {
        const float* r = rec + 9 * k;
        float dx, dy, w = 0.0f;
        const float power = lg_pair_power(r[0], r[1], r[2], r[3], r[4], pxf, pyf, dx, dy);
        const int res = lg_feature_step(power, lg_alpha_exact(r[5], power), T, w);
        if (res == 2) break;
        if (res == 0) continue;
        last = k + 1; cnt++;
    }
    *T_final = T;
    const float Tfb[3] = { T * bg[0], T * bg[1], T * bg[2] };
    float S[3] = { 0.0f, 0.0f, 0.0f };
    for (int k = n - 1; k >= 0; k--) {
        const float* r = rec + 9 * k;
        float dx, dy;
        const float power = lg_pair_power(r[0], r[1], r[2], r[3], r[4], pxf, pyf, dx, dy);
        const float G = lg_exp(fminf(power, 0.0f));
        const float alpha = lg_alpha_exact(r[5], power);
        float* m = mom + 12 * k;
        for (int v = 0; v < 12; v++) m[v] = 0.0f;
        lg_sensitivity_step<true>(k + 1 <= last, power, G, alpha, dx, dy, r + 6, Tfb, T, S, m);
    }
    return cnt;
}

static void block(const double* mo, float ha, float nb, float hc, float op, const float* vm, const float* pm, const float* xyz, const float* sc,
                  const float* rot, int W, int H, float tanfovx, float tanfovy, double* Hout)
{
    float cov[6];
    lg_cov3d(sc, 1.0f, rot, cov);
    double M[15];
    lg_sensitivity_moments_to_M(mo, ha, nb, hc, op, M);
    float A[5][6];
    for (int k = 0; k < 5; k++) {
        float acc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        acc[k] = 1.0f;
        LgGradOut go;
        float dsc[3], drot[4];
        lg_backward_geom(vm, pm, xyz[0], xyz[1], xyz[2], cov, acc, W, H, tanfovx, tanfovy, go);
        lg_backward_cov3d(sc, 1.0f, rot, go.cov3D, dsc, drot);
        for (int j = 0; j < 3; j++) { A[k][j] = go.mean3D[j]; A[k][3 + j] = dsc[j]; }
    }
    lg_sensitivity_AtMA(A, M, Hout);
}

void h_sens_block(const double* mo, float ha, float nb, float hc, float op, const float* vm, const float* pm, const float* xyz, const float* sc,
                  const float* rot, int W, int H, float tanfovx, float tanfovy, double* Hout)
{
    block(mo, ha, nb, hc, op, vm, pm, xyz, sc, rot, W, H, tanfovx, tanfovy, Hout);
}

double h_sens_logdet(const double* H) { return lg_sensitivity_logdet(H); }

// colors [N][3]; Hout [N][21] is ADDED to.  radii [N].  info[0] = the longest tile list, info[1] = pixels that ended before their list did.
// Returns the number of (tile, Gaussian) instances.
long long h_sens_view(int N, int W, int H, const float* means3D, const float* opacities, const float* scales, const float* rotations,
                      const float* colors, const float* bg, const float* vm, const float* pm, float tanfovx, float tanfovy, int* radii, double* Hout, long long* info)
{
    struct Splat { LgSplat s; float op; int vis; };
    std::vector<Splat> sp(N);
    const int gx = (W + LG_TILE - 1) / LG_TILE, gy = (H + LG_TILE - 1) / LG_TILE;
    for (int i = 0; i < N; i++) {
        float cov[6];
        sp[i].vis = 0; radii[i] = 0;
        lg_cov3d(scales + 3 * i, 1.0f, rotations + 4 * i, cov);
        sp[i].op = opacities[i];
        if (!lg_project(vm, pm, means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2], cov, sp[i].op, W, H, tanfovx, tanfovy, sp[i].s)) continue;
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
    long long longest = 0, n_early = 0;
    for (int t = 0; t < gx * gy; t++) longest = std::max<long long>(longest, hi[t] - lo[t]);
    std::vector<double> mo((size_t)N * 12, 0.0);
    std::vector<uint8_t> has(N, 0);
    for (size_t k = 0; k < inst.size(); k++) has[inst[k].id] = 1;
    for (int pyi = 0; pyi < H; pyi++)
        for (int pxi = 0; pxi < W; pxi++) {
            const int t = (pyi / LG_TILE) * gx + pxi / LG_TILE;
            float T = 1.0f;
            uint32_t last = 0;
            for (uint32_t k = lo[t]; k < hi[t]; k++) {
                const Splat& h = sp[inst[k].id];
                float dx, dy, w = 0.0f;
                const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                const int res = lg_feature_step(power, lg_alpha_exact(h.op, power), T, w);
                if (res == 2) { if (k + 1 < hi[t]) n_early++; break; }
                if (res == 0) continue;
                last = k - lo[t] + 1;
            }
            const float Tfb[3] = { T * bg[0], T * bg[1], T * bg[2] };
            float S[3] = { 0.0f, 0.0f, 0.0f };
            for (uint32_t k = hi[t]; k-- > lo[t];) {
                const uint32_t id = inst[k].id;
                const Splat& h = sp[id];
                float dx, dy;
                const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                const float G = lg_exp(fminf(power, 0.0f));
                const float alpha = lg_alpha_exact(h.op, power);
                float m[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
                if (!lg_sensitivity_step<true>(k - lo[t] + 1 <= last, power, G, alpha, dx, dy, colors + 3 * id, Tfb, T, S, m)) continue;
                for (int v = 0; v < 12; v++) mo[(size_t)id * 12 + v] += (double)m[v];
            }
        }
    for (int i = 0; i < N; i++) {
        if (!has[i]) continue;
        const LgSplat& s = sp[i].s;
        block(&mo[(size_t)i * 12], s.ha, s.nb, s.hc, sp[i].op, vm, pm, means3D + 3 * i, scales + 3 * i, rotations + 4 * i, W, H, tanfovx, tanfovy,
              Hout + 21 * (size_t)i);
    }
    info[0] = longest; info[1] = n_early;
    return (long long)inst.size();
}
}
