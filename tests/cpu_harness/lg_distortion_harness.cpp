// CPU harness around lg_distortion_step / lg_distortion_bwd_step (lightgaussian_amd/csrc/lg_math.h), the per-pixel steps of
// lg_distortion_fwd / lg_distortion_bwd (lg_distortion.h).  Test infrastructure: compiled with g++ (-ffp-contract=off).
//   h_distortion_step       one forward step on caller-held state
//   h_distortion_ray        one ray of n entries with given alphas (power 0, G = 1: alpha is the opacity) and m: lg_feature_step +
//                           lg_distortion_step front to back, then lg_distortion_bwd_step back to front; moment 5 of an entry is dL/dalpha
//   h_distortion_view       a whole view the way the kernels walk it: lg_project, the per-tile lists (tight rectangles, depth order, ties
//                           by id), per pixel the forward and the back-to-front replay, and the kernels' own summation ORDER -- the 64
//                           lanes of an 8 x 8 block as wave_reduce_via_lds adds them (quarters of 16 as a balanced tree, then (q0 + q1) +
//                           (q2 + q3)), the four blocks of a tile in order (only those with a contributing pixel), a Gaussian's instances
//                           in slot order from zero (lg_features_gather, K9's lane gather), then lg_rows_to_grads / lg_backward_geom /
//                           lg_backward_cov3d as K9 applies them -- so that tests/test_gpu_distortion.py can ask for the same BITS.
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../lightgaussian_amd/csrc/lg_math.h"

static float tree16(const float* c)
{
    return (((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]))) + (((c[8] + c[9]) + (c[10] + c[11])) + ((c[12] + c[13]) + (c[14] + c[15])));
}
static float wave_sum(const float* lanes) { return (tree16(lanes) + tree16(lanes + 16)) + (tree16(lanes + 32) + tree16(lanes + 48)); }

extern "C" {

// st: A, P1, P2, D, c, med
void h_distortion_step(float w, float Tin, float m, uint32_t pos, float* st, uint32_t* med_pos)
{
    LgDistortion s = { st[0], st[1], st[2], st[3], st[4], st[5], *med_pos };
    lg_distortion_step(w, Tin, m, pos, s);
    st[0] = s.A; st[1] = s.P1; st[2] = s.P2; st[3] = s.D; st[4] = s.c; st[5] = s.med; *med_pos = s.med_pos;
}

// out: D, median, final T; med_pos; w [n] (0 for entries that did not contribute); dalpha [n], dm [n] of gD D + gM median.
// Returns the number of contributors.
int h_distortion_ray(int n, const float* alpha, const float* m, float gD, float gM, float* out, uint32_t* med_pos, float* w, float* dalpha, float* dm)
{
    LgDistortion s = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u };
    float T = 1.0f;
    uint32_t last = 0;
    int cnt = 0;
    for (int k = 0; k < n; k++) {
        w[k] = dalpha[k] = dm[k] = 0.0f;
    }
    for (int k = 0; k < n; k++) {
        const float Tin = T;
        float wk = 0.0f;
        const int res = lg_feature_step(0.0f, alpha[k], T, wk);
        if (res == 2) break;
        if (res == 0) continue;
        w[k] = wk; last = (uint32_t)k + 1u; cnt++;
        lg_distortion_step(wk, Tin, m[k], (uint32_t)k + 1u, s);
    }
    out[0] = s.D; out[1] = s.med; out[2] = T; *med_pos = s.med_pos;
    float S = 0.0f;
    for (int k = n - 1; k >= 0; k--) {
        float mom[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, d = 0.0f;
        if (!lg_distortion_bwd_step<true>((uint32_t)k + 1u <= last, 0.0f, 1.0f, alpha[k], 0.0f, 0.0f, m[k], (uint32_t)k + 1u, s, gD, gM, T, S, mom, d)) continue;
        dalpha[k] = mom[5]; dm[k] = d;
    }
    return cnt;
}

// m [N] with stride m_stride floats; gD, gM [H][W] or NULL.  Outputs: D, median [H][W]; radii [N]; dm [N]; dmeans2D [N][3], dmeans3D [N][3],
// dopacity [N], dscales [N][3], drots [N][4].  info[0] = the longest tile list, info[1] = pixels that ended before their list did,
// info[2] = pixels whose median is not their last contributor.  Returns the number of (tile, Gaussian) instances.
long long h_distortion_view(int N, int W, int H, const float* means3D, const float* opacities, const float* scales, const float* rotations,
                            const float* vm, const float* pm, float tanfovx, float tanfovy, const float* m, int m_stride, const float* gD,
                            const float* gM, float* D, float* median, int* radii, float* dm, float* dmeans2D, float* dmeans3D, float* dopacity,
                            float* dscales, float* drots, long long* info)
{
    struct Splat { LgSplat s; float op; float cov[6]; int vis; uint32_t slot0; };
    std::vector<Splat> sp(N);
    const int gx = (W + LG_TILE - 1) / LG_TILE, gy = (H + LG_TILE - 1) / LG_TILE;
    uint32_t nslots = 0;
    for (int i = 0; i < N; i++) {
        sp[i].vis = 0; radii[i] = 0; sp[i].slot0 = nslots;
        lg_cov3d(scales + 3 * i, 1.0f, rotations + 4 * i, sp[i].cov);
        sp[i].op = opacities[i];
        if (!lg_project(vm, pm, means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2], sp[i].cov, sp[i].op, W, H, tanfovx, tanfovy, sp[i].s)) continue;
        sp[i].vis = 1; radii[i] = sp[i].s.radius;
        nslots += (uint32_t)((sp[i].s.ty1 - sp[i].s.ty0) * (sp[i].s.tx1 - sp[i].s.tx0));
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
    std::vector<float> rows((size_t)nslots * 7, 0.0f);      // per pre-sort slot: the six moments and dm
    long long longest = 0, n_early = 0, n_mid = 0;
    for (int ty = 0; ty < gy; ty++)
        for (int tx = 0; tx < gx; tx++) {
            const int t = ty * gx + tx;
            const uint32_t n_list = hi[t] - lo[t];
            longest = std::max<long long>(longest, n_list);
            // per (entry, block, lane): the seven partials of the pixel; per (entry, block): whether a pixel took the entry
            std::vector<float> p((size_t)n_list * 4 * 7 * 64, 0.0f);
            std::vector<uint8_t> took((size_t)n_list * 4, 0);
            for (int sub = 0; sub < 4; sub++)
                for (int lane = 0; lane < 64; lane++) {
                    const int pxi = tx * LG_TILE + (sub & 1) * 8 + (lane & 7), pyi = ty * LG_TILE + (sub >> 1) * 8 + (lane >> 3);
                    if (pxi >= W || pyi >= H) continue;
                    const size_t pid = (size_t)pyi * W + pxi;
                    float T = 1.0f;
                    uint32_t last = 0;
                    LgDistortion s = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u };
                    for (uint32_t k = lo[t]; k < hi[t]; k++) {
                        const Splat& h = sp[inst[k].id];
                        float dx, dy, w = 0.0f;
                        const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                        const float Tin = T;
                        const int res = lg_feature_step(power, lg_alpha_exact(h.op, power), T, w);
                        if (res == 2) { if (k + 1 < hi[t]) n_early++; break; }
                        if (res == 0) continue;
                        last = k - lo[t] + 1;
                        lg_distortion_step(w, Tin, m[(size_t)inst[k].id * m_stride], last, s);
                    }
                    D[pid] = s.D; median[pid] = s.med;
                    if (s.med_pos != last) n_mid++;
                    const float g_d = gD ? gD[pid] : 0.0f, g_m = gM ? gM[pid] : 0.0f;
                    float S = 0.0f;
                    for (uint32_t k = hi[t]; k-- > lo[t];) {
                        const Splat& h = sp[inst[k].id];
                        float dx, dy;
                        const float power = lg_pair_power(h.s.x, h.s.y, h.s.ha, h.s.nb, h.s.hc, (float)pxi, (float)pyi, dx, dy);
                        const float G = lg_exp(fminf(power, 0.0f));
                        const float alpha = lg_alpha_exact(h.op, power);
                        const uint32_t e = k - lo[t];
                        float v[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                        if (!lg_distortion_bwd_step<true>(e + 1 <= last, power, G, alpha, dx, dy, m[(size_t)inst[k].id * m_stride], e + 1, s, g_d, g_m, T, S, v, v[6]))
                            continue;
                        took[(size_t)e * 4 + sub] = 1;
                        for (int r = 0; r < 7; r++) p[(((size_t)e * 4 + sub) * 7 + r) * 64 + lane] = v[r];
                    }
                }
            for (uint32_t e = 0; e < n_list; e++) {
                const uint32_t id = inst[lo[t] + e].id;
                const LgSplat& s = sp[id].s;
                const uint32_t slot = sp[id].slot0 + (uint32_t)((ty - s.ty0) * (s.tx1 - s.tx0) + (tx - s.tx0));
                for (int r = 0; r < 7; r++) {
                    float tot = 0.0f;
                    for (int sub = 0; sub < 4; sub++)
                        if (took[(size_t)e * 4 + sub]) tot += wave_sum(&p[(((size_t)e * 4 + sub) * 7 + r) * 64]);
                    rows[(size_t)slot * 7 + r] = tot;
                }
            }
        }
    info[0] = longest; info[1] = n_early; info[2] = n_mid;
    for (int i = 0; i < N; i++) {
        for (int k = 0; k < 3; k++) { dmeans2D[3 * i + k] = 0; dmeans3D[3 * i + k] = 0; dscales[3 * i + k] = 0; }
        for (int k = 0; k < 4; k++) drots[4 * i + k] = 0;
        dopacity[i] = 0; dm[i] = 0;
        if (!sp[i].vis) continue;
        const LgSplat& s = sp[i].s;
        const uint32_t n = (uint32_t)((s.ty1 - s.ty0) * (s.tx1 - s.tx0));
        float m9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, acc[9], d = 0.0f;
        for (uint32_t j = 0; j < n; j++) {
            const float* r = &rows[(size_t)(sp[i].slot0 + j) * 7];
            for (int v = 0; v < 6; v++) m9[v] += r[v];
            d += r[6];
        }
        dm[i] = d;
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
