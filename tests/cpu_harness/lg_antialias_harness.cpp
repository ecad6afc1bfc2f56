// CPU harness around the antialiasing arithmetic of lightgaussian_amd/csrc/lg_math.h (LG_FLAG_ANTIALIAS): lg_aa_ratio / lg_aa_rho,
// lg_project_t, lg_backward_geom_t and lg_backward_camera_terms_t.  Test infrastructure: compiled with g++ (-ffp-contract=off).
// The blend-stage sums are INPUTS (acc[0..5] per Gaussian: d/d pixel mean, d/d conic, d/d compensated opacity), so that
// tests/test_antialias_host.py can compare the outputs with float64 autograd of a functional that is linear in the quantities those
// sums are gradients of.  `mode`: 1 = the antialiased instantiations, 0 = the <false> instantiations, 2 = the functions that existed
// before the mode did (lg_project, lg_backward_geom, lg_backward_camera_terms): 0 and 2 must give the same bits.
#include <cmath>
#include <cstdint>
#include "../../lightgaussian_amd/csrc/lg_math.h"

namespace {

float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// K1's / K9's covariance of Gaussian i (lg_preprocess.h: lg_k9_cov3d): the precomputed input, or from the scales / rotation, RAW ones
// activated with exactly the kernels' operations.  sc, q, qn: what K9's chain rule needs afterwards.
void cov3d_of(int i, int raw, const float* scales, const float* rotations, const float* cov3D, float S[6], float sc[3], float q[4], float& qn)
{
    qn = 1.0f;
    if (cov3D) {
        for (int k = 0; k < 6; k++) S[k] = cov3D[6 * i + k];
        return;
    }
    for (int k = 0; k < 3; k++) sc[k] = scales[3 * i + k];
    for (int k = 0; k < 4; k++) q[k] = rotations[4 * i + k];
    if (raw) {
        for (int k = 0; k < 3; k++) sc[k] = expf(sc[k]);
        qn = fmaxf(sqrtf((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3])), 1e-12f);
        for (int k = 0; k < 4; k++) q[k] /= qn;
    }
    lg_cov3d(sc, 1.0f, q, S);
}

}  // namespace

extern "C" {

// rho of n blurred-covariance triples given by their unblurred entries (a0, b, c0); the blur is added here as lg_cov2d adds it.
void h_aa_rho(int n, const float* a0, const float* b, const float* c0, float* rho)
{
    for (int i = 0; i < n; i++) rho[i] = lg_aa_rho(lg_aa_ratio(a0[i], b[i], c0[i], a0[i] + 0.3f, c0[i] + 0.3f));
}

// rho of every Gaussian of a view, from the inputs, with K1's own operations (lg_ewa, lg_cov2d); 1 for Gaussians at or behind the
// near plane (they are never projected).
void h_aa_rho_scene(int N, int raw, int W, int H, const float* means3D, const float* scales, const float* rotations, const float* cov3D,
                    const float* vm, float tanfovx, float tanfovy, float* rho)
{
    const float fx = (float)W / (2.0f * tanfovx), fy = (float)H / (2.0f * tanfovy);
    for (int i = 0; i < N; i++) {
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        const float vx = vm[0] * px + vm[4] * py + vm[8] * pz + vm[12];
        const float vy = vm[1] * px + vm[5] * py + vm[9] * pz + vm[13];
        const float vz = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
        rho[i] = 1.0f;
        if (!(vz > 0.2f)) continue;
        float S[6], sc[3], q[4], qn;
        cov3d_of(i, raw, scales, rotations, cov3D, S, sc, q, qn);
        LgEwa e;
        lg_ewa(vm, vx, vy, vz, fx, fy, 1.3f * tanfovx, 1.3f * tanfovy, e);
        LgCov2D c2;
        lg_cov2d(e.T2, S, c2);
        rho[i] = lg_aa_rho(lg_aa_ratio(c2.a0, c2.b, c2.c0, c2.a, c2.c));
    }
}

// lg_project of every Gaussian.  out [N][16]: visible, radius, reference rectangle (4), tight rectangle (4), x, y, ha, nb, hc, and
// the opacity K1 writes into the blend record.
void h_aa_project(int mode, int N, int W, int H, const float* means3D, const float* scales, const float* rotations, const float* opacities,
                  const float* vm, const float* pm, float tanfovx, float tanfovy, float* out)
{
    for (int i = 0; i < N; i++) {
        float S[6], sc[3], q[4], qn;
        cov3d_of(i, 0, scales, rotations, nullptr, S, sc, q, qn);
        LgSplat sp;
        float op_rec = opacities[i];
        bool vis;
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        if (mode == 2) vis = lg_project(vm, pm, px, py, pz, S, opacities[i], W, H, tanfovx, tanfovy, sp);
        else if (mode == 1) vis = lg_project_t<true>(vm, pm, px, py, pz, S, opacities[i], W, H, tanfovx, tanfovy, sp, op_rec);
        else { float unused = 0.0f; vis = lg_project_t<false>(vm, pm, px, py, pz, S, opacities[i], W, H, tanfovx, tanfovy, sp, unused); }
        float* o = out + 16 * i;
        for (int k = 0; k < 16; k++) o[k] = 0.0f;
        if (!vis) continue;
        o[0] = 1.0f; o[1] = (float)sp.radius;
        o[2] = (float)sp.rx0; o[3] = (float)sp.ry0; o[4] = (float)sp.rx1; o[5] = (float)sp.ry1;
        o[6] = (float)sp.tx0; o[7] = (float)sp.ty0; o[8] = (float)sp.tx1; o[9] = (float)sp.ty1;
        o[10] = sp.x; o[11] = sp.y; o[12] = sp.ha; o[13] = sp.nb; o[14] = sp.hc; o[15] = op_rec;
    }
}

// K9's per-Gaussian chain with acc6 [N][6] = (acc[0..4], dL/dop') handed in.  raw: the inputs are log-scales, unnormalised
// rotations and opacity logits.  Outputs: dmean [N][3], dscale [N][3], drot [N][4] (or dcov [N][6] with cov3D), dop [N].
// Gaussians at or behind the near plane get zeros (invisible lanes).
void h_aa_backward(int mode, int N, int raw, int W, int H, const float* means3D, const float* scales, const float* rotations,
                   const float* cov3D, const float* opacities, const float* acc6, const float* vm, const float* pm, float tanfovx,
                   float tanfovy, float* dmean, float* dscale, float* drot, float* dcov, float* dop, int* vis)
{
    for (int i = 0; i < N; i++) {
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        for (int k = 0; k < 3; k++) { dmean[3 * i + k] = 0.0f; if (dscale) dscale[3 * i + k] = 0.0f; }
        if (drot) for (int k = 0; k < 4; k++) drot[4 * i + k] = 0.0f;
        if (dcov) for (int k = 0; k < 6; k++) dcov[6 * i + k] = 0.0f;
        dop[i] = 0.0f; vis[i] = 0;
        const float vz = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
        if (!(vz > 0.2f)) continue;
        vis[i] = 1;
        float S[6], sc[3], q[4], qn;
        cov3d_of(i, raw, scales, rotations, cov3D, S, sc, q, qn);
        const float* a6 = acc6 + 6 * i;
        const float acc[9] = { a6[0], a6[1], a6[2], a6[3], a6[4], a6[5], 0.0f, 0.0f, 0.0f };
        const float op = raw ? sigmoid(opacities[i]) : opacities[i];
        LgGradOut go;
        float rho = 1.0f;
        if (mode == 2) lg_backward_geom(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, go);
        else if (mode == 1) lg_backward_geom_t<true>(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, go, op, rho);
        else lg_backward_geom_t<false>(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, go, op, rho);
        for (int k = 0; k < 3; k++) dmean[3 * i + k] = go.mean3D[k];
        float d = mode == 1 ? rho * acc[5] : acc[5];
        if (cov3D) {
            for (int k = 0; k < 6; k++) dcov[6 * i + k] = go.cov3D[k];
        } else {
            float ds[3], dr[4];
            lg_backward_cov3d(sc, 1.0f, q, go.cov3D, ds, dr);
            if (raw) {      // K9's chain through exp and normalize (lg_preprocess_bwd)
                ds[0] *= sc[0]; ds[1] *= sc[1]; ds[2] *= sc[2];
                const float qg = q[0] * dr[0] + q[1] * dr[1] + q[2] * dr[2] + q[3] * dr[3];
                const float inv = 1.0f / qn;
                for (int k = 0; k < 4; k++) dr[k] = (dr[k] - q[k] * qg) * inv;
            }
            for (int k = 0; k < 3; k++) dscale[3 * i + k] = ds[k];
            for (int k = 0; k < 4; k++) drot[4 * i + k] = dr[k];
        }
        if (raw) d = d * op * (1.0f - op);
        dop[i] = d;
    }
}

// The 27 camera sums (packed layout of LG_CAM_TERMS, summed in double) with colours as inputs (no view-direction term).
void h_aa_camera_terms(int mode, int N, int W, int H, const float* means3D, const float* scales, const float* rotations,
                       const float* opacities, const float* acc6, const float* vm, const float* pm, float tanfovx, float tanfovy, double* sums)
{
    for (int k = 0; k < LG_CAM_TERMS; k++) sums[k] = 0.0;
    for (int i = 0; i < N; i++) {
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        const float vz = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
        if (!(vz > 0.2f)) continue;
        float S[6], sc[3], q[4], qn;
        cov3d_of(i, 0, scales, rotations, nullptr, S, sc, q, qn);
        const float* a6 = acc6 + 6 * i;
        const float acc[9] = { a6[0], a6[1], a6[2], a6[3], a6[4], a6[5], 0.0f, 0.0f, 0.0f };
        const float d[3] = { 0.0f, 0.0f, 0.0f };
        float term[LG_CAM_TERMS];
        if (mode == 2) lg_backward_camera_terms(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, d, term);
        else if (mode == 1) lg_backward_camera_terms_t<true>(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, d, term, opacities[i]);
        else lg_backward_camera_terms_t<false>(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, d, term, opacities[i]);
        for (int k = 0; k < LG_CAM_TERMS; k++) sums[k] += (double)term[k];
    }
}

}
