// CPU harness around lg_backward_camera_terms (lightgaussian_amd/csrc/lg_math.h), the per-Gaussian step of lg_camera_bwd.
// Test infrastructure: compiled with g++ (-ffp-contract=off).  The blend-stage sums are INPUTS here (acc[0..4] and dL/drgb per
// Gaussian), so that tests/test_camera_host.py can compare the 27 camera sums with float64 autograd of a functional that is linear in
// the quantities those sums are gradients of.  Per Gaussian, as the kernel: lg_cov3d, the SH direction Jacobian by the product's
// lg_sh_dir_jacobian, the view-direction term by lg_backward_sh_jac on a zeroed dmean with a no-op store, then the 27 terms, summed in
// double.  A Gaussian at or behind the 0.2 near plane contributes zeros (an invisible lane).  dmean [N][3]: lg_backward_geom's mean3D
// plus the direction term -- dL/dmeans3D as K9 returns it, for the translation identity.
#include <cstdint>
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

// acc5 [N][5], drgb [N][3], sh [N][16][3] (NULL: colours are inputs, no direction term).  sums [27] (packed layout of LG_CAM_TERMS),
// dmean [N][3], vis [N].  Returns the number of Gaussians that contributed.
int h_camera_terms(int N, int deg, int W, int H, const float* means3D, const float* scales, const float* rotations, const float* acc5,
                   const float* drgb, const float* sh, const float* vm, const float* pm, const float* campos, float tanfovx, float tanfovy,
                   double* sums, float* dmean, int* vis)
{
    for (int k = 0; k < LG_CAM_TERMS; k++) sums[k] = 0.0;
    int n = 0;
    for (int i = 0; i < N; i++) {
        const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
        dmean[3 * i] = dmean[3 * i + 1] = dmean[3 * i + 2] = 0.0f;
        vis[i] = 0;
        const float vz = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
        if (!(vz > 0.2f)) continue;
        vis[i] = 1; n++;
        float S[6];
        lg_cov3d(scales + 3 * i, 1.0f, rotations + 4 * i, S);
        float acc[9] = { acc5[5 * i], acc5[5 * i + 1], acc5[5 * i + 2], acc5[5 * i + 3], acc5[5 * i + 4], 0.0f,
                         drgb[3 * i], drgb[3 * i + 1], drgb[3 * i + 2] };
        float d[3] = { 0.0f, 0.0f, 0.0f };
        if (sh) {
            float J[9];
            lg_sh_dir_jacobian(deg, sh + 48 * i, px, py, pz, campos, J);
            lg_backward_sh_jac(deg, J, px, py, pz, campos, acc + 6, d, [](int, int, float) {});
        }
        float term[LG_CAM_TERMS];
        lg_backward_camera_terms(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, d, term);
        for (int k = 0; k < LG_CAM_TERMS; k++) sums[k] += (double)term[k];
        LgGradOut go;
        lg_backward_geom(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, go);
        for (int k = 0; k < 3; k++) dmean[3 * i + k] = go.mean3D[k] + d[k];
    }
    return n;
}

}
