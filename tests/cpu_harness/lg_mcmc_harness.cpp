// CPU harness around the PRODUCT's 3DGS-MCMC math (lightgaussian_amd/csrc/lg_math.h: lg_mcmc_gate, lg_mcmc_noise_xyz,
// lg_mcmc_binomial_sum, lg_mcmc_relocate), row by row as the kernels of lg_mcmc.h evaluate it, for tests/test_mcmc_host.py.
// Test infrastructure, compiled with g++ (-ffp-contract=off); no GPU.
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

double h_mcmc_binomial_sum(double x, int M) { return lg_mcmc_binomial_sum(x, M); }

// n drawn rows: raw opacity and scaling, the number of draws of each
void h_mcmc_relocate(int n, const float* opacity, const float* scaling, const int* cnt, float min_opacity, float* out_opacity,
                     float* out_scaling)
{
    for (int i = 0; i < n; i++) lg_mcmc_relocate(opacity[i], scaling + 3 * i, cnt[i], min_opacity, out_opacity[i], out_scaling + 3 * i);
}

// n rows as lg_mcmc_noise_kernel steps them; gate_out: g c of each row
void h_mcmc_noise(int n, const float* xyz, const float* scaling, const float* rotation, const float* opacity, const float* noise, float c,
                  float k, float x0, float* out_xyz, float* gate_out)
{
    for (int i = 0; i < n; i++) {
        const float gate = lg_mcmc_gate(opacity[i], c, k, x0);
        gate_out[i] = gate;
        for (int a = 0; a < 3; a++) out_xyz[3 * i + a] = xyz[3 * i + a];
        if (gate == 0.0f) continue;
        const float s[3] = { expf(scaling[3 * i]), expf(scaling[3 * i + 1]), expf(scaling[3 * i + 2]) };
        lg_mcmc_noise_xyz(rotation + 4 * i, s, noise + 3 * i, gate, xyz + 3 * i, out_xyz + 3 * i);
    }
}
}
