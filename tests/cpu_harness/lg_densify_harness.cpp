// CPU harness around the PRODUCT's densification math (lightgaussian_amd/csrc/lg_math.h: lg_densify_child_xyz,
// lg_densify_child_scaling), row by row as lg_densify_move evaluates it, for tests/test_densify_host.py.
// Test infrastructure, compiled with g++ (-ffp-contract=off); no GPU.
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

// n children: raw rows of their parents and one unit-normal noise row each
void h_densify_children(int n, const float* xyz, const float* scaling, const float* rotation, const float* noise, float* out_xyz,
                        float* out_scaling)
{
    for (int i = 0; i < n; i++) {
        const float s[3] = { expf(scaling[3 * i]), expf(scaling[3 * i + 1]), expf(scaling[3 * i + 2]) };
        lg_densify_child_xyz(rotation + 4 * i, s, noise + 3 * i, xyz + 3 * i, out_xyz + 3 * i);
        for (int c = 0; c < 3; c++) out_scaling[3 * i + c] = lg_densify_child_scaling(s[c]);
    }
}
}
