// CPU harness around the 3D smoothing filter's per-camera term of lightgaussian_amd/csrc/lg_math.h (lg_filter3d_camera,
// lg_filter3d_term, lg_filter3d_value): the text lg_filter3d_update_kernel compiles, walked in the kernel's order.  Test
// infrastructure: compiled with g++ (-ffp-contract=off, -mfma: fmaf is the hardware instruction, one rounding).
#include <cmath>
#include <cstdint>
#include "../../lightgaussian_amd/csrc/lg_math.h"

extern "C" {

// cameras: V records of 20 floats {viewmatrix[16], tanfovx, tanfovy, (float) width, (float) height}.
// t [N][V], seen_nv [N][V]: the per-pair term and decision (either may be null).
// filter [N], seen [N]: what lg_filter3d_update leaves -- sqrtf(0.2f) min t over the seeing cameras; an unseen row gets the maximum over
// the seen rows, or 0 when no row is seen.
void h_filter3d(int N, const float* means, int V, const float* cameras, float* t, uint8_t* seen_nv, float* filter, uint8_t* seen)
{
    float best = -1.0f;
    for (int i = 0; i < N; i++) {
        const float px = means[3 * i], py = means[3 * i + 1], pz = means[3 * i + 2];
        float tmin = INFINITY;
        bool any = false;
        for (int n = 0; n < V; n++) {
            const float* c = cameras + 20 * n;
            LgFilterCam cam;
            lg_filter3d_camera(c, c[16], c[17], (int)c[18], (int)c[19], cam);
            float tn;
            const bool s = lg_filter3d_term(cam, px, py, pz, tn);
            if (t) t[(size_t)i * V + n] = tn;
            if (seen_nv) seen_nv[(size_t)i * V + n] = s ? 1 : 0;
            if (s) { any = true; tmin = tn < tmin ? tn : tmin; }
        }
        const float f = any ? lg_filter3d_value(tmin) : -1.0f;
        filter[i] = f;
        seen[i] = any ? 1 : 0;
        best = fmaxf(best, f);
    }
    const float fill = best < 0.0f ? 0.0f : best;
    for (int i = 0; i < N; i++)
        if (filter[i] < 0.0f) filter[i] = fill;
}

}  // extern "C"
