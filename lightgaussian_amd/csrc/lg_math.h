// lg_math.h -- per-Gaussian / per-pair arithmetic of the MI355X rasterizer.
//
// Pure scalar float code, no wave intrinsics: the same functions are called from the gfx950
// kernels (lg_preprocess.h / lg_blend.h, compiled through lg_api.hip) and, compiled with g++ by tests/cpu_harness, from the CPU-side unit
// tests that pin them bit-for-bit against the oracle.  Everything that feeds a threshold test
// (power > 0, alpha < 1/255, T < 1e-4, tile rectangles) follows the CANONICAL OPERATION ORDER
// documented in DESIGN.md section 4: plain IEEE mul/add/div/sqrt with contraction disabled
// (-ffp-contract=off) and explicit fmaf() only where written.
//
// Replaces (reference interface): the un-vendored CUDA submodule
// submodules/compress-diff-gaussian-rasterization (.gitmodules:6-8); conventions anchored on
// utils/sh_utils.py:26-103, utils/general_utils.py:68-119, scene/cameras.py:70-85.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LG_HD __host__ __device__ __forceinline__
#else
#define LG_HD static inline
#endif

#define LG_TILE 16
#define LG_ALPHA_MIN (1.0f / 255.0f)
#define LG_T_MIN 0.0001f
#define LG_ALPHA_MAX 0.99f

enum { LG_W_ONE = 0, LG_W_OPACITY = 1, LG_W_ALPHA = 2, LG_W_ALPHA_T = 3 };

LG_HD float lg_bits2f(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }
LG_HD uint32_t lg_f2bits(float f) { union { uint32_t u; float f; } c; c.f = f; return c.u; }

// ---------------------------------------------------------------------------------------------
// Canonical exp for x <= 0: Cody-Waite reduction + Cephes degree-5 polynomial.  Only exactly
// rounded primitives, so CPU and GPU agree bitwise.  (The hardware v_exp_f32 is ~1 ulp but not
// reproducible on a CPU; it is used only by the non-exact "fast" blend variant.)
LG_HD float lg_exp(float x)
{
    x = fmaxf(x, -87.0f);
    float t = x * 1.44269504088896341f;
    float n = rintf(t);
    float r = fmaf(n, -0.693359375f, x);
    r = fmaf(n, 2.12194440e-4f, r);
    float r2 = r * r;
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    p = fmaf(p, r2, r);
    p = p + 1.0f;
    return p * lg_bits2f((uint32_t)((int)n + 127) << 23);
}

// ---------------------------------------------------------------------------------------------
// Q24.40 fixed point of the per-hit significance weights (LG_W_ALPHA / LG_W_ALPHA_T).
// lg_fix40_bits(w): bit pattern of (double) w + 4096.  For 0 <= w < 4096 the sum lies in [2^12, 2^13), where a double's unit in the
// last place is 2^-40: the IEEE addition rounds w to the nearest multiple of 2^-40 (ties to even) and the low 40 bits of the
// mantissa field are that multiple.  LG_FIX_MAGIC = bits(4096.0); bits - LG_FIX_MAGIC = round(w 2^40).
// lg_fix40_score(q): the per-view sum as fp32 -- ONE rounding (nearest even) of the integer, then an exact scaling by 2^-40.
#define LG_FIX_FRAC_BITS 40
#define LG_FIX_MAGIC 0x40B0000000000000ull
LG_HD uint64_t lg_fix40_bits(float w) { union { double d; uint64_t u; } c; c.d = (double)w + 4096.0; return c.u; }
LG_HD uint64_t lg_fix40_quant(float w) { return lg_fix40_bits(w) - LG_FIX_MAGIC; }
LG_HD float lg_fix40_score(uint64_t q) { return (float)q * 0x1p-40f; }

// ---------------------------------------------------------------------------------------------
// seqsum32(w, c): the float obtained by c sequential additions of w starting from 0 -- i.e. what
// c atomicAdd(float*, w) calls produce (all addends equal, so order independent).  O(#binades)
// instead of O(c): inside one binade every step adds the same multiple of the ulp, so the run
// of identical steps is applied as one exact integer multiply.  SURVEY.md section 8a-note.
LG_HD float lg_seqsum32(float w, uint32_t c)
{
    float s = 0.0f;
    if (!(w > 0.0f)) { // w <= 0 or NaN: plain loop semantics are trivial for 0; keep exact loop otherwise
        for (uint32_t k = 0; k < c; k++) s = s + w;
        return s;
    }
    while (c > 0) {
        // three real steps a -> b -> d; if all in one binade the increment (d - b) is the steady one
        float a = s + w; c--;
        if (a == s) return s; // stalled: every further add is a no-op
        s = a;
        if (c == 0) break;
        float b = a + w; c--;
        s = b;
        if (c == 0) break;
        float d = b + w; c--;
        s = d;
        if (c == 0) break;
        uint32_t ua = lg_f2bits(a), ub = lg_f2bits(b), ud = lg_f2bits(d);
        uint32_t e = ud >> 23;
        if ((ua >> 23) != e || (ub >> 23) != e) continue;       // crossed a binade: keep stepping
        uint32_t inc = ud - ub;                                    // steady increment in ulps
        if (inc == 0) return s;
        uint32_t top = (e << 23) | 0x7FFFFFu;                      // largest value of this binade
        uint32_t room = (top - ud) / inc;                          // steps that stay inside it
        uint32_t k = room < c ? room : c;
        s = lg_bits2f(ud + k * inc);
        c -= k;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------
// Rotation matrix of a unit quaternion q = (r, x, y, z), row-major.  The ONE copy: lg_cov3d, lg_backward_cov3d and
// lg_densify_child_xyz call it (build_rotation, utils/general_utils.py:84-107).
LG_HD void lg_quat_to_rot(const float q[4], float R[9])
{
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - r * z); R[2] = 2.0f * (x * z + r * y);
    R[3] = 2.0f * (x * y + r * z); R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - r * x);
    R[6] = 2.0f * (x * z - r * y); R[7] = 2.0f * (y * z + r * x); R[8] = 1.0f - 2.0f * (x * x + y * y);
}

// 3D covariance from (scale, quaternion): Sigma = (R S)(R S)^T packed (xx,xy,xz,yy,yz,zz).
LG_HD void lg_cov3d(const float s_in[3], float mod, const float q[4], float cov[6])
{
    float s0 = mod * s_in[0], s1 = mod * s_in[1], s2 = mod * s_in[2];
    float R[9];
    lg_quat_to_rot(q, R);
    float L00 = R[0] * s0, L01 = R[1] * s1, L02 = R[2] * s2;
    float L10 = R[3] * s0, L11 = R[4] * s1, L12 = R[5] * s2;
    float L20 = R[6] * s0, L21 = R[7] * s1, L22 = R[8] * s2;
    cov[0] = L00 * L00 + L01 * L01 + L02 * L02;
    cov[1] = L00 * L10 + L01 * L11 + L02 * L12;
    cov[2] = L00 * L20 + L01 * L21 + L02 * L22;
    cov[3] = L10 * L10 + L11 * L11 + L12 * L12;
    cov[4] = L10 * L20 + L11 * L21 + L12 * L22;
    cov[5] = L20 * L20 + L21 * L21 + L22 * L22;
}

struct LgEwa {
    float T2[6];     // J * Wrot, 2x3 row-major
    float txc, tyc;  // clamped view-space x, y
    int xclamp, yclamp;
};

LG_HD void lg_ewa(const float* vm, float tx, float ty, float tz, float fx, float fy, float limx, float limy, LgEwa& e)
{
    float txtz = tx / tz, tytz = ty / tz;
    e.xclamp = (txtz < -limx || txtz > limx);
    e.yclamp = (tytz < -limy || tytz > limy);
    float cx = fminf(limx, fmaxf(-limx, txtz)) * tz;
    float cy = fminf(limy, fmaxf(-limy, tytz)) * tz;
    e.txc = cx; e.tyc = cy;
    float J00 = fx / tz, J02 = -(fx * cx) / (tz * tz);
    float J11 = fy / tz, J12 = -(fy * cy) / (tz * tz);
    for (int k = 0; k < 3; k++) {
        e.T2[k] = J00 * vm[4 * k + 0] + J02 * vm[4 * k + 2];
        e.T2[3 + k] = J11 * vm[4 * k + 1] + J12 * vm[4 * k + 2];
    }
}

struct LgCov2D { float a, b, c, U[3], V[3]; float a0, c0; };   // a0, c0: the diagonal before the +0.3 blur (lg_aa_*)

LG_HD void lg_cov2d(const float* T2, const float* S, LgCov2D& o)
{
    o.U[0] = T2[0] * S[0] + T2[1] * S[1] + T2[2] * S[2];
    o.U[1] = T2[0] * S[1] + T2[1] * S[3] + T2[2] * S[4];
    o.U[2] = T2[0] * S[2] + T2[1] * S[4] + T2[2] * S[5];
    o.V[0] = T2[3] * S[0] + T2[4] * S[1] + T2[5] * S[2];
    o.V[1] = T2[3] * S[1] + T2[4] * S[3] + T2[5] * S[4];
    o.V[2] = T2[3] * S[2] + T2[4] * S[4] + T2[5] * S[5];
    float a = o.U[0] * T2[0] + o.U[1] * T2[1] + o.U[2] * T2[2];
    float b = o.U[0] * T2[3] + o.U[1] * T2[4] + o.U[2] * T2[5];
    float c = o.V[0] * T2[3] + o.V[1] * T2[4] + o.V[2] * T2[5];
    o.a = a + 0.3f; o.b = b; o.c = c + 0.3f;
    o.a0 = a; o.c0 = c;
}

// ---------------------------------------------------------------------------------------------
// Opacity compensation of the blur (LG_FLAG_ANTIALIAS; Mip-Splatting's 2D filter, the `antialiasing` switch of upstream 3DGS).  With
// (a0, b, c0) the 2D covariance before the blur and a = a0 + 0.3f, c = c0 + 0.3f (lg_cov2d's own sums):
//   det0 = a0 c0 - b b    det1 = a c - b b    x = det0 / det1    rho = sqrt(max(0.000025, x))    op' = op rho
// Canonical order (every product, difference, the division and the square root rounded on their own).  det1 == 0 is culled before
// (lg_project); det0 <= 0 (a rank-one covariance, rounding) and a NaN x fall to the floor through fmaxf.
#define LG_AA_FLOOR 0.000025f
LG_HD float lg_aa_ratio(float a0, float b, float c0, float a, float c)
{
    const float det0 = a0 * c0 - b * b;
    const float det1 = a * c - b * b;
    return det0 / det1;
}
LG_HD float lg_aa_rho(float x) { return sqrtf(fmaxf(LG_AA_FLOOR, x)); }
// Backward: gp = dL/dop' (acc[5] of lg_rows_to_grads).  Returns rho (dL/dop = rho gp) and ADDS gx dx/d(a0, b, c0) to the gradients of
// the blurred covariance entries (a, b, c differ from a0, b, c0 by constants; b counts as one variable, as dL_db does), with
// gx = dL/dx = op gp / (2 rho) above the floor and 0 at it.  The partials
//   dx/da0 = (c0 det1 - det0 c) / det1^2     dx/dc0 = (a0 det1 - det0 a) / det1^2     dx/db = -2 b (det1 - det0) / det1^2
// are evaluated in the form without the cancellation of two nearly equal products (h = 0.3: a = a0 + h, c = c0 + h):
//   c0 det1 - det0 c = h (c0 c + b b)        a0 det1 - det0 a = h (a0 a + b b)        det1 - det0 = h (a0 + c0) + h h
LG_HD float lg_aa_backward(float a0, float b, float c0, float a, float c, float op, float gp, float& dL_da, float& dL_db, float& dL_dc)
{
    const float det0 = a0 * c0 - b * b;
    const float det1 = a * c - b * b;
    const float x = det0 / det1;
    const float rho = lg_aa_rho(x);
    if (x > LG_AA_FLOOR) {
        const float gx = (op * gp) * 0.5f / rho;
        const float s = gx / (det1 * det1);
        const float bb = b * b;
        dL_da += s * (0.3f * (c0 * c + bb));
        dL_dc += s * (0.3f * (a0 * a + bb));
        dL_db += s * (-2.0f * b * (0.3f * (a0 + c0) + 0.09f));
    }
    return rho;
}

// The three steps lg_project_t (the first and the last; it keeps the second inline, see there) and both backward functions share (row-vector layout m[4 k + c], p = the mean).
// lg_view_point: v = p vm, the view-space mean.
LG_HD void lg_view_point(const float* vm, float px, float py, float pz, float& vx, float& vy, float& vz)
{
    vx = vm[0] * px + vm[4] * py + vm[8] * pz + vm[12];
    vy = vm[1] * px + vm[5] * py + vm[9] * pz + vm[13];
    vz = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
}
// lg_hom_point: h = p pm, columns 0 and 1, and m_w = 1 / (h_w + 1e-7) of column 3 (ndc = h_xy m_w).
LG_HD void lg_hom_point(const float* pm, float px, float py, float pz, float& hx, float& hy, float& m_w)
{
    hx = pm[0] * px + pm[4] * py + pm[8] * pz + pm[12];
    hy = pm[1] * px + pm[5] * py + pm[9] * pz + pm[13];
    const float hw = pm[3] * px + pm[7] * py + pm[11] * pz + pm[15];
    m_w = 1.0f / (hw + 0.0000001f);
}
// lg_focal: focal lengths in pixels.
LG_HD void lg_focal(int W, int H, float tanfovx, float tanfovy, float& fx, float& fy)
{
    fx = (float)W / (2.0f * tanfovx); fy = (float)H / (2.0f * tanfovy);
}

// Result of projecting one Gaussian (K1).
struct LgSplat {
    float x, y, depth;       // pixel-space mean, view-space z
    float ha, nb, hc;        // -0.5*A, -B, -0.5*C of the conic (exact rescalings)
    float hx, hy;            // conservative half-extent of the alpha >= 1/255 footprint (inf = no cull)
    int radius;
    int rx0, ry0, rx1, ry1;  // reference tile rectangle (max exclusive)
    int tx0, ty0, tx1, ty1;  // tight tile rectangle actually emitted (subset of the reference one)
};

// Projection + EWA splat + radius + tile rectangles.  Returns false when the Gaussian is not
// rasterised (near-culled, singular covariance, empty rectangle) -- radii must then be 0.
// AA (LG_FLAG_ANTIALIAS): the opacity is compensated for the blur (lg_aa_rho) in front of the footprint cull -- both the
// `opacity < 1/255: no instances` branch and the tau = log(255 opacity) extents see op' -- and returned in op_out for the blend
// record; the radius and the reference rectangle do not depend on it.  op_out is written only when AA, and only on `return true`.
template <bool AA>
LG_HD bool lg_project_t(const float* vm, const float* pm, float px, float py, float pz, const float* cov3D, float opacity,
                        int W, int H, float tanfovx, float tanfovy, LgSplat& o, float& op_out)
{
    float vx, vy, vz;
    lg_view_point(vm, px, py, pz, vx, vy, vz);
    if (vz <= 0.2f) return false;
    // (lg_hom_point's four lines, written out for K1: EXPERIMENTS 14)
    float hxm = pm[0] * px + pm[4] * py + pm[8] * pz + pm[12];
    float hym = pm[1] * px + pm[5] * py + pm[9] * pz + pm[13];
    float hwm = pm[3] * px + pm[7] * py + pm[11] * pz + pm[15];
    float p_w = 1.0f / (hwm + 0.0000001f);
    float ndcx = hxm * p_w, ndcy = hym * p_w;

    float fx, fy;
    lg_focal(W, H, tanfovx, tanfovy, fx, fy);
    LgEwa e;
    lg_ewa(vm, vx, vy, vz, fx, fy, 1.3f * tanfovx, 1.3f * tanfovy, e);
    LgCov2D c2;
    lg_cov2d(e.T2, cov3D, c2);
    const float a = c2.a, b = c2.b, c = c2.c;
    float det = a * c - b * b;
    if (det == 0.0f) return false;
    if (AA) { opacity = opacity * lg_aa_rho(lg_aa_ratio(c2.a0, b, c2.c0, a, c)); op_out = opacity; }
    float det_inv = 1.0f / det;
    float A = c * det_inv, B = -b * det_inv, C = a * det_inv;
    float mid = 0.5f * (a + c);
    float sq = sqrtf(fmaxf(0.1f, mid * mid - det));
    float l1 = mid + sq, l2 = mid - sq;
    float rad = ceilf(3.0f * sqrtf(fmaxf(l1, l2)));
    float ix = ((ndcx + 1.0f) * (float)W - 1.0f) * 0.5f;
    float iy = ((ndcy + 1.0f) * (float)H - 1.0f) * 0.5f;
    const int gx = (W + LG_TILE - 1) / LG_TILE, gy = (H + LG_TILE - 1) / LG_TILE;
    // the casts must not overflow for absurd coordinates: clamp the float first (no effect in range)
    const float big = 1.0e7f;
    int r0 = (int)fminf(big, fmaxf(-big, (ix - rad) / (float)LG_TILE));
    int r1 = (int)fminf(big, fmaxf(-big, (iy - rad) / (float)LG_TILE));
    int r2 = (int)fminf(big, fmaxf(-big, (ix + rad + (float)(LG_TILE - 1)) / (float)LG_TILE));
    int r3 = (int)fminf(big, fmaxf(-big, (iy + rad + (float)(LG_TILE - 1)) / (float)LG_TILE));
    o.rx0 = r0 < 0 ? 0 : (r0 > gx ? gx : r0);
    o.ry0 = r1 < 0 ? 0 : (r1 > gy ? gy : r1);
    o.rx1 = r2 < 0 ? 0 : (r2 > gx ? gx : r2);
    o.ry1 = r3 < 0 ? 0 : (r3 > gy ? gy : r3);
    if ((o.rx1 - o.rx0) * (o.ry1 - o.ry0) == 0) return false;
    o.x = ix; o.y = iy; o.depth = vz; o.radius = (int)rad;
    o.ha = -0.5f * A; o.nb = -B; o.hc = -0.5f * C;

    // ---- exact-conservative footprint culling (not part of the reference semantics: it only
    // removes (tile, Gaussian) instances every pixel of which would fail alpha >= 1/255) ----
    o.tx0 = o.rx0; o.ty0 = o.ry0; o.tx1 = o.rx1; o.ty1 = o.ry1;
    o.hx = INFINITY; o.hy = INFINITY;
    if (!(opacity >= LG_ALPHA_MIN)) {
        // alpha = min(0.99, opacity * exp(power<=0)) <= opacity < 1/255 everywhere: no instance needed
        if (opacity < LG_ALPHA_MIN) { o.tx1 = o.tx0; o.ty1 = o.ty0; o.hx = -1.0f; o.hy = -1.0f; }
        return true; // (NaN opacity: keep the full rectangle, behave like the reference)
    }
    float amp = (a * c) / det; // cancellation amplification of det, conic
    if (amp > 0.0f && amp < 100.0f && rad < 4096.0f) {
        float dmax = rad + (float)LG_TILE;
        float smax = (fabsf(o.ha) + fabsf(o.nb) + fabsf(o.hc)) * dmax * dmax;
        float tau = logf(opacity * 255.0f);
        float taup = (tau + 1.0e-6f * smax) * 1.00001f + 1.0e-4f;
        if (taup < 1.0e30f) {
            float hx = sqrtf(2.0f * taup * a) * 1.001f + 0.01f;
            float hy = sqrtf(2.0f * taup * c) * 1.001f + 0.01f;
            int t0 = (int)fminf(big, fmaxf(-big, ceilf((ix - hx - (float)(LG_TILE - 1)) / (float)LG_TILE)));
            int t1 = (int)fminf(big, fmaxf(-big, floorf((ix + hx) / (float)LG_TILE))) + 1;
            int u0 = (int)fminf(big, fmaxf(-big, ceilf((iy - hy - (float)(LG_TILE - 1)) / (float)LG_TILE)));
            int u1 = (int)fminf(big, fmaxf(-big, floorf((iy + hy) / (float)LG_TILE))) + 1;
            o.tx0 = t0 > o.rx0 ? t0 : o.rx0; o.tx1 = t1 < o.rx1 ? t1 : o.rx1;
            o.ty0 = u0 > o.ry0 ? u0 : o.ry0; o.ty1 = u1 < o.ry1 ? u1 : o.ry1;
            if (o.tx0 > o.rx1) o.tx0 = o.rx1; // footprint entirely beside the rectangle: empty, but keep it a sub-rectangle
            if (o.ty0 > o.ry1) o.ty0 = o.ry1;
            if (o.tx1 < o.tx0) o.tx1 = o.tx0;
            if (o.ty1 < o.ty0) o.ty1 = o.ty0;
            o.hx = hx; o.hy = hy;
        }
    }
    return true;
}
LG_HD bool lg_project(const float* vm, const float* pm, float px, float py, float pz, const float* cov3D, float opacity,
                      int W, int H, float tanfovx, float tanfovy, LgSplat& o)
{
    float unused;
    return lg_project_t<false>(vm, pm, px, py, pz, cov3D, opacity, W, H, tanfovx, tanfovy, o, unused);
}

// ---------------------------------------------------------------------------------------------
// SH -> RGB (utils/sh_utils.py:57-103 polynomial; +0.5 and clamp as gaussian_renderer/__init__.py:99)
#define LG_SH_C0 0.28209479177387814f
#define LG_SH_C1 0.4886025119029199f
#define LG_SH_C2_0 1.0925484305920792f
#define LG_SH_C2_1 -1.0925484305920792f
#define LG_SH_C2_2 0.31539156525252005f
#define LG_SH_C2_3 -1.0925484305920792f
#define LG_SH_C2_4 0.5462742152960396f
#define LG_SH_C3_0 -0.5900435899266435f
#define LG_SH_C3_1 2.890611442640554f
#define LG_SH_C3_2 -0.4570457994644658f
#define LG_SH_C3_3 0.3731763325901154f
#define LG_SH_C3_4 -0.4570457994644658f
#define LG_SH_C3_5 1.445305721320277f
#define LG_SH_C3_6 -0.5900435899266435f

// sh: [M][3] for this Gaussian.  Writes rgb (clamped at 0) and the clamp bits (bit c = channel c clamped).
LG_HD void lg_sh_to_rgb(int deg, const float* sh, float px, float py, float pz, const float* campos, float rgb[3],
                        uint32_t& clamp_bits)
{
    float dx = px - campos[0], dy = py - campos[1], dz = pz - campos[2];
    float len = sqrtf(dx * dx + dy * dy + dz * dz);
    dx = dx / len; dy = dy / len; dz = dz / len;
    clamp_bits = 0;
    for (int c = 0; c < 3; c++) {
        float res = LG_SH_C0 * sh[0 * 3 + c];
        if (deg > 0) {
            res = res - LG_SH_C1 * dy * sh[1 * 3 + c] + LG_SH_C1 * dz * sh[2 * 3 + c] - LG_SH_C1 * dx * sh[3 * 3 + c];
            if (deg > 1) {
                float xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = dx * dy, yz = dy * dz, xz = dx * dz;
                res = res + LG_SH_C2_0 * xy * sh[4 * 3 + c] + LG_SH_C2_1 * yz * sh[5 * 3 + c] +
                      LG_SH_C2_2 * (2.0f * zz - xx - yy) * sh[6 * 3 + c] + LG_SH_C2_3 * xz * sh[7 * 3 + c] +
                      LG_SH_C2_4 * (xx - yy) * sh[8 * 3 + c];
                if (deg > 2) {
                    res = res + LG_SH_C3_0 * dy * (3.0f * xx - yy) * sh[9 * 3 + c] + LG_SH_C3_1 * xy * dz * sh[10 * 3 + c] +
                          LG_SH_C3_2 * dy * (4.0f * zz - xx - yy) * sh[11 * 3 + c] +
                          LG_SH_C3_3 * dz * (2.0f * zz - 3.0f * xx - 3.0f * yy) * sh[12 * 3 + c] +
                          LG_SH_C3_4 * dx * (4.0f * zz - xx - yy) * sh[13 * 3 + c] +
                          LG_SH_C3_5 * dz * (xx - yy) * sh[14 * 3 + c] + LG_SH_C3_6 * dx * (xx - 3.0f * yy) * sh[15 * 3 + c];
                }
            }
        }
        float v = res + 0.5f;
        if (v < 0.0f) clamp_bits |= (1u << c);
        rgb[c] = fmaxf(v, 0.0f);
    }
}

// ---------------------------------------------------------------------------------------------
// The two expressions every include / exclude decision of the blend kernels rests on, written ONCE: the forward, count and
// backward pair steps of lg_blend.h all call them, and so does lg_blend_pair below, which tests/cpu_harness pins against the
// oracle -- a one-token slip here breaks bit parity on a handful of pixels per view.
// lg_pair_power: power = ha dx^2 + nb dx dy + hc dy^2 of the pixel (pxf, pyf) under the splat centred at (gx, gy), canonical order.
LG_HD float lg_pair_power(float gx, float gy, float ha, float nb, float hc, float pxf, float pyf, float& dx, float& dy)
{
    dx = gx - pxf; dy = gy - pyf;
    return fmaf(fmaf(ha, dx, nb * dy), dx, (hc * dy) * dy);
}
// lg_alpha_exact: the canonical alpha (lg_exp; the clamp of the power only matters for pairs that `power <= 0` rejects anyway)
LG_HD float lg_alpha_exact(float op, float power) { return fminf(LG_ALPHA_MAX, op * lg_exp(fminf(power, 0.0f))); }

// ---------------------------------------------------------------------------------------------
// Checkpoint records of long tiles (lists of more than one segment of S entries; ckpt / ckpt_last of BinView, lg_host.h): a
// record holds one word per pixel of a 16 x 16 tile, and record j of the tile whose list starts at entry `first` is
//   ckpt[lg_ckpt_base(first, S) + j * LG_CKPT_PIX + pixel]     (pixel = 16 row + column inside the tile)
// 2 floor(first / S) leaves room for the tile's ceil(n / S) records before the next long tile's, so 2 (R / S + 1) records hold
// any view of R instances (carve_bin).  The forward's writers and the backward's reader must agree on this to the word.
#define LG_CKPT_PIX (LG_TILE * LG_TILE)
LG_HD uint32_t lg_nseg(uint32_t n, uint32_t S) { return (n + S - 1u) / S; }                  // segments of a list of n entries
LG_HD size_t lg_ckpt_base(uint32_t first, uint32_t S) { return (size_t)2 * (first / S) * LG_CKPT_PIX; }
LG_HD size_t lg_ckpt_records(size_t R, size_t S) { return 2 * (R / S + 1); }

// ---------------------------------------------------------------------------------------------
// One (pixel, Gaussian) evaluation of the forward blend, canonical order.
// Returns 0 = rejected, 1 = contributes (T, C updated), 2 = pixel saturated (done).
template <bool EXACT>
LG_HD int lg_blend_pair(float gx, float gy, float ha, float nb, float hc, float op, float r, float g, float b, float pxf,
                        float pyf, float& T, float& C0, float& C1, float& C2, float& alpha_out)
{
    float dx, dy;
    const float power = lg_pair_power(gx, gy, ha, nb, hc, pxf, pyf, dx, dy);
    if (!(power <= 0.0f)) return 0;             // the kernels' test (a NaN power is rejected, as there)
#if defined(__HIP_DEVICE_COMPILE__)
    const float alpha = EXACT ? lg_alpha_exact(op, power) : fminf(LG_ALPHA_MAX, op * __expf(power));
#else
    const float alpha = lg_alpha_exact(op, power);
#endif
    if (alpha < LG_ALPHA_MIN) return 0;
    const float test_T = T * (1.0f - alpha);
    if (test_T < LG_T_MIN) return 2;
    const float w = alpha * T;
    C0 = fmaf(r, w, C0);
    C1 = fmaf(g, w, C1);
    C2 = fmaf(b, w, C2);
    T = test_T;
    alpha_out = alpha;
    return 1;
}

// ---------------------------------------------------------------------------------------------
// Feature blending (lg_features.h): the three tests of lg_blend_pair on a pair whose power (lg_pair_power) and alpha the caller has
// evaluated -- lg_alpha_exact in canonical mode, the guarded hardware exp of the forward otherwise -- without the three colour
// channels: the caller blends as many channels as it carries, F_c = fmaf(f_c, w, F_c), with the weight w = alpha T returned here.
// Returns 0 = rejected (w, T untouched), 1 = contributes (w set, T advanced), 2 = pixel saturated (done).
LG_HD int lg_feature_step(float power, float alpha, float& T, float& w)
{
    if (!(power <= 0.0f)) return 0;
    if (alpha < LG_ALPHA_MIN) return 0;
    const float test_T = T * (1.0f - alpha);
    if (test_T < LG_T_MIN) return 2;
    w = alpha * T;
    T = test_T;
    return 1;
}

// One (pixel, entry) step of the BACK-TO-FRONT replay of the feature blend (lg_features_bwd_geom, lg_features.h): the geometry
// gradient of  L(out_c = sum_j f[j][c] w_j + T_final bg_c,  alpha = sum_j w_j).  Per pixel, with g_c = dL/dout_c and gA = dL/dalpha:
//   q   = sum_c f[j][c] g_c + gA       the entry's own features projected on the pixel's gradient (alpha: a column of ones, background 0)
//   Tfb = T_final sum_c bg_c g_c       the background term
// and the state T (starts at the forward's final_T) and S (starts at 0: the projection on g of what lies behind the entry -- the
// published colour recurrence a <- a + alpha (c - a) is linear, so its projection obeys S <- S + alpha (q - S), as in K7's
// bwd_pair_fast).  The entry's power (lg_pair_power, with dx, dy), G = exp(power) and alpha come from the caller exactly as the forward
// evaluated them -- lg_exp / lg_alpha_exact in canonical mode, the guarded hardware exp otherwise -- and `live` says that the entry's
// list position is not behind the pixel's last contributor (n_contrib): the include / exclude decisions are the forward's.
//   inv = 1 / (1 - alpha);  Tn = T inv;  d = q - S;  dL/dalpha = d Tn - Tfb inv;  t = G dL/dalpha     (straight through the 0.99 clamp, as K7)
//   m[0..5] += t {dx, dy, dx dx, dx dy, dy dy, 1}      the moments lg_rows_to_grads reads (m[6..8], d/d rgb, are K7's alone)
//   w = alpha Tn  (the blending weight of the entry);  T = Tn;  S += alpha d
// Everything is linear in (g, gA): channel groups may be replayed separately, each with its own S and Tfb, and their moments add.
// Returns false (nothing touched) when the entry does not contribute.  EXACT = false on the device: v_rcp_f32 for inv, as K7's fast path.
template <bool EXACT>
LG_HD bool lg_feature_bwd_step(bool live, float power, float G, float alpha, float dx, float dy, float q, float Tfb, float& T, float& S,
                               float* m, float& w)
{
    if (!live || !(power <= 0.0f) || alpha < LG_ALPHA_MIN) return false;
#if defined(__HIP_DEVICE_COMPILE__)
    const float inv = EXACT ? 1.0f / (1.0f - alpha) : __builtin_amdgcn_rcpf(1.0f - alpha);
#else
    const float inv = 1.0f / (1.0f - alpha);
#endif
    const float Tn = T * inv;
    const float d = q - S;
    const float dL_dalpha = d * Tn - Tfb * inv;
    const float t = G * dL_dalpha;
    const float tdx = t * dx, tdy = t * dy;
    m[0] += tdx;
    m[1] += tdy;
    m[2] += tdx * dx;
    m[3] += tdx * dy;
    m[4] += tdy * dy;
    m[5] += t;
    w = alpha * Tn;
    T = Tn;
    S = S + alpha * d;
    return true;
}

// ---------------------------------------------------------------------------------------------
// Backward of the per-Gaussian stage (K8 + K9 fused).  acc = the 9 blend-stage sums:
//   [0,1] d/d(mean2D pixel x,y)  [2,3,4] d/d(conic A,B,C) (B: full derivative)  [5] d/d(opacity)  [6..8] d/d(rgb)
struct LgGradOut {
    float mean2D[2];   // NDC units
    float mean3D[3];
    float cov3D[6];
    float scale[3];
    float rot[4];
};

// Gradient rows of the backward blend hold pixel-offset MOMENTS (lg_blend.h): m[0..4] = sum t {dx, dy, dx^2, dx dy, dy^2},
// m[5] = sum t, with t = G dL/dalpha and dx = x_g - px; m[6..8] = dL/drgb.  The published per-pair expressions are linear in
// them with per-Gaussian coefficients (ha = -A/2, nb = -B, hc = -C/2 of the conic, opacity op), applied here once per Gaussian:
// acc = {dL/dmean2D.x, .y (pixel units), dL/dA, dL/dB, dL/dC, dL/dopacity, dL/drgb}, the input of lg_backward_geom.
LG_HD void lg_rows_to_grads(const float* m, float ha, float nb, float hc, float op, float* acc)
{
    acc[0] = op * (2.0f * ha * m[0] + nb * m[1]);
    acc[1] = op * (2.0f * hc * m[1] + nb * m[0]);
    acc[2] = -0.5f * op * m[2];
    acc[3] = -op * m[3];
    acc[4] = -0.5f * op * m[4];
    acc[5] = m[5];
    acc[6] = m[6]; acc[7] = m[7]; acc[8] = m[8];
}

// Absolute screen-space mean gradients (LG_FLAG_ABSGRAD, lg_backward_abs): sum over pixels of |dL/dmean2D| per Gaussian
// instead of the |sum| the moments give.  An absolute value does not pass through the moments' linearity, so the per-pair magnitudes are
// two more partial sums of K7's pair step (floats 9 and 10 of the gradient row), without the opacity, which is applied once per Gaussian:
//   ax += |t (2 ha dx + nb dy)|   ay += |t (2 hc dy + nb dx)|        t = G dL/dalpha, dx = x_g - px, as the moments
// lg_two_prod_sum(a, b, c, d) = a b + c d with ONE rounding of the sum's size (the product c d is carried with its rounding error, both
// fmas are exact in their products): the two terms have opposite signs wherever nb dx dy > 0 and cancel, and a plain mul + fma
// leaves an error of an ulp of the larger TERM there.  Two fmas more per component; only the ABS kernels run them.
LG_HD float lg_two_prod_sum(float a, float b, float c, float d)
{
    const float w = c * d;
    const float e = fmaf(c, d, -w);          // exact: c d = w + e
    return fmaf(a, b, w) + e;
}
LG_HD void lg_abs_pair(float t, float dx, float dy, float ha, float nb, float hc, float& ax, float& ay)
{
    ax += fabsf(t * lg_two_prod_sum(2.0f * ha, dx, nb, dy));
    ay += fabsf(t * lg_two_prod_sum(2.0f * hc, dy, nb, dx));
}
// ... finished per Gaussian: sx, sy = its rows' floats 9 and 10 summed in slot order, op = the record's opacity (the value
// lg_rows_to_grads multiplies by: the compensated one under LG_FLAG_ANTIALIAS).  NDC units, those of dL_dmeans2D (lg_backward_geom:
// mean2D = 0.5 {W, H} acc), so that out >= |dL_dmeans2D| component-wise up to rounding; z = 0.
LG_HD void lg_abs_rows_to_grad(float sx, float sy, float op, int W, int H, float* out)
{
    out[0] = (op * sx) * (0.5f * (float)W);
    out[1] = (op * sy) * (0.5f * (float)H);
    out[2] = 0.0f;
}

// The backward chain of one Gaussian from the blend-stage sums acc to dL/d(view-space mean): the ONE copy that lg_backward_geom_t (chains
// it on to the mean and the 3D covariance) and lg_backward_camera_terms_t (chains it to the camera) call.  In order: the view-space
// transform, lg_ewa and lg_cov2d; the conic -> (a, b, c) chain with its 1e-7 in d2inv; the antialias terms; dT = dL/d(T2 = J Wrot),
// dJ, and dt with the clamp convention (the clamped txc / tyc in dtz, zeroed dtx / dty on clamped lanes: the +-1.3 tanfov clamp passes
// no gradient).  A convention changes HERE, once.
// AA (LG_FLAG_ANTIALIAS): acc[5] is dL/dop' of the compensated opacity op' = op rho; op = the input opacity (activated).  The three
// terms of lg_aa_backward join dL_da, dL_db, dL_dc before they are chained on -- rho depends on the view matrix through T2 and the
// view-space mean as well --, and rho is kept so that the caller writes dL/dop = rho acc[5] (1 without AA).
struct LgBackChain {
    LgEwa e;
    LgCov2D c2;
    float fx, fy, vz;
    float gndx, gndy;                 // dL/d(ndc x, y)
    float dL_da, dL_db, dL_dc;
    float dT0[3], dT1[3];             // dL/d(T2 rows)
    float dtx, dty, dtz;
    float rho;
};
template <bool AA>
LG_HD void lg_backward_chain(const float* vm, float px, float py, float pz, const float* S /*cov3D*/, const float* acc, int W, int H,
                             float tanfovx, float tanfovy, float op, LgBackChain& k)
{
    float fx, fy;
    lg_focal(W, H, tanfovx, tanfovy, fx, fy);
    k.fx = fx; k.fy = fy;
    k.gndx = acc[0] * (0.5f * (float)W); k.gndy = acc[1] * (0.5f * (float)H);
    float vx, vy, vz;
    lg_view_point(vm, px, py, pz, vx, vy, vz);
    k.vz = vz;
    LgEwa& e = k.e;
    lg_ewa(vm, vx, vy, vz, fx, fy, 1.3f * tanfovx, 1.3f * tanfovy, e);
    LgCov2D& c2 = k.c2;
    lg_cov2d(e.T2, S, c2);
    const float a = c2.a, b = c2.b, c = c2.c;
    const float gA = acc[2], gB = acc[3], gC = acc[4];
    float denom = a * c - b * b;
    float d2inv = 1.0f / (denom * denom + 0.0000001f);
    float dL_da = 0.0f, dL_db = 0.0f, dL_dc = 0.0f;
    if (d2inv != 0.0f) {
        dL_da = d2inv * (-c * c * gA + b * c * gB + (denom - a * c) * gC);
        dL_dc = d2inv * (-a * a * gC + a * b * gB + (denom - a * c) * gA);
        dL_db = d2inv * (2.0f * b * c * gA - (denom + 2.0f * b * b) * gB + 2.0f * a * b * gC);
    }
    k.rho = 1.0f;
    if (AA) k.rho = lg_aa_backward(c2.a0, b, c2.c0, a, c, op, acc[5], dL_da, dL_db, dL_dc);
    k.dL_da = dL_da; k.dL_db = dL_db; k.dL_dc = dL_dc;
    const float* U = c2.U; const float* V = c2.V;
    float* dT0 = k.dT0; float* dT1 = k.dT1;
    for (int j = 0; j < 3; j++) {
        dT0[j] = 2.0f * dL_da * U[j] + dL_db * V[j];
        dT1[j] = dL_db * U[j] + 2.0f * dL_dc * V[j];
    }
    float dJ00 = dT0[0] * vm[0] + dT0[1] * vm[4] + dT0[2] * vm[8];
    float dJ02 = dT0[0] * vm[2] + dT0[1] * vm[6] + dT0[2] * vm[10];
    float dJ11 = dT1[0] * vm[1] + dT1[1] * vm[5] + dT1[2] * vm[9];
    float dJ12 = dT1[0] * vm[2] + dT1[1] * vm[6] + dT1[2] * vm[10];
    float tz = 1.0f / vz, tz2 = tz * tz, tz3 = tz2 * tz;
    k.dtx = (e.xclamp ? 0.0f : 1.0f) * (-fx * tz2 * dJ02);
    k.dty = (e.yclamp ? 0.0f : 1.0f) * (-fy * tz2 * dJ12);
    k.dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.0f * fx * e.txc) * tz3 * dJ02 + (2.0f * fy * e.tyc) * tz3 * dJ12;
}

// dL/d(mean2D, mean3D, cov3D) of one Gaussian: lg_backward_chain, then its own three steps -- the cov3D assembly from T2, dm = vm^T dt,
// and the projection term of the NDC gradient through the homogeneous divide.  rho_out is written only when AA.
template <bool AA>
LG_HD void lg_backward_geom_t(const float* vm, const float* pm, float px, float py, float pz, const float* S /*cov3D*/,
                              const float* acc, int W, int H, float tanfovx, float tanfovy, LgGradOut& g, float op, float& rho_out)
{
    LgBackChain k;
    lg_backward_chain<AA>(vm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, op, k);
    if (AA) rho_out = k.rho;
    const float gndx = k.gndx, gndy = k.gndy;
    g.mean2D[0] = gndx; g.mean2D[1] = gndy;
    const float* T2 = k.e.T2;
    const float dL_da = k.dL_da, dL_db = k.dL_db, dL_dc = k.dL_dc;
    g.cov3D[0] = T2[0] * T2[0] * dL_da + T2[0] * T2[3] * dL_db + T2[3] * T2[3] * dL_dc;
    g.cov3D[3] = T2[1] * T2[1] * dL_da + T2[1] * T2[4] * dL_db + T2[4] * T2[4] * dL_dc;
    g.cov3D[5] = T2[2] * T2[2] * dL_da + T2[2] * T2[5] * dL_db + T2[5] * T2[5] * dL_dc;
    g.cov3D[1] = 2.0f * T2[0] * T2[1] * dL_da + (T2[0] * T2[4] + T2[1] * T2[3]) * dL_db + 2.0f * T2[3] * T2[4] * dL_dc;
    g.cov3D[2] = 2.0f * T2[0] * T2[2] * dL_da + (T2[0] * T2[5] + T2[2] * T2[3]) * dL_db + 2.0f * T2[3] * T2[5] * dL_dc;
    g.cov3D[4] = 2.0f * T2[1] * T2[2] * dL_da + (T2[1] * T2[5] + T2[2] * T2[4]) * dL_db + 2.0f * T2[4] * T2[5] * dL_dc;
    const float dtx = k.dtx, dty = k.dty, dtz = k.dtz;
    float dmx = vm[0] * dtx + vm[1] * dty + vm[2] * dtz;
    float dmy = vm[4] * dtx + vm[5] * dty + vm[6] * dtz;
    float dmz = vm[8] * dtx + vm[9] * dty + vm[10] * dtz;
    {
        float hxm, hym, m_w;
        lg_hom_point(pm, px, py, pz, hxm, hym, m_w);
        float mul1 = hxm * m_w * m_w, mul2 = hym * m_w * m_w;
        dmx += (pm[0] * m_w - pm[3] * mul1) * gndx + (pm[1] * m_w - pm[3] * mul2) * gndy;
        dmy += (pm[4] * m_w - pm[7] * mul1) * gndx + (pm[5] * m_w - pm[7] * mul2) * gndy;
        dmz += (pm[8] * m_w - pm[11] * mul1) * gndx + (pm[9] * m_w - pm[11] * mul2) * gndy;
    }
    g.mean3D[0] = dmx; g.mean3D[1] = dmy; g.mean3D[2] = dmz;
}
LG_HD void lg_backward_geom(const float* vm, const float* pm, float px, float py, float pz, const float* S /*cov3D*/,
                            const float* acc, int W, int H, float tanfovx, float tanfovy, LgGradOut& g)
{
    float unused;
    lg_backward_geom_t<false>(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, g, 0.0f, unused);
}

// Camera terms of one Gaussian (lg_camera.h: lg_camera_bwd sums them over the visible Gaussians): what lg_backward_geom computes on
// its way to dL/dmean3D and drops -- dt = dL/d(view-space mean) through the EWA Jacobian, dT = dL/d(T2 = J Wrot), the J entries, the
// NDC gradient and the homogeneous divide -- chained to the camera instead of to the mean.  Row-vector layout m[4 k + c], p = the mean:
//   t_c = sum_k p_k vm[4k+c] + vm[12+c],  T2[0][k] = J00 vm[4k] + J02 vm[4k+2],  T2[1][k] = J11 vm[4k+1] + J12 vm[4k+2]
//     g_vm[4k+0] = p_k dtx + dT0k J00    g_vm[4k+1] = p_k dty + dT1k J11    g_vm[4k+2] = p_k dtz + dT0k J02 + dT1k J12    g_vm[12+c] = dt_c
//   h_c = sum_k p_k pm[4k+c] + pm[12+c] (c = 0, 1, 3),  ndc = h_xy / (h_w + 1e-7):  dh = (gndx m_w, gndy m_w, -(mul1 gndx + mul2 gndy))
//     g_pm[4k+c] = p_k dh_c              g_pm[12+c] = dh_c
//   g_cp = -d,  d = the view-direction term lg_backward_sh_jac adds to dmean (zeros for colors_precomp)
// out[27]: g_vm columns 0..2 of rows 0..3 (12), g_pm columns 0, 1, 3 of rows 0..3 (12), g_cp (3); column 3 of vm and column 2 of pm take
// no part in the forward.  Everything up to dtz is lg_backward_chain, the copy lg_backward_geom_t runs, and the homogeneous point is
// lg_hom_point: the two functions cannot drift apart.  AA: as in lg_backward_chain.
// In real arithmetic  dL/dmean3D = vm[:3,:3] g_vm[3,:3] + pm[:3,:] g_pm[3,:] - g_cp  (tests/test_camera_host.py).
#define LG_CAM_TERMS 27
template <bool AA>
LG_HD void lg_backward_camera_terms_t(const float* vm, const float* pm, float px, float py, float pz, const float* S /*cov3D*/,
                                      const float* acc, int W, int H, float tanfovx, float tanfovy, const float d[3], float* out /*[27]*/,
                                      float op)
{
    LgBackChain k;
    lg_backward_chain<AA>(vm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, op, k);
    const float fx = k.fx, fy = k.fy, vz = k.vz, gndx = k.gndx, gndy = k.gndy, dtx = k.dtx, dty = k.dty, dtz = k.dtz;
    const float* dT0 = k.dT0; const float* dT1 = k.dT1;
    // the J entries, exactly lg_ewa's expressions
    const float J00 = fx / vz, J02 = -(fx * k.e.txc) / (vz * vz);
    const float J11 = fy / vz, J12 = -(fy * k.e.tyc) / (vz * vz);
    const float p[3] = { px, py, pz };
    for (int j = 0; j < 3; j++) {
        out[3 * j + 0] = p[j] * dtx + dT0[j] * J00;
        out[3 * j + 1] = p[j] * dty + dT1[j] * J11;
        out[3 * j + 2] = p[j] * dtz + dT0[j] * J02 + dT1[j] * J12;
    }
    out[9] = dtx; out[10] = dty; out[11] = dtz;
    float hxm, hym, m_w;
    lg_hom_point(pm, px, py, pz, hxm, hym, m_w);
    float mul1 = hxm * m_w * m_w, mul2 = hym * m_w * m_w;
    const float dh[3] = { gndx * m_w, gndy * m_w, -(mul1 * gndx + mul2 * gndy) };
    for (int j = 0; j < 3; j++) {
        out[12 + 3 * j + 0] = p[j] * dh[0];
        out[12 + 3 * j + 1] = p[j] * dh[1];
        out[12 + 3 * j + 2] = p[j] * dh[2];
    }
    out[21] = dh[0]; out[22] = dh[1]; out[23] = dh[2];
    out[24] = -d[0]; out[25] = -d[1]; out[26] = -d[2];
}
LG_HD void lg_backward_camera_terms(const float* vm, const float* pm, float px, float py, float pz, const float* S /*cov3D*/,
                                    const float* acc, int W, int H, float tanfovx, float tanfovy, const float d[3], float* out /*[27]*/)
{
    lg_backward_camera_terms_t<false>(vm, pm, px, py, pz, S, acc, W, H, tanfovx, tanfovy, d, out, 0.0f);
}

// dL/dR (row-major g) -> dL/dq through lg_quat_to_rot, q = (r, x, y, z) taken as free variables.  The ONE copy: lg_backward_cov3d and
// lg_normal_row_bwd call it.
LG_HD void lg_quat_rot_bwd(const float q[4], const float g[9], float drot[4])
{
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    drot[0] = 2.0f * (-z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
    drot[1] = 2.0f * (y * g[1] + z * g[2] + y * g[3] - 2.0f * x * g[4] - r * g[5] + z * g[6] + r * g[7] - 2.0f * x * g[8]);
    drot[2] = 2.0f * (-2.0f * y * g[0] + x * g[1] + r * g[2] + x * g[3] + z * g[5] - r * g[6] + z * g[7] - 2.0f * y * g[8]);
    drot[3] = 2.0f * (-2.0f * z * g[0] - r * g[1] + x * g[2] + r * g[3] - 2.0f * z * g[4] + y * g[5] + x * g[6] + y * g[7]);
}

// dL/dSigma(packed) -> dL/dscale, dL/dquaternion.  Like the published implementation the
// scale gradient carries no scale_modifier factor.
LG_HD void lg_backward_cov3d(const float sc[3], float mod, const float q[4], const float dS[6], float dscale[3], float drot[4])
{
    float sv[3] = { mod * sc[0], mod * sc[1], mod * sc[2] };
    float Rm[9];
    lg_quat_to_rot(q, Rm);
    float L[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) L[3 * i + j] = Rm[3 * i + j] * sv[j];
    float Gs[9] = { dS[0], 0.5f * dS[1], 0.5f * dS[2], 0.5f * dS[1], dS[3], 0.5f * dS[4], 0.5f * dS[2], 0.5f * dS[4], dS[5] };
    float dLm[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++)
        dLm[3 * i + j] = 2.0f * (Gs[3 * i] * L[j] + Gs[3 * i + 1] * L[3 + j] + Gs[3 * i + 2] * L[6 + j]);
    for (int j = 0; j < 3; j++) dscale[j] = dLm[j] * Rm[j] + dLm[3 + j] * Rm[3 + j] + dLm[6 + j] * Rm[6 + j];
    float g[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) g[3 * i + j] = dLm[3 * i + j] * sv[j];
    lg_quat_rot_bwd(q, g, drot);
}

// ---------------------------------------------------------------------------------------------
// SH backward, in four steps that are written ONCE each:
//   lg_sh_dir          the offset o = mean - camera centre and the unit view direction (x, y, z) = o / |o|
//   lg_sh_dir_deriv    d rgb_c / d (x, y, z) of channel c: needs the coefficients
//   lg_sh_store_basis  dL/dsh[k][c] = basis_k(x, y, z) dRGB_c through store(k, c, value): needs no coefficient
//   lg_sh_dir_to_mean  the gradient of the direction chained through the normalisation into dmean
// (lg_sh_to_rgb, the forward, keeps its own direction and polynomial: another association, pinned against the oracle as it is.)
struct LgShDir { float ox, oy, oz, x, y, z; };
LG_HD LgShDir lg_sh_dir(float px, float py, float pz, const float* campos)
{
    LgShDir v;
    v.ox = px - campos[0]; v.oy = py - campos[1]; v.oz = pz - campos[2];
    float len = sqrtf(v.ox * v.ox + v.oy * v.oy + v.oz * v.oz);
    v.x = v.ox / len; v.y = v.oy / len; v.z = v.oz / len;
    return v;
}
LG_HD void lg_sh_dir_deriv(int deg, const float* sh, int c, float x, float y, float z, float& dRdx, float& dRdy, float& dRdz)
{
    dRdx = 0.0f; dRdy = 0.0f; dRdz = 0.0f;
    if (deg > 0) {
        dRdx = -LG_SH_C1 * sh[3 * 3 + c];
        dRdy = -LG_SH_C1 * sh[1 * 3 + c];
        dRdz = LG_SH_C1 * sh[2 * 3 + c];
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            dRdx += LG_SH_C2_0 * y * sh[4 * 3 + c] + LG_SH_C2_2 * 2.0f * -x * sh[6 * 3 + c] + LG_SH_C2_3 * z * sh[7 * 3 + c] +
                    LG_SH_C2_4 * 2.0f * x * sh[8 * 3 + c];
            dRdy += LG_SH_C2_0 * x * sh[4 * 3 + c] + LG_SH_C2_1 * z * sh[5 * 3 + c] + LG_SH_C2_2 * 2.0f * -y * sh[6 * 3 + c] +
                    LG_SH_C2_4 * 2.0f * -y * sh[8 * 3 + c];
            dRdz += LG_SH_C2_1 * y * sh[5 * 3 + c] + LG_SH_C2_2 * 2.0f * 2.0f * z * sh[6 * 3 + c] + LG_SH_C2_3 * x * sh[7 * 3 + c];
            if (deg > 2) {
                dRdx += LG_SH_C3_0 * sh[9 * 3 + c] * 3.0f * 2.0f * xy + LG_SH_C3_1 * sh[10 * 3 + c] * yz +
                        LG_SH_C3_2 * sh[11 * 3 + c] * -2.0f * xy + LG_SH_C3_3 * sh[12 * 3 + c] * -3.0f * 2.0f * xz +
                        LG_SH_C3_4 * sh[13 * 3 + c] * (-3.0f * xx + 4.0f * zz - yy) + LG_SH_C3_5 * sh[14 * 3 + c] * 2.0f * xz +
                        LG_SH_C3_6 * sh[15 * 3 + c] * 3.0f * (xx - yy);
                dRdy += LG_SH_C3_0 * sh[9 * 3 + c] * 3.0f * (xx - yy) + LG_SH_C3_1 * sh[10 * 3 + c] * xz +
                        LG_SH_C3_2 * sh[11 * 3 + c] * (-3.0f * yy + 4.0f * zz - xx) +
                        LG_SH_C3_3 * sh[12 * 3 + c] * -3.0f * 2.0f * yz + LG_SH_C3_4 * sh[13 * 3 + c] * -2.0f * xy +
                        LG_SH_C3_5 * sh[14 * 3 + c] * -2.0f * yz + LG_SH_C3_6 * sh[15 * 3 + c] * -3.0f * 2.0f * xy;
                dRdz += LG_SH_C3_1 * sh[10 * 3 + c] * xy + LG_SH_C3_2 * sh[11 * 3 + c] * 4.0f * 2.0f * yz +
                        LG_SH_C3_3 * sh[12 * 3 + c] * 3.0f * (2.0f * zz - xx - yy) +
                        LG_SH_C3_4 * sh[13 * 3 + c] * 4.0f * 2.0f * xz + LG_SH_C3_5 * sh[14 * 3 + c] * (xx - yy);
            }
        }
    }
}
template <typename StoreFn>
LG_HD void lg_sh_store_basis(int deg, int c, float x, float y, float z, float d, StoreFn store)
{
    store(0, c, LG_SH_C0 * d);
    if (deg > 0) {
        store(1, c, -LG_SH_C1 * y * d);
        store(2, c, LG_SH_C1 * z * d);
        store(3, c, -LG_SH_C1 * x * d);
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            store(4, c, LG_SH_C2_0 * xy * d);
            store(5, c, LG_SH_C2_1 * yz * d);
            store(6, c, LG_SH_C2_2 * (2.0f * zz - xx - yy) * d);
            store(7, c, LG_SH_C2_3 * xz * d);
            store(8, c, LG_SH_C2_4 * (xx - yy) * d);
            if (deg > 2) {
                store(9, c, LG_SH_C3_0 * y * (3.0f * xx - yy) * d);
                store(10, c, LG_SH_C3_1 * xy * z * d);
                store(11, c, LG_SH_C3_2 * y * (4.0f * zz - xx - yy) * d);
                store(12, c, LG_SH_C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * d);
                store(13, c, LG_SH_C3_4 * x * (4.0f * zz - xx - yy) * d);
                store(14, c, LG_SH_C3_5 * z * (xx - yy) * d);
                store(15, c, LG_SH_C3_6 * x * (xx - 3.0f * yy) * d);
            }
        }
    }
}
LG_HD void lg_sh_dir_to_mean(const LgShDir& v, float ddx, float ddy, float ddz, float dmean[3])
{
    const float ox = v.ox, oy = v.oy, oz = v.oz;
    float sum2 = ox * ox + oy * oy + oz * oz;
    float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    dmean[0] += ((sum2 - ox * ox) * ddx - oy * ox * ddy - oz * ox * ddz) * invsum32;
    dmean[1] += (-ox * oy * ddx + (sum2 - oy * oy) * ddy - oz * oy * ddz) * invsum32;
    dmean[2] += (-ox * oz * ddx - oy * oz * ddy + (sum2 - oz * oz) * ddz) * invsum32;
}

// d rgb_c / d (unit view direction), J[3 c + {0,1,2}] = {dRdx, dRdy, dRdz} of channel c: the part of the SH backward that needs the
// coefficients, and it depends on forward-time quantities only.  K1 evaluates it next to the colours (the coefficients are in registers
// there) and leaves 36 bytes per visible Gaussian; K9 then never reads the 12 M bytes of SH coefficients again (round 4: 388 MB per view at
// C3).
LG_HD void lg_sh_dir_jacobian(int deg, const float* sh, float px, float py, float pz, const float* campos, float J[9])
{
    const LgShDir v = lg_sh_dir(px, py, pz, campos);
    for (int c = 0; c < 3; c++) lg_sh_dir_deriv(deg, sh, c, v.x, v.y, v.z, J[3 * c], J[3 * c + 1], J[3 * c + 2]);
}

// SH backward with the direction Jacobian handed in (lg_sh_dir_jacobian): dL/dSH through store(k, c, value), the view-direction term into
// dmean[3].  dRGB already has clamped channels zeroed.
template <typename StoreFn>
LG_HD void lg_backward_sh_jac(int deg, const float J[9], float px, float py, float pz, const float* campos, const float dRGB[3],
                              float dmean[3], StoreFn store)
{
    const LgShDir v = lg_sh_dir(px, py, pz, campos);
    float ddx = 0.0f, ddy = 0.0f, ddz = 0.0f;
    for (int c = 0; c < 3; c++) {
        const float d = dRGB[c];
        lg_sh_store_basis(deg, c, v.x, v.y, v.z, d, store);
        ddx += J[3 * c] * d; ddy += J[3 * c + 1] * d; ddz += J[3 * c + 2] * d;
    }
    lg_sh_dir_to_mean(v, ddx, ddy, ddz, dmean);
}

// SH backward from the coefficients: the two functions above, one after the other -- bit-identical to the saved-Jacobian path by
// construction (tests/test_gpu_call_shapes.py asserts it on the device).
template <typename StoreFn>
LG_HD void lg_backward_sh(int deg, const float* sh, float px, float py, float pz, const float* campos, const float dRGB[3],
                          float dmean[3], StoreFn store)
{
    float J[9];
    lg_sh_dir_jacobian(deg, sh, px, py, pz, campos, J);
    lg_backward_sh_jac(deg, J, px, py, pz, campos, dRGB, dmean, store);
}
// The same values from the same four steps in ONE pass over the channels, for a store that is not a register array (lg_vq_color_bwd.h's
// LDS tile: EXPERIMENTS 14).
template <typename StoreFn>
LG_HD void lg_backward_sh_one_pass(int deg, const float* sh, float px, float py, float pz, const float* campos, const float dRGB[3],
                                   float dmean[3], StoreFn store)
{
    const LgShDir v = lg_sh_dir(px, py, pz, campos);
    float ddx = 0.0f, ddy = 0.0f, ddz = 0.0f;
    for (int c = 0; c < 3; c++) {
        const float d = dRGB[c];
        float dRdx, dRdy, dRdz;
        lg_sh_dir_deriv(deg, sh, c, v.x, v.y, v.z, dRdx, dRdy, dRdz);
        lg_sh_store_basis(deg, c, v.x, v.y, v.z, d, store);
        ddx += dRdx * d; ddy += dRdy * d; ddz += dRdz * d;
    }
    lg_sh_dir_to_mean(v, ddx, ddy, ddz, dmean);
}

// ---------------------------------------------------------------------------------------------
// Densification (lg_densify.h): the two formulas that make a split child from its parent's RAW rows, as
// densify_and_split writes them (scene/gaussian_model.py:678-687, build_rotation utils/general_utils.py:84-107).
//   s = exp(raw scaling)      the caller evaluates it (expf in the kernels, as K1 under LG_FLAG_RAW_PARAMS)
//   xyz_child     = R(q / |q|) (noise * s) + xyz        noise: one unit-normal row per child; q in (r, x, y, z) order
//   scaling_child = log(s / 1.6f)                       1.6f = float(0.8 * 2)
// The norm is summed left to right and q divided by it (build_rotation's own statements); every product and sum below is
// rounded on its own (no contraction).
#define LG_DENSIFY_SHRINK 1.6f
LG_HD void lg_densify_child_xyz(const float q_raw[4], const float s[3], const float noise[3], const float xyz[3], float out[3])
{
    const float n = sqrtf(q_raw[0] * q_raw[0] + q_raw[1] * q_raw[1] + q_raw[2] * q_raw[2] + q_raw[3] * q_raw[3]);
    const float q[4] = { q_raw[0] / n, q_raw[1] / n, q_raw[2] / n, q_raw[3] / n };
    const float v0 = noise[0] * s[0], v1 = noise[1] * s[1], v2 = noise[2] * s[2];
    float R[9];
    lg_quat_to_rot(q, R);
    out[0] = ((R[0] * v0 + R[1] * v1) + R[2] * v2) + xyz[0];
    out[1] = ((R[3] * v0 + R[4] * v1) + R[5] * v2) + xyz[1];
    out[2] = ((R[6] * v0 + R[7] * v1) + R[8] * v2) + xyz[2];
}
LG_HD float lg_densify_child_scaling(float s) { return logf(s / LG_DENSIFY_SHRINK); }

// ---------------------------------------------------------------------------------------------
// 3D smoothing filter (lg_filter3d.h; Mip-Splatting's 3D filter): what ONE camera says about one Gaussian mean.
//   x, y, z = view-space coordinates: three explicit fmaf each, in K1's term order (x, then y, then z of the mean, the translation
//             innermost): fmaf(vm[8 + c], pz, fmaf(vm[4 + c], py, fmaf(vm[c], px, vm[12 + c])))
//   u = fmaf(x / z, fx, 0.5f W)    v = fmaf(y / z, fy, 0.5f H)       fx = W / (2 tanfovx), fy = H / (2 tanfovy)
//   seen = z > 0.2f && -0.15f W <= u <= 1.15f W && -0.15f H <= v <= 1.15f H          (a NaN compares false: unseen)
//   t    = z / fx                                                                      world units per pixel at the mean
// Every division is the correctly rounded one; nothing besides the written fmaf is contracted.
// LgFilterCam: the per-camera constants, evaluated once per camera (lg_filter3d_camera) and then read by every Gaussian.
#define LG_FILTER3D_NEAR 0.2f
#define LG_FILTER3D_VARIANCE 0.2f       // filter_3D = sqrtf(0.2f) t
struct LgFilterCam {
    float m[12];                        // view matrix columns 0..2, row-vector layout: m[4 c + k] = vm[4 k + c] (k = 3: translation)
    float fx, fy, cx, cy;               // focal lengths in pixels, 0.5f W, 0.5f H
    float ulo, uhi, vlo, vhi;           // -0.15f W, 1.15f W, -0.15f H, 1.15f H
};
LG_HD void lg_filter3d_camera(const float* vm, float tanfovx, float tanfovy, int W, int H, LgFilterCam& c)
{
    for (int col = 0; col < 3; col++)
        for (int k = 0; k < 4; k++) c.m[4 * col + k] = vm[4 * k + col];
    const float w = (float)W, h = (float)H;
    c.fx = w / (2.0f * tanfovx); c.fy = h / (2.0f * tanfovy);
    c.cx = 0.5f * w; c.cy = 0.5f * h;
    c.ulo = -0.15f * w; c.uhi = 1.15f * w;
    c.vlo = -0.15f * h; c.vhi = 1.15f * h;
}
LG_HD float lg_filter3d_value(float t) { return sqrtf(LG_FILTER3D_VARIANCE) * t; }
// true when the camera sees the mean; t is written either way (the caller takes the minimum over the cameras that see it)
LG_HD bool lg_filter3d_term(const LgFilterCam& c, float px, float py, float pz, float& t)
{
    const float x = fmaf(c.m[2], pz, fmaf(c.m[1], py, fmaf(c.m[0], px, c.m[3])));
    const float y = fmaf(c.m[6], pz, fmaf(c.m[5], py, fmaf(c.m[4], px, c.m[7])));
    const float z = fmaf(c.m[10], pz, fmaf(c.m[9], py, fmaf(c.m[8], px, c.m[11])));
    const float u = fmaf(x / z, c.fx, c.cx);
    const float v = fmaf(y / z, c.fy, c.cy);
    t = z / c.fx;
    return z > LG_FILTER3D_NEAR && u >= c.ulo && u <= c.uhi && v >= c.vlo && v <= c.vhi;
}

// ---------------------------------------------------------------------------------------------
// 3DGS-MCMC (lg_mcmc.h; Kheradmand et al. 2024): the per-row formulas of the position noise and of relocation.
// Noise, float32, every product and sum rounded on its own:
//   sigma = 1 / (1 + expf(-opacity_raw))     g = 1 / (1 + expf(-k ((1 - sigma) - x0)))     gate = g c
//   (expf overflowing to +inf gives g = 1 / inf = 0, never NaN)
//   v = noise * gate      xyz += R (s^2 o (R^T v))      R = R(q / |q|) as lg_densify_child_xyz builds it, s = exp(raw scaling)
// which is Sigma v for Sigma = L L^T, L = R diag(s), without the 3x3 matrix.
LG_HD float lg_mcmc_gate(float opacity_raw, float c, float k, float x0)
{
    const float sigma = 1.0f / (1.0f + expf(-opacity_raw));
    const float g = 1.0f / (1.0f + expf(-k * ((1.0f - sigma) - x0)));
    return g * c;
}
LG_HD void lg_mcmc_noise_xyz(const float q_raw[4], const float s[3], const float noise[3], float gate, const float xyz[3], float out[3])
{
    const float n = sqrtf(q_raw[0] * q_raw[0] + q_raw[1] * q_raw[1] + q_raw[2] * q_raw[2] + q_raw[3] * q_raw[3]);
    const float q[4] = { q_raw[0] / n, q_raw[1] / n, q_raw[2] / n, q_raw[3] / n };
    const float v0 = noise[0] * gate, v1 = noise[1] * gate, v2 = noise[2] * gate;
    float R[9];
    lg_quat_to_rot(q, R);
    const float t0 = (s[0] * s[0]) * ((R[0] * v0 + R[3] * v1) + R[6] * v2);       // s^2 o (R^T v)
    const float t1 = (s[1] * s[1]) * ((R[1] * v0 + R[4] * v1) + R[7] * v2);
    const float t2 = (s[2] * s[2]) * ((R[2] * v0 + R[5] * v1) + R[8] * v2);
    out[0] = xyz[0] + ((R[0] * t0 + R[1] * t1) + R[2] * t2);
    out[1] = xyz[1] + ((R[3] * t0 + R[4] * t1) + R[5] * t2);
    out[2] = xyz[2] + ((R[6] * t0 + R[7] * t1) + R[8] * t2);
}

// Relocation of a row drawn cnt >= 1 times: in DOUBLE from the float32 raw inputs, each output rounded once.
//   M = min(cnt + 1, 51)     o = sigmoid(opacity_raw)     x = 1 - (1 - o)^(1/M)
//   D = sum_{k=0..M-1} C(M, k+1) (-1)^k x^(k+1) / sqrt(k+1)
//       (the published double sum over i = 1..M and k = 0..i-1 of C(i-1, k) ..., collapsed by sum_i C(i-1, k) = C(M, k+1))
//   opacity_raw' = logit(clamp(x, min_opacity, 1 - 2^-23))          scaling_raw' = scaling_raw + log(o / D), o / D from the unclamped x
// 1 - o = 1 / (1 + exp(raw)) is formed directly and x = -expm1(-log1p(exp(raw)) / M): no cancellation at o -> 1.  The binomials are
// integers (C(51, .) < 2^48: each product c (M - k) < 2^54 fits 64 bits and the division is exact); x^(k+1) is a running product.
#define LG_MCMC_BINOM_MAX 51
LG_HD double lg_mcmc_binomial_sum(double x, int M)                 // D; 1 <= M <= LG_MCMC_BINOM_MAX
{
    double D = 0.0, xp = x;
    uint64_t c = (uint64_t)M;                                       // C(M, 1)
    for (int k = 0; k < M; k++) {
        const double term = (double)c * xp / sqrt((double)(k + 1));
        D += (k & 1) ? -term : term;
        xp *= x;
        c = c * (uint64_t)(M - k - 1) / (uint64_t)(k + 2);          // C(M, k+2)
    }
    return D;
}
LG_HD void lg_mcmc_relocate(float opacity_raw, const float scaling_raw[3], int cnt, float min_opacity, float& new_opacity, float new_scaling[3])
{
    const int M = cnt + 1 < LG_MCMC_BINOM_MAX ? cnt + 1 : LG_MCMC_BINOM_MAX;
    const double o = 1.0 / (1.0 + exp(-(double)opacity_raw));
    const double x = -expm1(-log1p(exp((double)opacity_raw)) / (double)M);
    const double D = lg_mcmc_binomial_sum(x, M);
    const double hi = 1.0 - 0x1p-23;
    const double xc = x < (double)min_opacity ? (double)min_opacity : (x > hi ? hi : x);
    new_opacity = (float)log(xc / (1.0 - xc));
    const double shift = log(o / D);
    for (int a = 0; a < 3; a++) new_scaling[a] = (float)((double)scaling_raw[a] + shift);
}

// ---------------------------------------------------------------------------------------------
// Normals (lg_normals.h).  Per Gaussian and view, float32, every product and sum rounded on its own, sums left
// to right unless bracketed:
//   q^ = q / max(|q|, 1e-12), |q| = sqrtf((q0^2 + q1^2) + (q2^2 + q3^2))       K1's F.normalize (lg_preprocess.h), now lg_quat_normalize
//   R = lg_quat_to_rot(q^)     k = the first index of the smallest scaling     n_w = column k of R
//   n_v[c] = (n_w[0] vm[c] + n_w[1] vm[4 + c]) + n_w[2] vm[8 + c]              p_v = lg_view_point(vm, xyz)
//   s = -1 when (n_v[0] p_v[0] + n_v[1] p_v[1]) + n_v[2] p_v[2] > 0, else +1   (a NaN compares false: +1)
//   row = (s n_v, p_v.z)
// Backward, k and s constants:  d xyz[a] = g[3] vm[4 a + 2];  dL/dn_w[a] = s ((vm[4 a] g[0] + vm[4 a + 1] g[1]) + vm[4 a + 2] g[2]) sits in
// column k of dL/dR, lg_quat_rot_bwd takes it to q^, and K9's statement of the normalisation, (d - q^ (q^ . d)) / |q|, to q.
LG_HD float lg_quat_normalize(const float q_raw[4], float q[4])
{
    const float qn = fmaxf(sqrtf((q_raw[0] * q_raw[0] + q_raw[1] * q_raw[1]) + (q_raw[2] * q_raw[2] + q_raw[3] * q_raw[3])), 1e-12f);
    q[0] = q_raw[0] / qn; q[1] = q_raw[1] / qn; q[2] = q_raw[2] / qn; q[3] = q_raw[3] / qn;
    return qn;
}
LG_HD int lg_normal_axis(const float sc[3])
{
    int k = 0;
    float m = sc[0];
    if (sc[1] < m) { k = 1; m = sc[1]; }
    if (sc[2] < m) k = 2;
    return k;
}
struct LgNormalRow { float q[4], qn, nv[3], pv[3], s; int k; };
LG_HD void lg_normal_view(const float* vm, const float xyz[3], const float sc[3], const float q_raw[4], LgNormalRow& o)
{
    o.qn = lg_quat_normalize(q_raw, o.q);
    float R[9];
    lg_quat_to_rot(o.q, R);
    const int k = o.k = lg_normal_axis(sc);
    const float n0 = k == 0 ? R[0] : (k == 1 ? R[1] : R[2]);
    const float n1 = k == 0 ? R[3] : (k == 1 ? R[4] : R[5]);
    const float n2 = k == 0 ? R[6] : (k == 1 ? R[7] : R[8]);
    for (int c = 0; c < 3; c++) o.nv[c] = (n0 * vm[c] + n1 * vm[4 + c]) + n2 * vm[8 + c];
    lg_view_point(vm, xyz[0], xyz[1], xyz[2], o.pv[0], o.pv[1], o.pv[2]);
    o.s = ((o.nv[0] * o.pv[0] + o.nv[1] * o.pv[1]) + o.nv[2] * o.pv[2]) > 0.0f ? -1.0f : 1.0f;
}
LG_HD void lg_normal_row(const float* vm, const float xyz[3], const float sc[3], const float q_raw[4], float row[4])
{
    LgNormalRow o;
    lg_normal_view(vm, xyz, sc, q_raw, o);
    row[0] = o.s * o.nv[0]; row[1] = o.s * o.nv[1]; row[2] = o.s * o.nv[2]; row[3] = o.pv[2];
}
LG_HD void lg_normal_row_bwd(const float* vm, const float xyz[3], const float sc[3], const float q_raw[4], const float g[4], float dxyz[3], float drot[4])
{
    LgNormalRow o;
    lg_normal_view(vm, xyz, sc, q_raw, o);
    float G[9], d[4];
    for (int a = 0; a < 3; a++) {
        dxyz[a] = g[3] * vm[4 * a + 2];
        const float dn = o.s * ((vm[4 * a] * g[0] + vm[4 * a + 1] * g[1]) + vm[4 * a + 2] * g[2]);
        for (int j = 0; j < 3; j++) G[3 * a + j] = j == o.k ? dn : 0.0f;
    }
    lg_quat_rot_bwd(o.q, G, d);
    const float qg = o.q[0] * d[0] + o.q[1] * d[1] + o.q[2] * d[2] + o.q[3] * d[3];
    const float inv = 1.0f / o.qn;
    for (int j = 0; j < 4; j++) drot[j] = (d[j] - o.q[j] * qg) * inv;
}

// Per pixel: the normal of the depth surface (2DGS's depth_to_normal).  The un-projected point of pixel (x, y) is depth (rx, ry, 1) with
//   rx = ((2 x + 1) / W - 1) tanfovx     ry = ((2 y + 1) / H - 1) tanfovy             (lg_pixel_ray: the pixel centre of ndc2Pix)
// and, with dc the depth of the pixel, du, dd, dl, dr the depths above (y - 1), below, left and right of the pixel and rxm / rxp, rym / ryp the rays of those columns / rows,
//   a = P(x, y + 1) - P(x, y - 1) = (dd rx - du rx, dd ryp - du rym, dd - du)     b = P(x + 1, y) - P(x - 1, y) = (dr rxp - dl rxm, dr ry - dl ry, dr - dl)
//   c = a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)     |c| = sqrtf((c0^2 + c1^2) + c2^2)     N_d = c / max(|c|, 1e-12)
// A pixel whose c has a non-finite component, or whose own depth dc is not finite (c does not read it), is zero and passes no gradient
// (ok = false); the caller zeroes the image border.
#define LG_NORMAL_EPS 1e-12f
LG_HD float lg_pixel_ray(int x, int W, float tanfov) { return ((float)(2 * x + 1) / (float)W - 1.0f) * tanfov; }
struct LgDepthNormal { float a[3], b[3], n[3], len; bool ok; };
LG_HD void lg_depth_normal(float dc, float du, float dd, float dl, float dr, float rx, float rxm, float rxp, float ry, float rym, float ryp, LgDepthNormal& o)
{
    o.a[0] = dd * rx - du * rx; o.a[1] = dd * ryp - du * rym; o.a[2] = dd - du;
    o.b[0] = dr * rxp - dl * rxm; o.b[1] = dr * ry - dl * ry; o.b[2] = dr - dl;
    const float c0 = o.a[1] * o.b[2] - o.a[2] * o.b[1], c1 = o.a[2] * o.b[0] - o.a[0] * o.b[2], c2 = o.a[0] * o.b[1] - o.a[1] * o.b[0];
    o.ok = fabsf(dc) < INFINITY && fabsf(c0) < INFINITY && fabsf(c1) < INFINITY && fabsf(c2) < INFINITY;
    o.len = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    const float m = fmaxf(o.len, LG_NORMAL_EPS);
    o.n[0] = o.ok ? c0 / m : 0.0f; o.n[1] = o.ok ? c1 / m : 0.0f; o.n[2] = o.ok ? c2 / m : 0.0f;
}
// Backward of one pixel q: G = dL/dN_d(q) -> what q adds to dL/ddepth of its four neighbours.  dL/dc = (G - n (n . G)) / |c| (G / 1e-12 under
// the clamp), dL/da = b x dL/dc, dL/db = dL/dc x a, and the neighbour's depth multiplies its own ray:
//   up = -(ray(x, y - 1) . dL/da)   down = ray(x, y + 1) . dL/da   left = -(ray(x - 1, y) . dL/db)   right = ray(x + 1, y) . dL/db
// lg_depth_grad is the GATHER of pixel p: the down tap of the pixel above it, the up tap of the one below, the right tap of its left
// neighbour and the left tap of its right one, summed in that order.
struct LgNormalTaps { float up, down, left, right; };
LG_HD void lg_depth_normal_bwd(const LgDepthNormal& o, const float G[3], float rx, float rxm, float rxp, float ry, float rym, float ryp, LgNormalTaps& t)
{
    if (!o.ok) { t.up = t.down = t.left = t.right = 0.0f; return; }
    const float m = fmaxf(o.len, LG_NORMAL_EPS);
    float dc[3];
    if (o.len > LG_NORMAL_EPS) {
        const float ng = (o.n[0] * G[0] + o.n[1] * G[1]) + o.n[2] * G[2];
        for (int k = 0; k < 3; k++) dc[k] = (G[k] - o.n[k] * ng) / m;
    } else {
        for (int k = 0; k < 3; k++) dc[k] = G[k] / m;
    }
    const float da0 = o.b[1] * dc[2] - o.b[2] * dc[1], da1 = o.b[2] * dc[0] - o.b[0] * dc[2], da2 = o.b[0] * dc[1] - o.b[1] * dc[0];
    const float db0 = dc[1] * o.a[2] - dc[2] * o.a[1], db1 = dc[2] * o.a[0] - dc[0] * o.a[2], db2 = dc[0] * o.a[1] - dc[1] * o.a[0];
    t.up = -((rx * da0 + rym * da1) + da2);
    t.down = (rx * da0 + ryp * da1) + da2;
    t.left = -((rxm * db0 + ry * db1) + db2);
    t.right = (rxp * db0 + ry * db1) + db2;
}
LG_HD float lg_depth_grad(float down_of_above, float up_of_below, float right_of_left, float left_of_right)
{
    return ((down_of_above + up_of_below) + right_of_left) + left_of_right;
}
// The consistency loss at one pixel: term = 1 - w (N_r . N_d); with coef = -(scale w), scale = dL/dL / (H W): dL/dN_r = coef N_d and G = coef N_r.
LG_HD float lg_normal_term(float w, const float nr[3], const float nd[3]) { return 1.0f - w * ((nr[0] * nd[0] + nr[1] * nd[1]) + nr[2] * nd[2]); }

// ---------------------------------------------------------------------------------------------
// Depth distortion and median depth over a pixel's contributors (lg_distortion.h).  With the blending weights
// w_i = alpha_i T_i (lg_feature_step) and a per-Gaussian scalar m_i,
//   D = sum_{i<j} w_i w_j (m_i - m_j)^2,      median = the m of the entry that carries T across one half (2DGS).
// D is invariant under a shift of m, and A M2 - M1^2 on the raw m cancels catastrophically for a thin surface far from the camera, so the
// sums run about the pixel's FIRST contributor: c = its m, u = m - c.  State per pixel, all zero at the start.
struct LgDistortion { float A, P1, P2, D, c, med; uint32_t med_pos; };
// One contributing (pixel, entry) pair in list order: w the weight lg_feature_step returned, Tin the T before that step, pos the entry's
// 1-based position in the tile's list.  The first contributor is the one that finds med_pos == 0 (its Tin is 1 > 0.5, so it sets
// med_pos).  Order of the float operations, one rounding each (no contraction):
//   u = m - c;   uu = u u;   t = (uu A + P2) - (2 u) P1;   D = D + w t;   A = A + w;   P1 = P1 + w u;   P2 = P2 + w uu
// The median rule: the last entry whose incoming T is above 0.5 -- the entry that takes T to 0.5 or below, or the last contributor
// when T never gets there.  A pixel without contributors keeps D = 0, med = 0, med_pos = 0.
LG_HD void lg_distortion_step(float w, float Tin, float m, uint32_t pos, LgDistortion& s)
{
    if (s.med_pos == 0u) s.c = m;
    const float u = m - s.c;
    const float uu = u * u;
    const float two_u = 2.0f * u;
    const float t = (uu * s.A + s.P2) - two_u * s.P1;
    s.D = s.D + w * t;
    s.A = s.A + w;
    s.P1 = s.P1 + w * u;
    s.P2 = s.P2 + w * uu;
    if (Tin > 0.5f) { s.med = m; s.med_pos = pos; }
}
// One contributing pair of the BACK-TO-FRONT replay (lg_distortion_bwd): s holds the pixel's FINAL A, P1, P2, c and med_pos, gD = dL/dD
// and gM = dL/dmedian of the pixel.  dD/dw_k = u_k^2 A - 2 u_k P1 + P2 is the entry's "feature" q, chained through alpha and T by
// lg_feature_bwd_step unchanged (no background term); dD/dm_k = 2 w_k (u_k A - P1); the median passes its gradient to the m of the
// selected entry only (the selection is piecewise constant).  Order:
//   u = m - c;   q = gD (((u u) A - (2 u) P1) + P2);   [lg_feature_bwd_step -> mom[0..5], w]
//   dm = ((2 gD) w) (u A - P1) + (pos == med_pos ? gM : 0)
// Returns false (mom, dm, T, S untouched) when the entry does not contribute.
template <bool EXACT>
LG_HD bool lg_distortion_bwd_step(bool live, float power, float G, float alpha, float dx, float dy, float m, uint32_t pos, const LgDistortion& s,
                                  float gD, float gM, float& T, float& S, float* mom, float& dm)
{
    const float u = m - s.c;
    const float uu = u * u;
    const float two_u = 2.0f * u;
    const float q = gD * ((uu * s.A - two_u * s.P1) + s.P2);
    float w = 0.0f;
    if (!lg_feature_bwd_step<EXACT>(live, power, G, alpha, dx, dy, q, 0.0f, T, S, mom, w)) return false;
    const float gw = (2.0f * gD) * w;
    dm = gw * (u * s.A - s.P1) + (pos == s.med_pos ? gM : 0.0f);
    return true;
}

// ---------------------------------------------------------------------------------------------
// TSDF fusion of depth maps and marching tetrahedra (include/lightgaussian_mesh.h; lg_tsdf.h's kernels and
// tests/cpu_harness/lg_tsdf_harness.cpp call the same functions).
//
// The volume: nx x ny x nz points, x fastest; point (x, y, z) lies at origin + voxel (x, y, z): one product, one sum per axis.
// One point under one view, in this order (a step that fails leaves the point's values as they are):
//   p_v = p vm (lg_view_point)                                  z = p_v.z > z_min
//   fx = (p_v.x / (z tanfovx) + 1) (0.5 W)   px = floor(fx)     fy, py likewise     0 <= px < W, 0 <= py < H   (a NaN fails)
//   d = depth[py, px]       d > 0, finite, d <= depth_max where depth_max > 0;  alpha[py, px] >= alpha_min where an alpha map is given
//   sdf = d - z >= -trunc   t = min(1, sdf / trunc)
//   w' = w + 1   tsdf = (tsdf w + t) / w'   colour_c = (colour_c w + image_c[py, px]) / w'   weight = w'
struct LgTsdfCam { int W, H; float tanfovx, tanfovy, depth_max, z_min, alpha_min; };
LG_HD float lg_tsdf_coord(float origin, float voxel, int i) { return origin + voxel * (float)i; }
// the pixel that contains the projection of the world point p, and its view-space z
LG_HD bool lg_tsdf_project(const float* vm, const LgTsdfCam& c, float px, float py, float pz, int& ix, int& iy, float& z)
{
    float vx, vy, vz;
    lg_view_point(vm, px, py, pz, vx, vy, vz);
    if (!(vz > c.z_min)) return false;
    const float fx = (vx / (vz * c.tanfovx) + 1.0f) * (0.5f * (float)c.W);
    const float fy = (vy / (vz * c.tanfovy) + 1.0f) * (0.5f * (float)c.H);
    const float flx = floorf(fx), fly = floorf(fy);
    if (!(flx >= 0.0f && flx < (float)c.W && fly >= 0.0f && fly < (float)c.H)) return false;
    ix = (int)flx; iy = (int)fly; z = vz;
    return true;
}
// the truncated signed distance t of a point at depth z under a pixel of depth d
LG_HD bool lg_tsdf_sample(const LgTsdfCam& c, float trunc, float d, float z, float& t)
{
    if (!(d > 0.0f) || !(d <= 3.402823466e+38f)) return false;
    if (c.depth_max > 0.0f && d > c.depth_max) return false;
    const float sdf = d - z;
    if (sdf < -trunc) return false;
    t = fminf(1.0f, sdf / trunc);
    return true;
}
LG_HD float lg_tsdf_mean(float v, float w, float x, float w1) { return (v * w + x) / w1; }
// What the pixel under a point holds: its depth, its alpha (read only with has_alpha) and its colour (read only where the point has one).
struct LgTsdfPixel { float d, alpha, rgb[3]; };
// One point at view-space depth z under its pixel: rgb = the point's colour or NULL.  Returns whether the point was updated.
LG_HD bool lg_tsdf_apply(const LgTsdfCam& c, float trunc, const LgTsdfPixel& p, bool has_alpha, float z, float& tsdf, float& weight, float* rgb)
{
    float t;
    if (!lg_tsdf_sample(c, trunc, p.d, z, t)) return false;
    if (has_alpha && p.alpha < c.alpha_min) return false;
    const float w = weight, w1 = w + 1.0f;
    tsdf = lg_tsdf_mean(tsdf, w, t, w1);
    if (rgb) {
        rgb[0] = lg_tsdf_mean(rgb[0], w, p.rgb[0], w1);
        rgb[1] = lg_tsdf_mean(rgb[1], w, p.rgb[1], w1);
        rgb[2] = lg_tsdf_mean(rgb[2], w, p.rgb[2], w1);
    }
    weight = w1;
    return true;
}
// One point under one view, the gathers included: depth [H,W], color [3,H,W] or NULL, alpha [H,W] or NULL; rgb = the point's colour or NULL.
LG_HD bool lg_tsdf_update(const float* vm, const LgTsdfCam& c, const float* depth, const float* color, const float* alpha, float trunc,
                          float px, float py, float pz, float& tsdf, float& weight, float* rgb)
{
    int ix, iy;
    float z;
    if (!lg_tsdf_project(vm, c, px, py, pz, ix, iy, z)) return false;
    const size_t pix = (size_t)iy * (size_t)c.W + (size_t)ix, plane = (size_t)c.H * (size_t)c.W;
    LgTsdfPixel p = { depth[pix], alpha ? alpha[pix] : 0.0f, { 0.0f, 0.0f, 0.0f } };
    const bool colour = rgb && color;
    if (colour) { p.rgb[0] = color[pix]; p.rgb[1] = color[plane + pix]; p.rgb[2] = color[2 * plane + pix]; }
    return lg_tsdf_apply(c, trunc, p, alpha != nullptr, z, tsdf, weight, colour ? rgb : nullptr);
}

// Marching tetrahedra over the volume.  Axis bits x = 1, y = 2, z = 4; a corner or edge mask m stands for the offset (m & 1, m >> 1 & 1,
// m >> 2 & 1).  A point is observed when weight >= min_weight and inside when tsdf < iso (a NaN is neither).
//   edge slots      point p owns the edges to p + offset(m) for m = 1, 2, 4, 3, 5, 6, 7 (slot k = 0 .. 6) that stay inside the grid
//   vertex rule     an edge carries a vertex iff both ends are observed and exactly one is inside; f = tsdf - iso, t = f0 / (f0 - f1)
//                   (f0 and f1 differ in sign or one is zero and the other negative: f0 - f1 is not zero), grid position p0 + t offset,
//                   world position origin + voxel * that; colour c0 + t (c1 - c0).  Vertex ids count the carrying edges by (point, slot).
//   cells           the cube at p < (nx - 1, ny - 1, nz - 1), valid when its eight corners are observed
//   tetrahedra      six per cell, one per permutation (a, b, c) of the axes in lexicographic order, local corners 0, 1<<a, 1<<a | 1<<b, 7;
//                   the edge between local corners i < j is the slot of mask_j ^ mask_i at the point of corner i
//   triangles       by the 4-bit inside mask of the local corners: none for 0 and 15; one corner apart from the other three: the three
//                   edges from it in ascending order of the other end; two and two (a < b inside, c < d outside): the quad (a,c), (a,d),
//                   (b,d), (b,c) as (q0, q1, q2), (q0, q2, q3).  LG_MESH_FLIP_* bit `mask`: the triangle as listed has its normal (unit
//                   cube, edge midpoints) pointing from the outside corners to the inside ones, so its 2nd and 3rd index are swapped: the
//                   normals of the result point toward larger tsdf.  The bits were derived from that rule (the even permutations share
//                   one word, the odd ones its complement); the closed-surface tests of tests/test_mesh_host.py hold them.
#define LG_MESH_SLOTS 7
#define LG_MESH_SLOT_MASKS 0x7653421u       // nibble k: the offset mask of slot k
#define LG_MESH_MASK_SLOTS 0x65423100u      // nibble m: the slot of offset mask m (m = 1 .. 7)
#define LG_MESH_PERM_A 0xA50u               // two bits per tetrahedron: the axis a, and b
#define LG_MESH_PERM_B 0x489u
#define LG_MESH_FLIP_EVEN 0x4D24u           // tetrahedra 0, 3, 4
#define LG_MESH_FLIP_ODD 0x32DAu            // tetrahedra 1, 2, 5
LG_HD uint32_t lg_mesh_slot_mask(uint32_t k) { return (LG_MESH_SLOT_MASKS >> (4u * k)) & 7u; }
LG_HD uint32_t lg_mesh_mask_slot(uint32_t m) { return (LG_MESH_MASK_SLOTS >> (4u * m)) & 7u; }
LG_HD uint32_t lg_mesh_popc8(uint32_t m) { m = (m & 0x55u) + ((m >> 1) & 0x55u); m = (m & 0x33u) + ((m >> 2) & 0x33u); return (m + (m >> 4)) & 0xFu; }
LG_HD bool lg_mesh_observed(float w, float min_weight) { return w >= min_weight; }
LG_HD bool lg_mesh_inside(float f, float iso) { return f < iso; }
LG_HD size_t lg_mesh_index(int nx, int ny, int x, int y, int z) { return ((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x; }

// bit k: slot k of the point (x, y, z) carries a vertex
LG_HD uint32_t lg_mesh_edge_mask(const float* tsdf, const float* weight, int nx, int ny, int nz, int x, int y, int z, float iso, float min_weight)
{
    const size_t p = lg_mesh_index(nx, ny, x, y, z);
    if (!lg_mesh_observed(weight[p], min_weight)) return 0u;
    const bool in0 = lg_mesh_inside(tsdf[p], iso);
    uint32_t mask = 0u;
    for (uint32_t k = 0; k < LG_MESH_SLOTS; k++) {
        const uint32_t m = lg_mesh_slot_mask(k);
        const int x1 = x + (int)(m & 1u), y1 = y + (int)((m >> 1) & 1u), z1 = z + (int)((m >> 2) & 1u);
        if (x1 < nx && y1 < ny && z1 < nz) {
            const size_t q = lg_mesh_index(nx, ny, x1, y1, z1);
            if (lg_mesh_observed(weight[q], min_weight) && lg_mesh_inside(tsdf[q], iso) != in0) mask |= 1u << k;
        }
    }
    return mask;
}
// The vertex on slot k of the lattice point (x, y, z) from the values of the edge's two ends: f0v, c0 at the point, f1v, c1 at the point +
// offset(slot k); c0 = NULL: no colour.  World position, and colour.  (x, y, z) counts from the point `origin` lies at: the grid index of
// a dense volume, the GLOBAL index of a block volume.
LG_HD void lg_mesh_edge_vertex(float f0v, float f1v, const float* c0, const float* c1, int x, int y, int z, uint32_t k, float iso, const float* origin,
                               float voxel, float* pos, float* rgb)
{
    const uint32_t m = lg_mesh_slot_mask(k);
    const int ox = (int)(m & 1u), oy = (int)((m >> 1) & 1u), oz = (int)((m >> 2) & 1u);
    const float f0 = f0v - iso, f1 = f1v - iso;
    const float t = f0 / (f0 - f1);
    pos[0] = origin[0] + voxel * ((float)x + t * (float)ox);
    pos[1] = origin[1] + voxel * ((float)y + t * (float)oy);
    pos[2] = origin[2] + voxel * ((float)z + t * (float)oz);
    if (rgb && c0) {
        rgb[0] = c0[0] + t * (c1[0] - c0[0]);
        rgb[1] = c0[1] + t * (c1[1] - c0[1]);
        rgb[2] = c0[2] + t * (c1[2] - c0[2]);
    }
}
// the vertex on slot k of the point (x, y, z) of a dense grid: world position, and colour where the volume keeps one
LG_HD void lg_mesh_vertex(const float* tsdf, const float* color, int nx, int ny, int x, int y, int z, uint32_t k, float iso, const float* origin,
                          float voxel, float* pos, float* rgb)
{
    const uint32_t m = lg_mesh_slot_mask(k);
    const size_t p = lg_mesh_index(nx, ny, x, y, z), q = lg_mesh_index(nx, ny, x + (int)(m & 1u), y + (int)((m >> 1) & 1u), z + (int)((m >> 2) & 1u));
    lg_mesh_edge_vertex(tsdf[p], tsdf[q], color ? color + 3 * p : nullptr, color ? color + 3 * q : nullptr, x, y, z, k, iso, origin, voxel, pos, rgb);
}
// bit m (0 .. 7): corner offset(m) of the cell at (x, y, z) is inside; false when a corner is unobserved.  x < nx - 1, y < ny - 1, z < nz - 1.
LG_HD bool lg_mesh_cell_corners(const float* tsdf, const float* weight, int nx, int ny, int x, int y, int z, float iso, float min_weight, uint32_t& inside8)
{
    inside8 = 0u;
    bool valid = true;
    for (uint32_t m = 0; m < 8u; m++) {
        const size_t q = lg_mesh_index(nx, ny, x + (int)(m & 1u), y + (int)((m >> 1) & 1u), z + (int)((m >> 2) & 1u));
        valid = valid && lg_mesh_observed(weight[q], min_weight);
        inside8 |= (lg_mesh_inside(tsdf[q], iso) ? 1u : 0u) << m;
    }
    return valid;
}
LG_HD uint32_t lg_mesh_tet_corner(uint32_t t, uint32_t i)        // the cell corner (offset mask) of local corner i of tetrahedron t
{
    const uint32_t a = 1u << ((LG_MESH_PERM_A >> (2u * t)) & 3u), b = 1u << ((LG_MESH_PERM_B >> (2u * t)) & 3u);
    return i == 0u ? 0u : (i == 1u ? a : (i == 2u ? (a | b) : 7u));
}
LG_HD uint32_t lg_mesh_tet_inside(uint32_t t, uint32_t inside8)   // bit i: local corner i is inside
{
    uint32_t m4 = 0u;
    for (uint32_t i = 0; i < 4u; i++) m4 |= ((inside8 >> lg_mesh_tet_corner(t, i)) & 1u) << i;
    return m4;
}
LG_HD uint32_t lg_mesh_tet_count(uint32_t m4)
{
    const uint32_t n = lg_mesh_popc8(m4);
    return n == 2u ? 2u : ((n == 1u || n == 3u) ? 1u : 0u);
}
LG_HD uint32_t lg_mesh_cell_count(uint32_t inside8)
{
    uint32_t n = 0u;
    for (uint32_t t = 0; t < 6u; t++) n += lg_mesh_tet_count(lg_mesh_tet_inside(t, inside8));
    return n;
}
// the triangles of tetrahedron t under the inside mask m4, winding applied: tri[j][v] = lo | hi << 2, the edge between the local corners
// lo < hi.  Returns their number.
LG_HD uint32_t lg_mesh_tet_triangles(uint32_t t, uint32_t m4, uint32_t tri[2][3])
{
    const uint32_t n = lg_mesh_tet_count(m4);
    if (n == 0u) return 0u;
    const uint32_t w4 = ~m4 & 15u;                                 // the outside corners
#define LG_MESH_LOWEST(m) (((m) & 1u) ? 0u : (((m) & 2u) ? 1u : (((m) & 4u) ? 2u : 3u)))
#define LG_MESH_HIGHEST(m) (((m) & 8u) ? 3u : (((m) & 4u) ? 2u : (((m) & 2u) ? 1u : 0u)))
#define LG_MESH_EDGE(u, v) ((u) < (v) ? ((u) | ((v) << 2)) : ((v) | ((u) << 2)))
    if (n == 1u) {
        const uint32_t a = lg_mesh_popc8(m4) == 1u ? LG_MESH_LOWEST(m4) : LG_MESH_LOWEST(w4);
        for (uint32_t v = 0; v < 3u; v++) { const uint32_t o = v + (v >= a ? 1u : 0u); tri[0][v] = LG_MESH_EDGE(a, o); }
    } else {
        const uint32_t in0 = LG_MESH_LOWEST(m4), in1 = LG_MESH_HIGHEST(m4), out0 = LG_MESH_LOWEST(w4), out1 = LG_MESH_HIGHEST(w4);
        const uint32_t q0 = LG_MESH_EDGE(in0, out0), q1 = LG_MESH_EDGE(in0, out1), q2 = LG_MESH_EDGE(in1, out1), q3 = LG_MESH_EDGE(in1, out0);
        tri[0][0] = q0; tri[0][1] = q1; tri[0][2] = q2;
        tri[1][0] = q0; tri[1][1] = q2; tri[1][2] = q3;
    }
#undef LG_MESH_EDGE
#undef LG_MESH_LOWEST
#undef LG_MESH_HIGHEST
    const uint32_t word = (t == 0u || t == 3u || t == 4u) ? LG_MESH_FLIP_EVEN : LG_MESH_FLIP_ODD;
    if ((word >> m4) & 1u)
        for (uint32_t j = 0; j < n; j++) { const uint32_t s = tri[j][1]; tri[j][1] = tri[j][2]; tri[j][2] = s; }
    return n;
}
// The faces of the valid cell at (x, y, z) with corner bits inside8, written to faces[3 j + v] in order: vprefix[p] = vertex id of the
// first carrying slot of point p, vmask[p] = its lg_mesh_edge_mask; `room` = faces the buffer holds from `faces` on (one past it is not
// written).  Returns their number (= lg_mesh_cell_count).
LG_HD uint32_t lg_mesh_cell_faces(int nx, int ny, int x, int y, int z, uint32_t inside8, const uint32_t* vprefix, const uint8_t* vmask, int32_t* faces,
                                  int64_t room)
{
    uint32_t nf = 0u;
    for (uint32_t t = 0; t < 6u; t++) {
        uint32_t tri[2][3];
        const uint32_t n = lg_mesh_tet_triangles(t, lg_mesh_tet_inside(t, inside8), tri);
        for (uint32_t j = 0; j < n; j++, nf++)
            for (uint32_t v = 0; v < 3u; v++) {
                const uint32_t c0 = lg_mesh_tet_corner(t, tri[j][v] & 3u), c1 = lg_mesh_tet_corner(t, tri[j][v] >> 2);
                const size_t q = lg_mesh_index(nx, ny, x + (int)(c0 & 1u), y + (int)((c0 >> 1) & 1u), z + (int)((c0 >> 2) & 1u));
                const uint32_t k = lg_mesh_mask_slot(c1 ^ c0);
                if ((int64_t)nf < room) faces[3u * nf + v] = (int32_t)(vprefix[q] + lg_mesh_popc8((uint32_t)vmask[q] & ((1u << k) - 1u)));
            }
    }
    return nf;
}

// ---------------------------------------------------------------------------------------------
// Sensitivity pruning score (lg_sensitivity.h, include/lightgaussian_sensitivity.h): the per-Gaussian 6 x 6 block
//   H_i = sum_views sum_pixels sum_channels (dI_c/dtheta_i)(dI_c/dtheta_i)^T,   theta_i = (mean3D, activated scale),
// of the Gauss-Newton Hessian of the L2 reconstruction error, colours held constant, and score = log det H_i.  A pixel depends on theta_i
// through the 2D mean and the conic only, so dI_c/dtheta_i = v_c G u^T B A with
//   v_c = (c_c - S_c) Tn - T_final bg_c / (1 - alpha)      lg_feature_bwd_step's dL/dalpha with q = c_c, Tfb = T_final bg_c, per channel
//   u   = (dx, dy, dx^2, dx dy, dy^2)                      the monomials of its moments m[0..4]
//   B                                                      lg_rows_to_grads' per-Gaussian coefficients: acc[0..4] = B (t u), t = G v_c
//   A   [5][6]                                             row k = lg_backward_geom_t<false> + lg_backward_cov3d of acc = e_k (the chain is linear in acc)
// and H_i(view) = A^T M A, M = B U B^T, U = sum_pixels w u u^T, w = |v|^2 G^2.  U's entries are the twelve moments sum w dx^a dy^b,
// 2 <= a + b <= 4 -- non-negative multiples of monomials, no cancellation in their sums -- in the order of LG_SENS_MOMENTS below.
#define LG_SENS_NV 12           // dx2, dxdy, dy2 | dx3, dx2dy, dxdy2, dy3 | dx4, dx3dy, dx2dy2, dxdy3, dy4
#define LG_SENS_H 21            // the upper triangle of a 6 x 6 block, row-major
#define LG_SENS_PIVOT_MIN 0x1p-26

// One (pixel, entry) step of the back-to-front replay: lg_feature_bwd_step's decisions and recurrences for three colour channels at
// once (c = the entry's colour, Tfb[k] = T_final bg[k], S[k] = the colour blended behind the entry, starts at 0; T starts at final_T),
// then m[0..11] += w {monomials}.  Straight through the 0.99 clamp; power > 0 and alpha < 1/255 take no part.  Returns false (nothing
// touched) when the entry does not contribute.  EXACT = false on the device: v_rcp_f32 for 1 / (1 - alpha), as K7's fast path.
template <bool EXACT>
LG_HD bool lg_sensitivity_step(bool live, float power, float G, float alpha, float dx, float dy, const float* c, const float* Tfb, float& T,
                               float* S, float* m)
{
    if (!live || !(power <= 0.0f) || alpha < LG_ALPHA_MIN) return false;
#if defined(__HIP_DEVICE_COMPILE__)
    const float inv = EXACT ? 1.0f / (1.0f - alpha) : __builtin_amdgcn_rcpf(1.0f - alpha);
#else
    const float inv = 1.0f / (1.0f - alpha);
#endif
    const float Tn = T * inv;
    float vv = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float d = c[k] - S[k];
        const float v = d * Tn - Tfb[k] * inv;
        vv += v * v;
        S[k] = S[k] + alpha * d;
    }
    const float w = vv * (G * G);
    const float xx = dx * dx, xy = dx * dy, yy = dy * dy;
    const float wxx = w * xx, wxy = w * xy, wyy = w * yy;
    m[0] += wxx;
    m[1] += wxy;
    m[2] += wyy;
    m[3] += wxx * dx;
    m[4] += wxx * dy;
    m[5] += wyy * dx;
    m[6] += wyy * dy;
    m[7] += wxx * xx;
    m[8] += wxx * xy;
    m[9] += wxx * yy;
    m[10] += wyy * xy;
    m[11] += wyy * yy;
    T = Tn;
    return true;
}

// moments -> M = B U B^T (upper triangle, row-major [15]), float64.  U[a][b] = sum w u_a u_b read from the twelve moments; B from the
// record's conic (ha = -A/2, nb = -B, hc = -C/2) and opacity, lg_rows_to_grads' coefficients:
//   acc0 = op (2 ha u0 + nb u1)   acc1 = op (nb u0 + 2 hc u1)   acc2 = -op u2 / 2   acc3 = -op u3   acc4 = -op u4 / 2
LG_HD void lg_sensitivity_moments_to_M(const double* mo, float ha, float nb, float hc, float op, double* M)
{
    const double U[5][5] = {
        { mo[0], mo[1], mo[3], mo[4], mo[5] },
        { mo[1], mo[2], mo[4], mo[5], mo[6] },
        { mo[3], mo[4], mo[7], mo[8], mo[9] },
        { mo[4], mo[5], mo[8], mo[9], mo[10] },
        { mo[5], mo[6], mo[9], mo[10], mo[11] } };
    const double o = (double)op;
    const double p = 2.0 * (double)ha * o, q = (double)nb * o, r = 2.0 * (double)hc * o;
    const double d[3] = { -0.5 * o, -o, -0.5 * o };
    // rows 0, 1 of B U: the 2 x 2 block mixes u0, u1; rows 2..4 scale
    double BU[5][5];
    for (int b = 0; b < 5; b++) {
        BU[0][b] = p * U[0][b] + q * U[1][b];
        BU[1][b] = q * U[0][b] + r * U[1][b];
        BU[2][b] = d[0] * U[2][b];
        BU[3][b] = d[1] * U[3][b];
        BU[4][b] = d[2] * U[4][b];
    }
    int k = 0;
    for (int a = 0; a < 5; a++)
        for (int b = a; b < 5; b++, k++) {
            if (b == 0) M[k] = BU[a][0] * p + BU[a][1] * q;
            else if (b == 1) M[k] = BU[a][0] * q + BU[a][1] * r;
            else M[k] = BU[a][b] * d[b - 2];
        }
}

// H[21] += A^T M A (upper triangle, row-major), float64: A [5][6] float32 (the chain's own precision), M [15] from above.
LG_HD void lg_sensitivity_AtMA(const float (*A)[6], const double* M, double* H)
{
    double Mf[5][5];
    int k = 0;
    for (int a = 0; a < 5; a++)
        for (int b = a; b < 5; b++, k++) { Mf[a][b] = M[k]; Mf[b][a] = M[k]; }
    double MA[5][6];
    for (int a = 0; a < 5; a++)
        for (int j = 0; j < 6; j++) {
            double s = 0.0;
            for (int b = 0; b < 5; b++) s += Mf[a][b] * (double)A[b][j];
            MA[a][j] = s;
        }
    k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++, k++) {
            double s = 0.0;
            for (int a = 0; a < 5; a++) s += (double)A[a][i] * MA[a][j];
            H[k] += s;
        }
}

// log det of a 6 x 6 block given as its upper triangle [21]: Cholesky H = L L^T in float64, 2 sum_k log L_kk; -inf at the first pivot
// that is not positive.  "Not positive" is taken up to the rounding the block carries: a pivot must exceed LG_SENS_PIVOT_MIN (2^-26) of
// its diagonal entry.  A block of rank 5 (one view: A has five rows) leaves a last pivot of either sign, measured up to 5e-11 of the
// diagonal entry on the golden scene (float64 rounding times the growth of the elimination); and A and the moments are float32, so a
// pivot below 2^-26 of its diagonal is below what the inputs resolve.
LG_HD double lg_sensitivity_logdet(const double* H)
{
    double L[6][6];
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++, k++) L[j][i] = H[k];        // lower triangle holds the block
    double s = 0.0;
    for (int j = 0; j < 6; j++) {
        const double ajj = L[j][j];
        double d = ajj;
        for (int u = 0; u < j; u++) d -= L[j][u] * L[j][u];
        if (!(d > LG_SENS_PIVOT_MIN * ajj) || !(ajj > 0.0)) return -(double)INFINITY;
        const double l = sqrt(d);
        L[j][j] = l;
        s += log(l);
        for (int i = j + 1; i < 6; i++) {
            double t = L[i][j];
            for (int u = 0; u < j; u++) t -= L[i][u] * L[j][u];
            L[i][j] = t / l;
        }
    }
    return 2.0 * s;
}

// ---------------------------------------------------------------------------------------------
// Sparse block TSDF volume (include/lightgaussian_blocks.h; lg_blocks.h's kernels and
// tests/cpu_harness/lg_blocks_harness.cpp call the same functions).
//
// The lattice is unbounded: point (i, j, k) lies at lg_tsdf_coord(origin, voxel, i) per axis, the dense expression with the GLOBAL
// index.  A block is 8 x 8 x 8 points, block coordinate b = floor(i / 8) in [-2^20, 2^20) per axis; the volume is the list of its
// blocks' keys in strictly ascending order and storage follows that order, x fastest inside a block.  Integration per point is the
// text of the dense volume above (lg_tsdf_project / _sample / _apply); the marching tetrahedra run lg_mesh_*'s rule functions on the
// 9 x 9 x 9 halo of a block (its own points and the first layer of its seven + neighbours; a missing neighbour is unobserved).
#define LG_BLK 8
#define LG_BLK_POINTS 512
#define LG_BLK_BIAS (1 << 20)                  // block coordinates are stored as b + 2^20 in 21 bits
#define LG_BLK_INDEX_LIMIT 8388608.0f          // lattice indices stay in [-2^23, 2^23): exact as floats, block coordinates in range
#define LG_BLK_MAX_SPAN 4                      // blocks a pixel may touch per axis
#define LG_BLK_HALO 9
#define LG_BLK_HALO_POINTS 729
LG_HD int64_t lg_blk_key(int bx, int by, int bz)
{
    return ((int64_t)(bz + LG_BLK_BIAS) << 42) | ((int64_t)(by + LG_BLK_BIAS) << 21) | (int64_t)(bx + LG_BLK_BIAS);
}
LG_HD void lg_blk_coords(int64_t key, int& bx, int& by, int& bz)
{
    bx = (int)(key & 0x1FFFFF) - LG_BLK_BIAS; by = (int)((key >> 21) & 0x1FFFFF) - LG_BLK_BIAS; bz = (int)((key >> 42) & 0x1FFFFF) - LG_BLK_BIAS;
}
LG_HD int lg_blk_of_index(int i) { return i >> 3; }            // floor(i / 8): the shift of a negative int is arithmetic on every target here
LG_HD int lg_blk_local(int x, int y, int z) { return (z * LG_BLK + y) * LG_BLK + x; }

// The blocks a pixel touches: lo[a] is the first block along axis a and n[a] (1 .. 4) their number.
struct LgBlkBox { int lo[3], n[3]; };
// Pixel (ix, iy) with depth d (and alpha, read only with has_alpha) of a view, in this order:
//   gates        d > 0 and finite; d <= depth_max where depth_max > 0; alpha >= alpha_min where an alpha map is given     else: 0
//   r            (((2 ix + 1) / W - 1) tanfovx, ((2 iy + 1) / H - 1) tanfovy, 1): the ray through the pixel centre, z = 1
//   za, zb       d - trunc, d + trunc
//   pad          voxel + zb sqrt((tanfovx / W)^2 + (tanfovy / H)^2): one voxel for the extraction's + neighbours, and the half
//                diagonal of the pixel's footprint at the far end of the band
//   a_w, b_w     the world points of r za and r zb under a RIGID view matrix: p[a] = sum_c (p_v[c] - vm[12 + c]) vm[4 a + c]
//   per axis     lo = min(a_w, b_w) - pad, hi = max(a_w, b_w) + pad; lattice indices floor((. - origin) / voxel), which must lie in
//                [-2^23, 2^23) (a NaN fails); blocks floor(. / 8); more than 4 blocks along an axis                           else: 2
// Returns 1 with the box, 2 for a pixel that is skipped (and counted), 0 for one that takes no part.
LG_HD int lg_blk_touch(const float* vm, const LgTsdfCam& c, const float* origin, float voxel, float trunc, int ix, int iy, float d, bool has_alpha,
                       float alpha, LgBlkBox& box)
{
    if (!(d > 0.0f) || !(d <= 3.402823466e+38f)) return 0;
    if (c.depth_max > 0.0f && d > c.depth_max) return 0;
    if (has_alpha && alpha < c.alpha_min) return 0;
    const float rx = ((float)(2 * ix + 1) / (float)c.W - 1.0f) * c.tanfovx;
    const float ry = ((float)(2 * iy + 1) / (float)c.H - 1.0f) * c.tanfovy;
    const float za = d - trunc, zb = d + trunc;
    const float fw = c.tanfovx / (float)c.W, fh = c.tanfovy / (float)c.H;
    const float pad = voxel + zb * sqrtf(fw * fw + fh * fh);
    const float ax = rx * za - vm[12], ay = ry * za - vm[13], az = za - vm[14];
    const float bx = rx * zb - vm[12], by = ry * zb - vm[13], bz = zb - vm[14];
    for (int a = 0; a < 3; a++) {
        const float wa = ax * vm[4 * a] + ay * vm[4 * a + 1] + az * vm[4 * a + 2];
        const float wb = bx * vm[4 * a] + by * vm[4 * a + 1] + bz * vm[4 * a + 2];
        const float lo = fminf(wa, wb) - pad, hi = fmaxf(wa, wb) + pad;
        const float flo = floorf((lo - origin[a]) / voxel), fhi = floorf((hi - origin[a]) / voxel);
        if (!(flo >= -LG_BLK_INDEX_LIMIT && fhi < LG_BLK_INDEX_LIMIT && flo <= fhi)) return 2;
        const int blo = lg_blk_of_index((int)flo), bhi = lg_blk_of_index((int)fhi);
        if (bhi - blo + 1 > LG_BLK_MAX_SPAN) return 2;
        box.lo[a] = blo; box.n[a] = bhi - blo + 1;
    }
    return 1;
}

// The halo of a block: point (x, y, z), each 0 .. 8, at (z 9 + y) 9 + x; it lives in the + neighbour m = (x == 8) | (y == 8) << 1 |
// (z == 8) << 2 of the block (m = 0: the block itself) at the local index of (x & 7, y & 7, z & 7).
LG_HD int lg_blk_halo_index(int x, int y, int z) { return (z * LG_BLK_HALO + y) * LG_BLK_HALO + x; }
LG_HD void lg_blk_halo_source(int h, uint32_t& m, int& local)
{
    const int x = h % LG_BLK_HALO, y = (h / LG_BLK_HALO) % LG_BLK_HALO, z = h / (LG_BLK_HALO * LG_BLK_HALO);
    m = (x == LG_BLK ? 1u : 0u) | (y == LG_BLK ? 2u : 0u) | (z == LG_BLK ? 4u : 0u);
    local = lg_blk_local(x & 7, y & 7, z & 7);
}
// The vertex on slot k of the lattice point (gx, gy, gz), GLOBAL indices: lg_mesh_edge_vertex under the name that
// tests/cpu_harness/lg_blocks_harness.cpp calls.  It exists for that harness alone: no kernel calls it.
LG_HD void lg_blk_vertex(float f0v, float f1v, const float* c0, const float* c1, int gx, int gy, int gz, uint32_t k, float iso, const float* origin,
                         float voxel, float* pos, float* rgb)
{
    lg_mesh_edge_vertex(f0v, f1v, c0, c1, gx, gy, gz, k, iso, origin, voxel, pos, rgb);
}
