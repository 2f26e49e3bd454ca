// sspp_rng.h — the kernels' random numbers (sspp_kern.h): Philox4x32-10, the FP64 and FP32
// Box-Muller normals and sampleWithNoise in work items (sample_item_to).
#pragma once
#include <hip/hip_runtime.h>

#include "sspp_logtab.h"

namespace sspk {

// ---------------------------------------------------------------- Philox4x32-10 + Box-Muller
__device__ __forceinline__ void philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                       unsigned k0, unsigned k1, unsigned o[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        // one 32 x 32 -> 64-bit multiply per product (v_mad_u64_u32): hi and lo together
        const unsigned long long p0 = (unsigned long long)c0 * 0xD2511F53u;
        const unsigned long long p1 = (unsigned long long)c2 * 0xCD9E8D57u;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ void philox_words(unsigned long long seed, unsigned long long g,
                                             unsigned idx, unsigned stream, unsigned o[4]) {
    philox(idx, stream, (unsigned)g, (unsigned)(g >> 32), (unsigned)seed, (unsigned)(seed >> 32), o);
}
// FP64 Box-Muller (the default sampler of both planners; std::normal_distribution<double> in the
// reference, include/sspp.h:116,125 and include/sspp/tsp_sampler.h:17): one Philox4x32-10 call
// gives two 53-bit uniforms u1 in (0, 1], u2 in [0, 1) -> z0 = r cos(2 pi u2), z1 = r sin(2 pi u2),
// r = sqrt(-2 ln u1), |z| <= 8.57.  ln and sincos are written out as FP64 polynomials with
// explicit fma (sin / cos: Taylor on |a| <= pi/4 to a^17 / a^16), an IEEE sqrt, and no division:
// ln u = e ln 2 + ln m with m = k/64 (1 + t), k = round(64 m) — a 64-entry table (sspp_logtab.h,
// tools/gen_log_table.py) holds r = RN(64/k) and -ln r as hi + lo, t = fma(m, r, -1) is one
// rounding with |t| <= 2^-7, and ln(1 + t) is its series to t^8 (remainder < 2e-20).  m near 2
// takes the next exponent's entry k = 64 (r = 1, t = m/2 - 1 exact), so ln u keeps its relative
// precision as u -> 1.  (Round 5 computed ln m by the atanh series of s = (m-1)/(m+1), an IEEE
// FP64 division: v_div_scale x2, v_rcp_f64, four fma, v_div_fmas / fixup per pair.)
// oracle/sspp_oracle.c::or_normal_pair reproduces every normal bit for bit.
__device__ __forceinline__ double bm_log64(double u) {  // ln u, u in [2^-53, 1]
    static const double tab[64][4] = {SSPP_LOGTAB_ENTRIES};
    const unsigned long long bits = (unsigned long long)__double_as_longlong(u);
    const unsigned long long mb = bits & 0x000fffffffffffffull;
    int e = (int)(bits >> 52) - 1023;
    int k = (int)((mb + (1ull << 45)) >> 46);  // round(64 m) - 64, 0..64
    double m = __longlong_as_double((long long)(mb | 0x3ff0000000000000ull));
    if (k == 64) { k = 0; e += 1; m = m * 0.5; }  // m in [2 - 2^-7, 2): its half, next to 1
    const double t = fma(m, tab[k][0], -1.0);     // m r - 1
    const double t2 = t * t;
    double p = -0.125;                             // -1/8
    p = fma(t, p, 0x1.2492492492492p-3);           // 1/7
    p = fma(t, p, -0x1.5555555555555p-3);          // -1/6
    p = fma(t, p, 0x1.999999999999ap-3);           // 1/5
    p = fma(t, p, -0.25);                          // -1/4
    p = fma(t, p, 0x1.5555555555555p-2);           // 1/3
    p = fma(t, p, -0.5);                           // -1/2
    const double l1 = fma(t2, p, t);               // ln(1 + t)
    const double de = (double)e;                   // ln 2 = hi + lo (hi: 42 bits, e hi exact)
    const double hi = fma(de, 0x1.62e42fefa3800p-1, tab[k][1]);
    const double lo = fma(de, 0x1.ef35793c76730p-45, tab[k][2]) + l1;
    return hi + lo;
}
__device__ __forceinline__ void bm_sincos2pi64(double u, double* sn, double* cs) {  // u in [0, 1)
    const double q = rint(4.0 * u);
    const double r = fma(-0.25, q, u);         // exact, |r| <= 1/8
    const double a = r * 0x1.921fb54442d18p+2; // 2 pi r, |a| <= pi/4
    const double a2 = a * a;
    double sp = 0x1.952c77030ad4ap-49;         // 1/17!
    sp = fma(a2, sp, -0x1.ae7f3e733b81fp-41);
    sp = fma(a2, sp, 0x1.6124613a86d09p-33);
    sp = fma(a2, sp, -0x1.ae64567f544e4p-26);
    sp = fma(a2, sp, 0x1.71de3a556c734p-19);
    sp = fma(a2, sp, -0x1.a01a01a01a01ap-13);
    sp = fma(a2, sp, 0x1.1111111111111p-7);
    sp = fma(a2, sp, -0x1.5555555555555p-3);   // -1/3!
    const double sa = fma(a * a2, sp, a);
    double cp = 0x1.ae7f3e733b81fp-45;         // 1/16! (the a^18 term: < 2.1e-18 on |a| <= pi/4)
    cp = fma(a2, cp, -0x1.93974a8c07c9dp-37);
    cp = fma(a2, cp, 0x1.1eed8eff8d898p-29);
    cp = fma(a2, cp, -0x1.27e4fb7789f5cp-22);
    cp = fma(a2, cp, 0x1.a01a01a01a01ap-16);
    cp = fma(a2, cp, -0x1.6c16c16c16c17p-10);
    cp = fma(a2, cp, 0x1.5555555555555p-5);
    cp = fma(a2, cp, -0x1.0000000000000p-1);   // -1/2!
    const double ca = fma(a2, cp, 1.0);
    const int qi = (int)q & 3;
    *sn = qi == 0 ? sa : (qi == 1 ? ca : (qi == 2 ? -sa : -ca));
    *cs = qi == 0 ? ca : (qi == 1 ? -sa : (qi == 2 ? -ca : sa));
}
__device__ __forceinline__ void normal_pair(unsigned long long seed, unsigned long long g,
                                            unsigned idx, unsigned stream, double* z0, double* z1) {
    unsigned o[4];
    philox_words(seed, g, idx, stream, o);
    const unsigned long long a = ((((unsigned long long)o[0]) << 32) | o[1]) >> 11;
    const unsigned long long b = ((((unsigned long long)o[2]) << 32) | o[3]) >> 11;
    const double u1 = (double)(a + 1) * 0x1p-53;  // (0, 1], exact
    const double u2 = (double)b * 0x1p-53;        // [0, 1), exact
    const double r = sqrt(-2.0 * bm_log64(u1));
    double sn, cs;
    bm_sincos2pi64(u2, &sn, &cs);
    *z0 = r * cs;
    *z1 = r * sn;
}
// Opt-in FP32 SamplingPathPlanner normals (sspp_sspp_args::sampler = 1, the round-2 default): one
// Philox4x32-10 call gives four 24-bit uniforms -> two Box-Muller pairs in FP32, with fmaf
// polynomials written out (ln u by the atanh series on the mantissa, sin / cos of 2 pi u after an
// exact quarter-turn reduction) and a correctly rounded sqrtf, so
// oracle/sspp_oracle.c::or_normal_quad reproduces it bit for bit.  |z| <= 5.77 (u1 >= 2^-24):
// narrower than the reference's std::normal_distribution<double>, hence not the default.
__device__ __forceinline__ float bm_log(float u) {  // ln u, u in [2^-24, 1]
    const unsigned bits = __float_as_uint(u);
    int e = (int)(bits >> 23) - 127;
    float m = __uint_as_float((bits & 0x7fffffu) | 0x3f800000u);  // [1, 2)
    if (m > 1.41421356f) { m = m * 0.5f; e += 1; }
    const float s = (m - 1.0f) / (m + 1.0f);                      // |s| <= 0.1716
    const float s2 = s * s;
    float p = fmaf(s2, 0.111111111f, 0.142857143f);
    p = fmaf(s2, p, 0.2f);
    p = fmaf(s2, p, 0.333333333f);
    p = fmaf(s2, p, 1.0f);
    return fmaf((float)e, 0.693147181f, (s + s) * p);
}
__device__ __forceinline__ void bm_sincos2pi(float u, float* sn, float* cs) {  // u in [0, 1)
    const float q = rintf(4.0f * u);
    const float r = fmaf(-0.25f, q, u);  // exact
    const float a = r * 6.28318531f;     // |a| <= pi / 4
    const float a2 = a * a;
    float sp = fmaf(a2, 2.75573192e-6f, -1.98412698e-4f);
    sp = fmaf(a2, sp, 8.33333333e-3f);
    sp = fmaf(a2, sp, -0.166666667f);
    const float sa = fmaf(a * a2, sp, a);
    float cp = fmaf(a2, 2.48015873e-5f, -1.38888889e-3f);
    cp = fmaf(a2, cp, 4.16666667e-2f);
    cp = fmaf(a2, cp, -0.5f);
    const float ca = fmaf(a2, cp, 1.0f);
    const int qi = (int)q & 3;
    *sn = qi == 0 ? sa : (qi == 1 ? ca : (qi == 2 ? -sa : -ca));
    *cs = qi == 0 ? ca : (qi == 1 ? -sa : (qi == 2 ? -ca : sa));
}
__device__ __forceinline__ void normal_quad(unsigned long long seed, unsigned long long g,
                                            unsigned idx, unsigned stream, double z[4]) {
    unsigned o[4];
    philox_words(seed, g, idx, stream, o);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = (float)((o[2 * h] >> 8) + 1u) * 5.96046448e-8f;  // (0, 1], exact
        const float u2 = (float)(o[2 * h + 1] >> 8) * 5.96046448e-8f;     // [0, 1), exact
        const float r = sqrtf(-2.0f * bm_log(u1));
        float sn, cs;
        bm_sincos2pi(u2, &sn, &cs);
        z[2 * h] = (double)(r * cs);
        z[2 * h + 1] = (double)(r * sn);
    }
}
__device__ __forceinline__ double uniform01(unsigned long long seed, unsigned long long g,
                                            unsigned idx, unsigned stream) {
    unsigned o[4];
    philox_words(seed, g, idx, stream, o);
    unsigned long long b = ((((unsigned long long)o[2]) << 32) | o[3]) >> 11;
    return (double)b * 1.1102230246251565e-16;
}

// sampleWithNoise (include/sspp.h:114-130) in work items: item m of a candidate draws normals
// 2m, 2m+1 (sampler 0: FP64 pair, Philox idx m) or 4m .. 4m+3 (sampler 1: FP32 quad) and adds
// (sigma z) limits(d) to the initial spline's perturbed control-point block `base` (row-major
// (j - p) * D + d), writing the candidate's block c: c[k] = base[k] + (sigma z_k) limits[k % D].
__device__ __forceinline__ int sample_items(int sampler, int npert) {
    return sampler ? (npert + 3) >> 2 : (npert + 1) >> 1;
}
// c32 (optional): the FP32 copy of the same values (k_sspp_c2f's filtered scan)
__device__ __forceinline__ void sample_item_to(int sampler, unsigned long long seed, unsigned long long g,
                                               int m, int npert, int D, double sigma,
                                               const double* limits, const double* base, double* c,
                                               float* c32 = nullptr) {
    if (sampler == 0) {
        double z0, z1;
        normal_pair(seed, g, (unsigned)m, 0u, &z0, &z1);
        const int k = 2 * m;
        const double v0 = base[k] + (sigma * z0) * limits[k % D];
        c[k] = v0;
        if (c32) c32[k] = (float)v0;
        if (k + 1 < npert) {
            const double v1 = base[k + 1] + (sigma * z1) * limits[(k + 1) % D];
            c[k + 1] = v1;
            if (c32) c32[k + 1] = (float)v1;
        }
    } else {
        double z[4];
        normal_quad(seed, g, (unsigned)m, 0u, z);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int k = 4 * m + h;
            if (k < npert) {
                const double v = base[k] + (sigma * z[h]) * limits[k % D];
                c[k] = v;
                if (c32) c32[k] = (float)v;
            }
        }
    }
}

}  // namespace sspk
