// What the host checks of the FP32 filter share (check_filter.cpp, check_envelope.cpp): the random
// stream, v_rsq_f32's emulated 1-ulp error, the kernel's spline evaluation in both precisions and the
// SAT separations in either precision.  Include after defining SSPF_HOST_RSQ_JITTER and sspp_filter.h.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

static std::mt19937_64 g_rng(20261018);
static std::uniform_real_distribution<double> U01(0.0, 1.0);
float sspf::rsq_jitter() { return 1.0f + (float)((U01(g_rng) * 2.0 - 1.0) * 1.2e-7); }

static double U(double a, double b) { return a + (b - a) * U01(g_rng); }

// eval_split's operation order: acc = N0 c0, acc = fma(Nr, cr, acc)
static void spline4(const double N[4], const double c[4][7], int D, double* qd, float* q32) {
    for (int d = 0; d < D; ++d) {
        double a = N[0] * c[0][d];
        float f = (float)N[0] * (float)c[0][d];
        for (int r = 1; r < 4; ++r) {
            a = fma(N[r], c[r][d], a);
            f = fmaf((float)N[r], (float)c[r][d], f);
        }
        qd[d] = a;
        q32[d] = f;
    }
}

// the 15 SAT quantities FP64 and FP32 compare with the margin (sat_box_box's formulas, both
// precisions), for the error measurement: max |FP32 - FP64| over axes FP64 evaluates
template <class T>
static void sat_seps(const T* pa, const T* ma, const T* ea, const T* pb, const T* mb, const T* eb, T* out, bool* used) {
    const T Tv[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
    T t[3], R[3][3];
    for (int i = 0; i < 3; ++i) {
        t[i] = ma[i] * Tv[0] + ma[3 + i] * Tv[1] + ma[6 + i] * Tv[2];
        for (int j = 0; j < 3; ++j) R[i][j] = ma[i] * mb[j] + ma[3 + i] * mb[3 + j] + ma[6 + i] * mb[6 + j];
    }
    int o = 0;
    for (int i = 0; i < 3; ++i) {
        out[o] = std::fabs(t[i]) - (ea[i] + eb[0] * std::fabs(R[i][0]) + eb[1] * std::fabs(R[i][1]) + eb[2] * std::fabs(R[i][2]));
        used[o++] = true;
    }
    for (int j = 0; j < 3; ++j) {
        out[o] = std::fabs(t[0] * R[0][j] + t[1] * R[1][j] + t[2] * R[2][j]) -
                 (ea[0] * std::fabs(R[0][j]) + ea[1] * std::fabs(R[1][j]) + ea[2] * std::fabs(R[2][j]) + eb[j]);
        used[o++] = true;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            T L[3];
            if (i == 0) { L[0] = 0; L[1] = -R[2][j]; L[2] = R[1][j]; }
            else if (i == 1) { L[0] = R[2][j]; L[1] = 0; L[2] = -R[0][j]; }
            else { L[0] = -R[1][j]; L[1] = R[0][j]; L[2] = 0; }
            const T len2 = L[0] * L[0] + L[1] * L[1] + L[2] * L[2];
            T rb = 0;
            for (int k = 0; k < 3; ++k) rb += eb[k] * std::fabs(R[0][k] * L[0] + R[1][k] * L[1] + R[2][k] * L[2]);
            out[o] = std::fabs(t[0] * L[0] + t[1] * L[1] + t[2] * L[2]) -
                     (ea[0] * std::fabs(L[0]) + ea[1] * std::fabs(L[1]) + ea[2] * std::fabs(L[2]) + rb);
            used[o++] = len2 >= (T)1e-10;
        }
}

static void rand_quat(double* q) {
    double s = 0;
    for (int k = 0; k < 4; ++k) { q[k] = U(-1, 1); s += q[k] * q[k]; }
    s = std::sqrt(s);
    for (int k = 0; k < 4; ++k) q[k] /= s;
}
