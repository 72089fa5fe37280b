// ransac_device.hpp -- the device side both RANSAC translation units share (ransac.hip: one solve; ransac_pairs.hip: a batch
// of pairs): the sampler, the hypothesis, the point test, the host-side argument checks.  The bodies of the score and
// the finalize kernels are ransac_score_body.hpp and ransac_finalize_body.hpp.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.hpp"

namespace micv {
namespace {

constexpr int kWaves = 4;      // 256-thread workgroups
constexpr int kChunk = 32;     // hypotheses per workgroup chunk (8 per wave)
constexpr int kLdsMax = 4096;  // matches staged in LDS (16 B each)

// ctl words (device): [0] n, [1] first stop iteration seen (unsigned; ~0 = none), [2] bad-input flag.
__device__ inline uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The sample of iteration h: the caller's, or the counter-based sampler of mi_cv.h.  Unused entries
// are -1.  Returns false when a caller's index is outside [0, n).
__device__ inline bool draw_sample(const int32_t *samples, uint64_t seed, int h, int k, int n, int s[3]) {
    s[0] = s[1] = s[2] = -1;
    if (samples) {
        for (int j = 0; j < k; j++) {
            s[j] = samples[(size_t)h * k + j];
            if (s[j] < 0 || s[j] >= n) return false;
        }
        return true;
    }
    for (int j = 0; j < k; j++) {
        for (uint32_t a = 0;; a++) {
            const uint64_t r = splitmix64(seed ^ (((uint64_t)(uint32_t)h << 32) | ((uint64_t)j << 30) | a));
            const int idx = (int)(((r >> 32) * (uint64_t)(uint32_t)n) >> 32);
            bool dup = false;
            for (int e = 0; e < j; e++) dup |= s[e] == idx;
            if (!dup) {
                s[j] = idx;
                break;
            }
        }
    }
    return true;
}

// cv::solve(A, b, x, DECOMP_LU) on the 4x4 float system of RANSAC.cpp:75-86: hal::LU32f, partial
// pivoting (first row of largest |a|), failure below 10 * FLT_EPSILON -> x = 0.
__device__ inline void lu4_solve(float A[4][4], float b[4]) {
    const float eps = FLT_EPSILON * 10;
    for (int i = 0; i < 4; i++) {
        int k = i;
        for (int j = i + 1; j < 4; j++)
            if (fabsf(A[j][i]) > fabsf(A[k][i])) k = j;
        if (fabsf(A[k][i]) < eps) {
            b[0] = b[1] = b[2] = b[3] = 0.f;
            return;
        }
        if (k != i) {
            for (int j = i; j < 4; j++) {
                const float t = A[i][j];
                A[i][j] = A[k][j];
                A[k][j] = t;
            }
            const float t = b[i];
            b[i] = b[k];
            b[k] = t;
        }
        const float d = -1.f / A[i][i];
        for (int j = i + 1; j < 4; j++) {
            const float alpha = A[j][i] * d;
            for (int c = i + 1; c < 4; c++) A[j][c] = A[j][c] + alpha * A[i][c];
            b[j] = b[j] + alpha * b[i];
        }
    }
    for (int i = 3; i >= 0; i--) {
        float s = b[i];
        for (int c = i + 1; c < 4; c++) s = s - A[i][c] * b[c];
        b[i] = s / A[i][i];
    }
}

// The hypothesis of RANSAC.cpp:56-117 from the k sample points q[j] = (x, y, x', y').
__device__ inline void hypothesis(int type, const float4 q[3], float t[6]) {
    if (type == MICV_RANSAC_TRANSLATION) {
        t[0] = 1.f; t[1] = 0.f; t[2] = q[0].z - q[0].x;
        t[3] = 0.f; t[4] = 1.f; t[5] = q[0].w - q[0].y;
        return;
    }
    if (type == MICV_RANSAC_SIMILARITY) {
        float A[4][4] = {{q[0].x, -q[0].y, 1.f, 0.f},
                         {q[0].y, q[0].x, 0.f, 1.f},
                         {q[1].x, -q[1].y, 1.f, 0.f},
                         {q[1].y, q[1].x, 0.f, 1.f}};
        float b[4] = {q[0].z, q[0].w, q[1].z, q[1].w};
        lu4_solve(A, b);
        t[0] = b[0]; t[1] = -b[1]; t[2] = b[2];
        t[3] = b[1]; t[4] = b[0]; t[5] = b[3];
        return;
    }
    // AFFINE: Pprime * P.inv(), rows 0..1.  P.inv(): the closed form of cv::invert for 3x3 CV_32F
    // (determinant and cofactors in double, each rounded to float once; zeros when det == 0).
    const float P[3][3] = {{q[0].x, q[1].x, q[2].x}, {q[0].y, q[1].y, q[2].y}, {1.f, 1.f, 1.f}};
    const float Pp[2][3] = {{q[0].z, q[1].z, q[2].z}, {q[0].w, q[1].w, q[2].w}};
    double d = P[0][0] * ((double)P[1][1] * P[2][2] - (double)P[1][2] * P[2][1]) -
               P[0][1] * ((double)P[1][0] * P[2][2] - (double)P[1][2] * P[2][0]) +
               P[0][2] * ((double)P[1][0] * P[2][1] - (double)P[1][1] * P[2][0]);
    float I[3][3] = {};
    if (d != 0.) {
        d = 1. / d;
        I[0][0] = (float)(((double)P[1][1] * P[2][2] - (double)P[1][2] * P[2][1]) * d);
        I[0][1] = (float)(((double)P[0][2] * P[2][1] - (double)P[0][1] * P[2][2]) * d);
        I[0][2] = (float)(((double)P[0][1] * P[1][2] - (double)P[0][2] * P[1][1]) * d);
        I[1][0] = (float)(((double)P[1][2] * P[2][0] - (double)P[1][0] * P[2][2]) * d);
        I[1][1] = (float)(((double)P[0][0] * P[2][2] - (double)P[0][2] * P[2][0]) * d);
        I[1][2] = (float)(((double)P[0][2] * P[1][0] - (double)P[0][0] * P[1][2]) * d);
        I[2][0] = (float)(((double)P[1][0] * P[2][1] - (double)P[1][1] * P[2][0]) * d);
        I[2][1] = (float)(((double)P[0][1] * P[2][0] - (double)P[0][0] * P[2][1]) * d);
        I[2][2] = (float)(((double)P[0][0] * P[1][1] - (double)P[0][1] * P[1][0]) * d);
    }
    // gemm: double accumulation, k ascending from the first product, one rounding to float.
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 3; c++) {
            double s = (double)Pp[r][0] * I[0][c];
            s = s + (double)Pp[r][1] * I[1][c];
            s = s + (double)Pp[r][2] * I[2][c];
            t[r * 3 + c] = (float)s;
        }
}

// cvRound(float) as SSE2's cvtss2si: round half to even, INT_MIN for NaN and out-of-range values.
__device__ inline int cv_round(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)rintf(v);
}

// The point test of RANSAC.cpp:122-135: testB = transform * [x, y, 1] (the gemm rule above), both
// points to cv::Point, int32 wrap-around differences / squares / sum, float(sqrt(double(sum)))
// <= (float)thresh.  That last test is monotone in the sum, so the host folds it into smax, the
// largest sum it admits; a negative (wrapped) sum gives NaN in the reference: an outlier.
__device__ inline bool point_pass(const float t[6], float4 p, int smax) {
    const float bx = (float)(((double)t[0] * p.x + (double)t[1] * p.y) + (double)t[2]);
    const float by = (float)(((double)t[3] * p.x + (double)t[4] * p.y) + (double)t[5]);
    const uint32_t dx = (uint32_t)cv_round(bx) - (uint32_t)cv_round(p.z);
    const uint32_t dy = (uint32_t)cv_round(by) - (uint32_t)cv_round(p.w);
    const int32_t s = (int32_t)(dx * dx + dy * dy);
    return s >= 0 && s <= smax;
}

// The largest int32 sum s >= 0 with (float)std::sqrt((double)s) <= (float)thresh (RANSAC.cpp:17,133).
inline int sum_limit(int thresh) {
    const float T = (float)thresh;
    int64_t lo = 0, hi = INT_MAX;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if ((float)std::sqrt((double)mid) <= T) lo = mid;
        else hi = mid - 1;
    }
    return (int)lo;
}

inline bool args_ok(const char *fn, int iters, int type, int thresh, double min_ratio) {
    if (type < MICV_RANSAC_TRANSLATION || type > MICV_RANSAC_AFFINE) {
        set_error("%s: type %d is not TRANSLATION (1), SIMILARITY (2) or AFFINE (3)", fn, type);
        return false;
    }
    if (iters < 1) {
        set_error("%s: iters %d < 1", fn, iters);
        return false;
    }
    if (thresh < 0) {
        set_error("%s: negative threshold %d", fn, thresh);
        return false;
    }
    if (std::isnan(min_ratio)) {
        set_error("%s: min_ratio is NaN", fn);
        return false;
    }
    return true;
}

}  // namespace
}  // namespace micv
