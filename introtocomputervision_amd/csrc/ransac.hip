// ransac.hip -- ransac::solve (ps4_cpp/lib/RANSAC.cpp:27-152) on the device, and the reference's
// host-side sampler (RANSAC.cpp:11-13,20-25,53).
//
// One wave scores one hypothesis: every lane builds the same transform in registers from the k
// sample points, the lanes stride over the matches, and a ballot + popcount per 64 matches counts
// the inliers (the sample indices excluded).  Matches are staged once per workgroup in LDS as
// float4 (src x, y, dst x, y) while they fit (kLdsMax = 4096 matches = 64 KiB, two workgroups per
// CU); larger sets stream from global memory.  Hypotheses run in chunks of kChunk per workgroup; a
// chunk starting after a stop iteration already found is skipped -- every iteration up to the
// first stop is always scored, so the result does not depend on the skipping.  A one-workgroup
// finalize kernel then finds the stop iteration and the first argmax and writes every output.
//
// Arithmetic: DESIGN.md section 2 ("RANSAC").  -ffp-contract=off: no fma anywhere here.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <numeric>
#include <random>
#include <vector>

#include "common.hpp"

struct micv_ransac_rng {
    std::mt19937 eng;
};

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

__global__ __launch_bounds__(256) void ransac_pack_kernel(const float *__restrict__ src, const float *__restrict__ dst,
                                                          int n, float4 *__restrict__ pts, int *ctl) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) {
        ctl[0] = n;
        ctl[1] = -1;
    }
    if (j < n) pts[j] = make_float4(src[2 * (size_t)j], src[2 * (size_t)j + 1], dst[2 * (size_t)j], dst[2 * (size_t)j + 1]);
}

// Solution.cpp:222-225: src = kp_a[queryIdx].pt, dst = kp_b[trainIdx].pt, n = min(*count, cap).
__global__ __launch_bounds__(256) void ransac_gather_kernel(const float *__restrict__ kpa, int64_t na,
                                                            const float *__restrict__ kpb, int64_t nb,
                                                            const int32_t *__restrict__ mqt, const int64_t *count,
                                                            int64_t cap, float4 *__restrict__ pts, int *ctl) {
    const int64_t c = *count;
    const int n = (int)(c < 0 ? 0 : (c < cap ? c : cap));
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) {
        ctl[0] = n;
        ctl[1] = -1;
    }
    if (j >= n) return;
    const int32_t q = mqt[2 * (size_t)j], t = mqt[2 * (size_t)j + 1];
    if (q < 0 || q >= na || t < 0 || t >= nb) {
        atomicOr(&ctl[2], 1);
        pts[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    pts[j] = make_float4(kpa[4 * (size_t)q], kpa[4 * (size_t)q + 1], kpb[4 * (size_t)t], kpb[4 * (size_t)t + 1]);
}

template <bool kLds>
__global__ __launch_bounds__(256) void ransac_score_kernel(const float4 *__restrict__ pts, int *ctl,
                                                           const int32_t *__restrict__ samples, uint64_t seed,
                                                           int iters, int type, int smax, double min_ratio,
                                                           int *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = ctl[0];
    const int k = type;
    if (n < k || ctl[2]) return;
    const float4 *P = pts;
    if (kLds) {
        float4 *lp = reinterpret_cast<float4 *>(smem);
        for (int j = threadIdx.x; j < n; j += blockDim.x) lp[j] = pts[j];
        __syncthreads();
        P = lp;
    }
    unsigned *stop = reinterpret_cast<unsigned *>(&ctl[1]);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t h0 = (int64_t)blockIdx.x * kChunk; h0 < iters; h0 += (int64_t)gridDim.x * kChunk) {
        // chunks ascend: once one starts after a known stop, so does every later one
        if ((uint64_t)h0 > __hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        const int hend = (int)std::min<int64_t>(h0 + kChunk, iters);
        for (int h = (int)h0 + wave; h < hend; h += kWaves) {
            int s[3];
            if (!draw_sample(samples, seed, h, k, n, s)) {
                if (lane == 0) {
                    atomicOr(&ctl[2], 1);
                    counts[h] = 0;
                }
                continue;
            }
            float4 q[3];
            for (int e = 0; e < 3; e++) q[e] = e < k ? P[s[e]] : make_float4(0.f, 0.f, 0.f, 0.f);
            float t[6];
            hypothesis(type, q, t);
            int cnt = 0;
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int j = j0 + lane;
                const bool in = j < n && j != s[0] && j != s[1] && j != s[2] && point_pass(t, P[j], smax);
                cnt += __popcll(__ballot(in));
            }
            if (lane == 0) {
                counts[h] = cnt;
                if ((double)cnt / (double)n >= min_ratio) atomicMin(stop, (unsigned)h);
            }
        }
    }
}

__global__ __launch_bounds__(256) void ransac_finalize_kernel(const float4 *__restrict__ pts, const int *ctl,
                                                              const int32_t *__restrict__ samples, uint64_t seed,
                                                              int iters, int type, int smax, double min_ratio,
                                                              const int *__restrict__ counts, float *transforms,
                                                              uint8_t *mask, int64_t mask_len, int32_t *stats) {
    __shared__ unsigned first;
    __shared__ unsigned long long best_key;
    __shared__ float tb[6];
    __shared__ int sb[3];
    __shared__ int ran;  // 1: iterations ran, 0: none, -1: bad input
    const int n = ctl[0];
    const int k = type;
    if (threadIdx.x == 0) {
        first = ~0u;
        best_key = 0;
        ran = ctl[2] ? -1 : (n < k || 0.0 >= min_ratio) ? 0 : 1;
    }
    __syncthreads();
    if (ran != 1) {
        if (threadIdx.x == 0) {
            stats[0] = ran;
            stats[1] = -1;
            stats[2] = 0;
        }
        if (threadIdx.x < 12) transforms[threadIdx.x] = 0.f;
        for (int64_t j = threadIdx.x; j < mask_len; j += blockDim.x) mask[j] = 0;
        return;
    }
    // the stop iteration: the first i with count_i / n >= min_ratio.  Every i up to the stop word
    // was scored (and no i beyond it is read).
    const unsigned sw = (unsigned)ctl[1];
    const int bound = sw < (unsigned)iters ? (int)sw : iters - 1;
    unsigned f = ~0u;
    for (int i = threadIdx.x; i <= bound; i += blockDim.x)
        if ((double)counts[i] / (double)n >= min_ratio) {
            f = (unsigned)i;
            break;
        }
    atomicMin(&first, f);
    __syncthreads();
    const int last = first != ~0u ? (int)first : iters - 1;
    // the first maximum over [0, last]: the reference's strict '>' update
    unsigned long long key = 0;
    for (int i = threadIdx.x; i <= last; i += blockDim.x) {
        const unsigned long long kk = ((unsigned long long)(unsigned)counts[i] << 32) | (0xFFFFFFFFu - (unsigned)i);
        key = kk > key ? kk : key;
    }
    atomicMax(&best_key, key);
    __syncthreads();
    const int best = (int)(0xFFFFFFFFu - (unsigned)(best_key & 0xFFFFFFFFu));
    if (threadIdx.x == 0) {
        int s[3];
        float4 q[3];
        float t[6];
        draw_sample(samples, seed, last, k, n, s);
        for (int e = 0; e < 3; e++) q[e] = e < k ? pts[s[e]] : make_float4(0.f, 0.f, 0.f, 0.f);
        hypothesis(type, q, t);
        for (int e = 0; e < 6; e++) transforms[e] = t[e];
        draw_sample(samples, seed, best, k, n, s);
        for (int e = 0; e < 3; e++) q[e] = e < k ? pts[s[e]] : make_float4(0.f, 0.f, 0.f, 0.f);
        hypothesis(type, q, t);
        for (int e = 0; e < 6; e++) {
            transforms[6 + e] = t[e];
            tb[e] = t[e];
        }
        for (int e = 0; e < 3; e++) sb[e] = s[e];
        stats[0] = last + 1;
        stats[1] = best;
        stats[2] = (int)(best_key >> 32);
    }
    __syncthreads();
    float t[6];
    for (int e = 0; e < 6; e++) t[e] = tb[e];
    for (int64_t j = threadIdx.x; j < mask_len; j += blockDim.x)
        mask[j] = j < n && j != sb[0] && j != sb[1] && j != sb[2] && point_pass(t, pts[j], smax);
}

// The largest int32 sum s >= 0 with (float)std::sqrt((double)s) <= (float)thresh (RANSAC.cpp:17,133).
int sum_limit(int thresh) {
    const float T = (float)thresh;
    int64_t lo = 0, hi = INT_MAX;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if ((float)std::sqrt((double)mid) <= T) lo = mid;
        else hi = mid - 1;
    }
    return (int)lo;
}

bool args_ok(const char *fn, int iters, int type, int thresh, double min_ratio) {
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

// Scratch, the score launch and the finalize launch; `bound` is a host-known upper bound of n.
int solve_enqueue(micv_ctx *ctx, hipStream_t s, int64_t bound, const int32_t *samples, uint64_t seed, int iters,
                  int type, int thresh, double min_ratio, float4 *pts, int *ctl, int *counts, float *transforms,
                  uint8_t *mask, int64_t mask_len, int32_t *stats) {
    const int smax = sum_limit(thresh);
    if (min_ratio > 0.0) {
        const int64_t chunks = ((int64_t)iters + kChunk - 1) / kChunk;
        const int grid = (int)std::min<int64_t>(chunks, (int64_t)ctx->wave_slots(2) / kWaves);
        if (bound <= kLdsMax)
            ransac_score_kernel<true><<<grid, 64 * kWaves, (size_t)bound * 16, s>>>(pts, ctl, samples, seed, iters,
                                                                                     type, smax, min_ratio, counts);
        else
            ransac_score_kernel<false><<<grid, 64 * kWaves, 0, s>>>(pts, ctl, samples, seed, iters, type, smax,
                                                                    min_ratio, counts);
        MICV_LAUNCH_CHECK();
    }
    ransac_finalize_kernel<<<1, 256, 0, s>>>(pts, ctl, samples, seed, iters, type, smax, min_ratio, counts, transforms,
                                             mask, mask_len, stats);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_ransac_rng_create(const uint32_t *seed_words, int nwords, micv_ransac_rng **out) {
    MICV_REQUIRE(out && nwords >= 0, "micv_ransac_rng_create: bad argument");
    micv_ransac_rng *r = new micv_ransac_rng;
    if (seed_words) {
        std::seed_seq seq(seed_words, seed_words + nwords);
        r->eng.seed(seq);
    }
    *out = r;
    return MICV_OK;
}

void micv_ransac_rng_destroy(micv_ransac_rng *rng) { delete rng; }

int micv_ransac_rng_samples(const micv_ransac_rng *rng, int64_t n, int k, int iters, int32_t *samples) {
    MICV_REQUIRE(rng && samples && n >= 1 && n <= (int64_t)1 << 30 && k >= 1 && k <= n && iters >= 0,
                 "micv_ransac_rng_samples: bad argument");
    std::mt19937 eng = rng->eng;
    std::vector<int> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    for (int i = 0; i < iters; i++) {
        std::shuffle(idx.begin(), idx.end(), eng);
        for (int j = 0; j < k; j++) samples[(size_t)i * k + j] = idx[j];
    }
    return MICV_OK;
}

int micv_ransac_rng_permutation(const micv_ransac_rng *rng, int64_t n, int iter, int32_t *perm) {
    MICV_REQUIRE(rng && perm && n >= 1 && n <= (int64_t)1 << 30 && iter >= 0,
                 "micv_ransac_rng_permutation: bad argument");
    std::mt19937 eng = rng->eng;
    std::vector<int> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    for (int i = 0; i <= iter; i++) std::shuffle(idx.begin(), idx.end(), eng);
    std::copy(idx.begin(), idx.end(), perm);
    return MICV_OK;
}

int micv_ransac_rng_advance(micv_ransac_rng *rng, int64_t n, int iterations) {
    MICV_REQUIRE(rng && n >= 1 && n <= (int64_t)1 << 30 && iterations >= 0, "micv_ransac_rng_advance: bad argument");
    std::vector<int> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    for (int i = 0; i < iterations; i++) std::shuffle(idx.begin(), idx.end(), rng->eng);
    return MICV_OK;
}

int micv_ransac_solve_dev(micv_ctx *ctx, const float *src_xy, const float *dst_xy, int64_t n,
                          const int32_t *samples, int iters, int type, int thresh, double min_ratio,
                          float *transforms, uint8_t *inlier_mask, int32_t *stats, micv_stream stream) {
    MICV_REQUIRE(ctx && src_xy && dst_xy && samples && transforms && inlier_mask && stats,
                 "micv_ransac_solve_dev: null argument");
    if (!args_ok("micv_ransac_solve_dev", iters, type, thresh, min_ratio)) return MICV_EINVAL;
    MICV_REQUIRE(n >= type && n <= (int64_t)1 << 30, "micv_ransac_solve_dev: n = %lld points, need %d .. 2^30",
                 (long long)n, type);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need((size_t)n, 16) + Carver::need(4, 4) + Carver::need((size_t)iters, 4), &scratch));
    Carver c(scratch);
    float4 *pts = c.take<float4>((size_t)n);
    int *ctl = c.take<int>(4);
    int *counts = c.take<int>((size_t)iters);
    MICV_HIP(hipMemsetAsync(ctl, 0, 16, s));
    ransac_pack_kernel<<<(unsigned)cdiv((unsigned)n, 256), 256, 0, s>>>(src_xy, dst_xy, (int)n, pts, ctl);
    MICV_LAUNCH_CHECK();
    return solve_enqueue(ctx, s, n, samples, 0, iters, type, thresh, min_ratio, pts, ctl, counts, transforms,
                         inlier_mask, n, stats);
}

int micv_ransac_solve_matches_dev(micv_ctx *ctx, const float *kp_a, int64_t na, const float *kp_b,
                                  int64_t nb, const int32_t *matches_qt, const int64_t *count,
                                  int64_t cap, uint64_t seed, int iters, int type, int thresh,
                                  double min_ratio, float *transforms, uint8_t *inlier_mask,
                                  int32_t *stats, micv_stream stream) {
    MICV_REQUIRE(ctx && kp_a && kp_b && matches_qt && count && transforms && inlier_mask && stats,
                 "micv_ransac_solve_matches_dev: null argument");
    if (!args_ok("micv_ransac_solve_matches_dev", iters, type, thresh, min_ratio)) return MICV_EINVAL;
    MICV_REQUIRE(cap >= 1 && cap <= (int64_t)1 << 30 && na >= 0 && nb >= 0,
                 "micv_ransac_solve_matches_dev: cap %lld outside 1 .. 2^30, or a negative keypoint count",
                 (long long)cap);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need((size_t)cap, 16) + Carver::need(4, 4) + Carver::need((size_t)iters, 4),
                          &scratch));
    Carver c(scratch);
    float4 *pts = c.take<float4>((size_t)cap);
    int *ctl = c.take<int>(4);
    int *counts = c.take<int>((size_t)iters);
    MICV_HIP(hipMemsetAsync(ctl, 0, 16, s));
    ransac_gather_kernel<<<(unsigned)cdiv((unsigned)cap, 256), 256, 0, s>>>(kp_a, na, kp_b, nb, matches_qt, count,
                                                                           cap, pts, ctl);
    MICV_LAUNCH_CHECK();
    return solve_enqueue(ctx, s, cap, nullptr, seed, iters, type, thresh, min_ratio, pts, ctl, counts, transforms,
                         inlier_mask, cap, stats);
}

}  // extern "C"
