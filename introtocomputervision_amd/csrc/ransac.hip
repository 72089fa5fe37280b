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

#include "ransac_device.hpp"

struct micv_ransac_rng {
    std::mt19937 eng;
};

namespace micv {
namespace {

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
#include "ransac_score_body.hpp"
}

__global__ __launch_bounds__(256) void ransac_finalize_kernel(const float4 *__restrict__ pts, const int *ctl,
                                                              const int32_t *__restrict__ samples, uint64_t seed,
                                                              int iters, int type, int smax, double min_ratio,
                                                              const int *__restrict__ counts, float *transforms,
                                                              uint8_t *mask, int64_t mask_len, int32_t *stats) {
#include "ransac_finalize_body.hpp"
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
