// ransac_pairs.hip -- micv_ransac_solve_pairs_dev: the solve of ransac.hip on a batch of pairs.  The pair is blockIdx.y of
// the gather and the score launch and blockIdx.x of finalize; points, control words and count rows are per pair, and the
// seed of pair p is splitmix64(seed + p).  The score and finalize bodies are the single solve's
// (ransac_score_body.hpp, ransac_finalize_body.hpp), unchanged.
#include <algorithm>

#include "ransac_device.hpp"

namespace micv {
namespace {

__global__ __launch_bounds__(256) void ransac_gather_pairs_kernel(const float *__restrict__ kp, int images, size_t image_floats,
                                                                  int64_t kcap, const int32_t *__restrict__ pairs,
                                                                  const int32_t *__restrict__ mqt,
                                                                  const int64_t *__restrict__ count, int64_t mcap,
                                                                  float4 *__restrict__ pts, int *ctl) {
    const size_t p = blockIdx.y;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    const bool valid = (unsigned)a < (unsigned)images && (unsigned)b < (unsigned)images;
    const int64_t c = count[p];
    const int n = !valid ? 0 : (int)(c < 0 ? 0 : (c < mcap ? c : mcap));
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    ctl += 4 * p;
    if (j == 0) {
        ctl[0] = n;
        ctl[1] = -1;
        if (!valid) ctl[2] = 1;
    }
    if (j >= n) return;
    pts += p * (size_t)mcap;
    mqt += p * (size_t)mcap * 2;
    const int32_t q = mqt[2 * (size_t)j], t = mqt[2 * (size_t)j + 1];
    if (q < 0 || q >= kcap || t < 0 || t >= kcap) {
        atomicOr(&ctl[2], 1);
        pts[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float *kpa = kp + a * image_floats, *kpb = kp + b * image_floats;
    pts[j] = make_float4(kpa[4 * (size_t)q], kpa[4 * (size_t)q + 1], kpb[4 * (size_t)t], kpb[4 * (size_t)t + 1]);
}

template <bool kLds>
__global__ __launch_bounds__(256) void ransac_score_pairs_kernel(const float4 *__restrict__ pts_all, int64_t mcap, int *ctl_all,
                                                                 uint64_t seed0, int iters, int type, int smax,
                                                                 double min_ratio, int *__restrict__ counts_all) {
    const size_t p = blockIdx.y;
    const float4 *pts = pts_all + p * (size_t)mcap;
    int *ctl = ctl_all + 4 * p, *counts = counts_all + p * (size_t)iters;
    const int32_t *samples = nullptr;
    const uint64_t seed = splitmix64(seed0 + p);
#include "ransac_score_body.hpp"
}

__global__ __launch_bounds__(256) void ransac_finalize_pairs_kernel(const float4 *__restrict__ pts_all, int64_t mcap,
                                                                    const int *ctl_all, uint64_t seed0, int iters, int type,
                                                                    int smax, double min_ratio,
                                                                    const int *__restrict__ counts_all, float *transforms_all,
                                                                    uint8_t *mask_all, int32_t *stats_all) {
    const size_t p = blockIdx.x;
    const float4 *pts = pts_all + p * (size_t)mcap;
    const int *ctl = ctl_all + 4 * p, *counts = counts_all + p * (size_t)iters;
    const int32_t *samples = nullptr;
    const uint64_t seed = splitmix64(seed0 + p);
    float *transforms = transforms_all + 12 * p;
    uint8_t *mask = mask_all + p * (size_t)mcap;
    int32_t *stats = stats_all + 3 * p;
    const int64_t mask_len = mcap;
#include "ransac_finalize_body.hpp"
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_ransac_solve_pairs_dev(micv_ctx *ctx, const float *kp_xysa, int images, size_t kimage_stride, int64_t kcap,
                                const int32_t *pairs, int npairs, const int32_t *matches_qt, const int64_t *match_count,
                                int64_t mcap, uint64_t seed, int iters, int type, int thresh, double min_ratio,
                                float *transforms, uint8_t *inlier_mask, int32_t *stats, micv_stream stream) {
    MICV_REQUIRE(ctx && kp_xysa && pairs && matches_qt && match_count && transforms && inlier_mask && stats,
                 "micv_ransac_solve_pairs_dev: null argument");
    if (!args_ok("micv_ransac_solve_pairs_dev", iters, type, thresh, min_ratio)) return MICV_EINVAL;
    MICV_REQUIRE(mcap >= 1 && mcap <= (int64_t)1 << 30 && kcap >= 0,
                 "micv_ransac_solve_pairs_dev: mcap %lld outside 1 .. 2^30, or a negative keypoint capacity", (long long)mcap);
    MICV_REQUIRE(images >= 1 && npairs >= 1 && npairs <= 65535,
                 "micv_ransac_solve_pairs_dev: images %d < 1 or npairs %d outside 1 .. 65535", images, npairs);
    MICV_REQUIRE(kimage_stride % 4 == 0 && kimage_stride >= (size_t)kcap * 16,
                 "micv_ransac_solve_pairs_dev: kimage_stride %zu is no multiple of 4 or below kcap rows", kimage_stride);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t np = (size_t)npairs;
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need(np * (size_t)mcap, 16) + Carver::need(4 * np, 4) + Carver::need(np * (size_t)iters, 4), &scratch));
    Carver c(scratch);
    float4 *pts = c.take<float4>(np * (size_t)mcap);
    int *ctl = c.take<int>(4 * np);
    int *counts = c.take<int>(np * (size_t)iters);
    MICV_HIP(hipMemsetAsync(ctl, 0, 16 * np, s));
    ransac_gather_pairs_kernel<<<dim3((unsigned)cdiv((unsigned)mcap, 256), npairs), 256, 0, s>>>(
        kp_xysa, images, kimage_stride / 4, kcap, pairs, matches_qt, match_count, mcap, pts, ctl);
    MICV_LAUNCH_CHECK();
    const int smax = sum_limit(thresh);
    if (min_ratio > 0.0) {
        // the chunk workgroups of one pair: the single call's bound shared among the pairs (any grid gives the same bytes)
        const int64_t chunks = ((int64_t)iters + kChunk - 1) / kChunk;
        const int64_t share = std::max<int64_t>(1, (int64_t)ctx->wave_slots(2) / kWaves / npairs);
        const dim3 grid((unsigned)std::min<int64_t>(chunks, share), npairs);
        if (mcap <= kLdsMax)
            ransac_score_pairs_kernel<true><<<grid, 64 * kWaves, (size_t)mcap * 16, s>>>(pts, mcap, ctl, seed, iters, type, smax,
                                                                                         min_ratio, counts);
        else
            ransac_score_pairs_kernel<false><<<grid, 64 * kWaves, 0, s>>>(pts, mcap, ctl, seed, iters, type, smax, min_ratio, counts);
        MICV_LAUNCH_CHECK();
    }
    ransac_finalize_pairs_kernel<<<npairs, 256, 0, s>>>(pts, mcap, ctl, seed, iters, type, smax, min_ratio, counts, transforms,
                                                        inlier_mask, stats);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // extern "C"
