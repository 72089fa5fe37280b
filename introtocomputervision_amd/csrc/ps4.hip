// ps4.hip -- what the ps4 driver (ProblemSets/ps4_cpp/src/Solution.cpp) writes out between the library's calls:
//   * drawDots (:59-69): the grey image as 8-bit BGR, red where the normalised corner map is non-zero;
//   * cv::hconcat (:86, :161, :191, :241);
//   * cv::drawKeypoints(.., Scalar::all(-1), DRAW_RICH_KEYPOINTS) (:147-158) on a column window of the seam canvas;
//   * the match lines coloured from cv::RNG(12345) (:190-207) and the consensus lines (:240-250);
//   * harrisHelper's three pictures and siftHelper's / ransacHelper's panels as one call each.
// The contract is shim/micv_ps4.hpp and DESIGN.md sections 2 and 3 (OpenCV's drawing restated, PARITY UNPINNED).
// Nothing here synchronises the host or reads a count on the host.
//
// Every glyph and every line has a colour of its own and later strokes overwrite earlier ones, so the order of the
// serial painter is part of the result.  It is reproduced with an owner plane: a u32 per pixel, zero = nobody; the claim
// pass gives a wave to a stroke and a lane to a step of its walk and stores priority + 1 with an atomic max; the resolve
// pass paints every owned pixel with its owner's colour.  The highest priority owns the pixel, which is what the last
// writer of the serial loop leaves.  The colours are the words of a multiply-with-carry generator, which is serial: one
// lane walks them into a table before the claim pass, 3 n steps for the n strokes the DEVICE count names.
#include <algorithm>
#include <cmath>

#include "draw.hpp"
#include "kernels.hpp"
#include "pixmap.hpp"
#include "sincos_deg.hpp"

namespace micv {
namespace {

constexpr int kWave = 64;
constexpr unsigned kMaxStrokeWaves = 2048;  // waves of a claim launch; each strides over the strokes

__device__ __forceinline__ uint32_t rng_next(uint64_t &s) {  // cv::RNG::next (cv_rng.hpp)
    s = (uint64_t)(uint32_t)s * 4164903690u + (s >> 32);
    return (uint32_t)s;
}
// Scalar(rng(m), rng(m), rng(m)): the arguments are evaluated right to left, so the first draw is byte 2
__device__ __forceinline__ uint32_t rng_colour(uint64_t &s, uint32_t m) {
    const uint32_t b2 = rng_next(s) % m, b1 = rng_next(s) % m, b0 = rng_next(s) % m;
    return b0 | b1 << 8 | b2 << 16;
}
__device__ __forceinline__ int64_t clamp_count(const int64_t *count, int64_t cap) {
    const int64_t c = count ? *count : 0;
    return c < 0 ? 0 : (c < cap ? c : cap);
}
// cvRound of a coordinate: half to even; values that are not finite or beyond 1e9 draw nothing.  1e9 < 2^30 =
// 1 073 741 824, and a glyph's stroke ends within 32767 + 1 of its centre: inside the bound of draw.hpp's narrow walk.
__device__ __forceinline__ bool coord_ok(float v) { return fabsf(v) < 1e9f; }  // (false for NaN and inf)

__device__ __forceinline__ void claim(unsigned *owner, int rows, int cols, long long x, long long y, unsigned tag) {
    if (x >= 0 && x < cols && y >= 0 && y < rows) atomicMax(owner + (size_t)y * cols + (size_t)x, tag);
}

// The in-image steps of micv_viz::line(p1, p2) (draw.hpp), dealt out to the wave's lanes; every pixel claims its owner word.
__device__ __forceinline__ void claim_stroke(unsigned *owner, int rows, int cols, long long x1, long long y1, long long x2,
                                             long long y2, unsigned tag) {
    const draw::LineWalk w = draw::line_walk(rows, cols, x1, y1, x2, y2);
    draw::walk_steps(w, threadIdx.x & (kWave - 1), kWave, draw::narrow_minor(w),
                     [&](long long x, long long y) { claim(owner, rows, cols, x, y, tag); });
}

// ---- keypoint glyphs ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void glyph_colours_kernel(const int64_t *__restrict__ count, int64_t cap,
                                                               uint64_t *__restrict__ state, uint32_t *__restrict__ table) {
    if (threadIdx.x != 0) return;
    const int64_t n = clamp_count(count, cap);
    uint64_t s = *state;
    if (s == 0) s = 0xffffffffull;  // cv::theRNG()'s start
    for (int64_t j = 0; j < n; j++) table[j] = rng_colour(s, 256u);
    *state = s;
}

// blockIdx.x strides over the glyphs; coordinates are those of the window (the image the keypoints were found in).
__global__ __launch_bounds__(kWave) void glyph_claim_kernel(unsigned *__restrict__ owner, int rows, int cols,
                                                             const float *__restrict__ kp, const int64_t *__restrict__ count,
                                                             int64_t cap) {
    const int64_t n = clamp_count(count, cap);
    const int lane = threadIdx.x;
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        const float x = kp[4 * j], y = kp[4 * j + 1], size = kp[4 * j + 2], angle = kp[4 * j + 3];
        const float half = size * 0.5f;
        if (!coord_ok(x) || !coord_ok(y) || !(half >= 0.f && half <= 32767.f)) continue;
        const long long cx = (long long)rintf(x), cy = (long long)rintf(y), radius = (long long)rintf(half);
        const unsigned tag = (unsigned)j + 1u;
        // the circle (draw.hpp): the eight points of a step go to lanes 0..7, which walk the octant together
        if (lane < 8 && draw::circle_reaches(cx, cy, radius, rows, cols)) {
            const bool swap = lane & 4;
            const long long sa = (lane & 1) ? -1 : 1, sb = (lane & 2) ? -1 : 1;
            draw::circle_walk(radius, [&](long long dx, long long dy) {
                claim(owner, rows, cols, cx + sa * (swap ? dy : dx), cy + sb * (swap ? dx : dy), tag);
            });
        }
        if (angle != -1.f && fabsf(angle) < 1e9f) {  // the orientation stroke
            float s, c;
            sincos_deg(angle, s, c);
            const long long ex = cx + (long long)rintf(c * (float)radius), ey = cy + (long long)rintf(s * (float)radius);
            claim_stroke(owner, rows, cols, cx, cy, ex, ey, tag);
        }
    }
}

// The panel: the owner's colour, or the source pixel as pixmap.hpp copies it (src NULL: what the canvas holds).
__global__ __launch_bounds__(256) void glyph_resolve_kernel(const uint8_t *__restrict__ src, int channels, size_t sstride, int rows,
                                                             int cols, const unsigned *__restrict__ owner,
                                                             const uint32_t *__restrict__ table, uint8_t *__restrict__ dst,
                                                             size_t dstride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const draw::Target panel{dst, dstride, rows, cols, 3};
    const unsigned o = owner[(size_t)y * cols + x];
    if (o) {
        draw::put(panel, x, y, table[o - 1]);
    } else if (src) {
        const uint8_t *s = src + (size_t)y * sstride;
        draw::put(panel, x, y, channels == 3 ? draw::read_bgr<uint8_t, 3>(s, x) : draw::read_bgr<uint8_t, 1>(s, x));
    }
}

// ---- match lines --------------------------------------------------------------------------------------------------
// One wave.  Match i < n is DRAWN when the mask (if any) marks it and both of its indices name a keypoint; its rank is
// the number of drawn matches before it: a ballot per chunk of 64, the bits below the lane counted, the chunk's total
// carried into the next.  Then lane 0 walks the colours of the drawn lines.
__global__ __launch_bounds__(kWave) void line_ranks_kernel(const int32_t *__restrict__ matches, const int64_t *__restrict__ count,
                                                            int64_t cap, const uint8_t *__restrict__ mask, int64_t na, int64_t nb,
                                                            uint64_t seed, int32_t *__restrict__ rank, uint32_t *__restrict__ table) {
    const int64_t n = clamp_count(count, cap);
    const int lane = threadIdx.x;
    int64_t base = 0;
    for (int64_t c0 = 0; c0 < n; c0 += kWave) {
        const int64_t i = c0 + lane;
        bool drawn = false;
        if (i < n) {
            const int64_t q = matches[2 * i], t = matches[2 * i + 1];
            drawn = (!mask || mask[i]) && q >= 0 && q < na && t >= 0 && t < nb;
        }
        const unsigned long long votes = __ballot(drawn);
        const int below = __popcll(votes & ((1ull << lane) - 1ull));
        if (i < n) rank[i] = drawn ? (int32_t)(base + below) : -1;
        base += __popcll(votes);
    }
    if (lane == 0) {
        uint64_t s = seed ? seed : 0xffffffffull;
        for (int64_t r = 0; r < base; r++) table[r] = rng_colour(s, 255u);  // rng.uniform(0, 255): next() % 255
    }
}

__global__ __launch_bounds__(kWave) void line_claim_kernel(unsigned *__restrict__ owner, int rows, int cols,
                                                            const float *__restrict__ kp_a, const float *__restrict__ kp_b,
                                                            const int32_t *__restrict__ matches, const int64_t *__restrict__ count,
                                                            int64_t cap, const int32_t *__restrict__ rank, float x_offset) {
    const int64_t n = clamp_count(count, cap);
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t r = rank[i];
        if (r < 0) continue;
        const float *a = kp_a + 4 * (int64_t)matches[2 * i], *b = kp_b + 4 * (int64_t)matches[2 * i + 1];
        const float x1 = a[0], y1 = a[1], x2 = b[0] + x_offset, y2 = b[1];  // (the sum in float, Solution.cpp:201)
        if (!coord_ok(x1) || !coord_ok(y1) || !coord_ok(x2) || !coord_ok(y2)) continue;
        claim_stroke(owner, rows, cols, (long long)rintf(x1), (long long)rintf(y1), (long long)rintf(x2), (long long)rintf(y2),
                     (unsigned)r + 1u);
    }
}

// ---- dots, hconcat ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dots_kernel(const T *__restrict__ gray, size_t gstride, const uint8_t *__restrict__ mask,
                                                    size_t mstride, int rows, int cols, uint8_t *__restrict__ dst, size_t dstride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const T *row = reinterpret_cast<const T *>(reinterpret_cast<const char *>(gray) + (size_t)y * gstride);
    const bool dot = mask[(size_t)y * mstride + x] != 0;
    draw::put(draw::Target{dst, dstride, rows, cols, 3}, x, y, dot ? 0xFF0000u : draw::read_bgr<T, 1>(row, x));
}

// x counts BYTES of the destination row
__global__ __launch_bounds__(256) void hconcat_kernel(const uint8_t *__restrict__ a, size_t astride, int abytes,
                                                       const uint8_t *__restrict__ b, size_t bstride, int bbytes, int rows,
                                                       uint8_t *__restrict__ dst, size_t dstride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= abytes + bbytes || y >= rows) return;
    dst[(size_t)y * dstride + x] = x < abytes ? a[(size_t)y * astride + x] : b[(size_t)y * bstride + (x - abytes)];
}

constexpr int kMaxSide = 32767;
constexpr int64_t kMaxStrokes = (int64_t)1 << 24;  // per call: the owner word holds priority + 1

unsigned stroke_waves(int64_t cap) { return (unsigned)std::min<int64_t>(std::max<int64_t>(cap, 1), kMaxStrokeWaves); }

int dots_from_mask(hipStream_t s, const void *gray, int depth, size_t gstride, const uint8_t *mask, size_t mstride, int rows,
                   int cols, uint8_t *dst, size_t dstride) {
    const dim3 grid(cdiv(cols, 64), cdiv(rows, 4));
    if (depth == MICV_DEPTH_32F)
        dots_kernel<float><<<grid, 256, 0, s>>>(static_cast<const float *>(gray), gstride, mask, mstride, rows, cols, dst, dstride);
    else
        dots_kernel<uint8_t><<<grid, 256, 0, s>>>(static_cast<const uint8_t *>(gray), gstride, mask, mstride, rows, cols, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_draw_dots_dev(micv_ctx *ctx, const void *gray, int depth, int rows, int cols, size_t gstride, const float *corners,
                       size_t cstride, uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && gray && corners && dst, "micv_draw_dots: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_draw_dots: depth %d not supported (8U, 32F)", depth);
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide) && stride_ok(gstride, cols, depth == MICV_DEPTH_32F ? 4 : 1) && stride_ok(cstride, cols, 4) &&
                     dstride >= (size_t)cols * 3,
                 "micv_draw_dots: bad size %dx%d (1..32767) or stride", rows, cols);
    MICV_REQUIRE(gray != dst && static_cast<const void *>(corners) != dst, "micv_draw_dots: dst aliases an input");
    MICV_HIP(hipSetDevice(ctx->device));
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need((size_t)rows * cols, 1), &scratch));
    uint8_t *mask = static_cast<uint8_t *>(scratch);
    // cv::normalize(mask, maskNorm, 0, 255, NORM_MINMAX, CV_8U), Solution.cpp:67: the range and the bytes of display.hip
    MICV_TRY(micv_normalize_minmax_dev(ctx, corners, MICV_DEPTH_32F, rows, cols, cstride, mask, (size_t)cols, nullptr, 0, nullptr, 0,
                                       nullptr, stream));
    return dots_from_mask(static_cast<hipStream_t>(stream), gray, depth, gstride, mask, (size_t)cols, rows, cols, dst, dstride);
}

int micv_hconcat_dev(micv_ctx *ctx, const uint8_t *a, size_t astride, int acols, const uint8_t *b, size_t bstride, int bcols,
                     int rows, int bpp, uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && a && b && dst, "micv_hconcat: null argument");
    MICV_REQUIRE(bpp == 1 || bpp == 3, "micv_hconcat: %d bytes per pixel not supported (1 or 3)", bpp);
    MICV_REQUIRE(draw::size_ok(rows, acols, kMaxSide) && draw::size_ok(rows, bcols, kMaxSide), "micv_hconcat: bad size %d x (%d + %d) (1..32767)", rows, acols, bcols);
    MICV_REQUIRE(astride >= (size_t)acols * bpp && bstride >= (size_t)bcols * bpp && dstride >= ((size_t)acols + bcols) * bpp,
                 "micv_hconcat: a stride is smaller than its row");
    MICV_REQUIRE(a != dst && b != dst, "micv_hconcat: dst aliases an input");
    MICV_HIP(hipSetDevice(ctx->device));
    hconcat_kernel<<<dim3(cdiv((unsigned)(acols + bcols) * bpp, 64), cdiv(rows, 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        a, astride, acols * bpp, b, bstride, bcols * bpp, rows, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_draw_keypoints_dev(micv_ctx *ctx, const uint8_t *src, int channels, int rows, int cols, size_t sstride, uint8_t *canvas,
                            int canvas_cols, size_t cstride, int x0, const float *kp_xysa, const int64_t *count, int64_t cap,
                            uint64_t *rng_state, micv_stream stream) {
    MICV_REQUIRE(ctx && canvas && rng_state, "micv_draw_keypoints: null argument");
    MICV_REQUIRE(cap >= 0 && cap <= kMaxStrokes && (cap == 0 || (kp_xysa && count)),
                 "micv_draw_keypoints: cap %lld out of 0..2^24, or keypoints / count missing", (long long)cap);
    MICV_REQUIRE(!src || channels == 1 || channels == 3, "micv_draw_keypoints: %d channels not supported (1 or 3)", channels);
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide) && (!src || sstride >= (size_t)cols * channels), "micv_draw_keypoints: bad size %dx%d or stride",
                 rows, cols);
    MICV_REQUIRE(x0 >= 0 && canvas_cols <= 65534 && (int64_t)x0 + cols <= canvas_cols && cstride >= (size_t)canvas_cols * 3 &&
                     cstride < (size_t)1 << 32,
                 "micv_draw_keypoints: the window [%d, %d + %d) does not lie in a canvas of %d columns, or bad stride", x0, x0, cols,
                 canvas_cols);
    MICV_REQUIRE(src != canvas, "micv_draw_keypoints: src aliases the canvas (NULL draws on what the canvas holds)");
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *panel = canvas + 3 * (size_t)x0;
    const dim3 grid(cdiv(cols, 64), cdiv(rows, 4));
    if (cap == 0)  // the copy alone
        return src ? launch_to_bgr8(s, src, MICV_DEPTH_8U, channels, sstride, rows, cols, panel, cstride) : MICV_OK;
    const size_t npix = (size_t)rows * cols;
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need(npix, 4) + Carver::need((size_t)cap, 4), &scratch));
    Carver carve(scratch);
    unsigned *owner = carve.take<unsigned>(npix);
    uint32_t *table = carve.take<uint32_t>((size_t)cap);
    MICV_HIP(hipMemsetAsync(owner, 0, npix * 4, s));
    glyph_colours_kernel<<<1, kWave, 0, s>>>(count, cap, rng_state, table);
    MICV_LAUNCH_CHECK();
    glyph_claim_kernel<<<stroke_waves(cap), kWave, 0, s>>>(owner, rows, cols, kp_xysa, count, cap);
    MICV_LAUNCH_CHECK();
    glyph_resolve_kernel<<<grid, 256, 0, s>>>(src, channels, sstride, rows, cols, owner, table, panel, cstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_draw_match_lines_dev(micv_ctx *ctx, uint8_t *canvas, int rows, int cols, size_t stride, const float *kp_a, int64_t na,
                              const float *kp_b, int64_t nb, const int32_t *matches_qt, const int64_t *count, int64_t cap,
                              const uint8_t *mask, int x_offset, uint64_t seed, micv_stream stream) {
    MICV_REQUIRE(ctx && canvas, "micv_draw_match_lines: null argument");
    MICV_REQUIRE(cap >= 0 && cap <= kMaxStrokes && na >= 0 && nb >= 0, "micv_draw_match_lines: cap %lld out of 0..2^24, or a negative size",
                 (long long)cap);
    MICV_REQUIRE(rows > 0 && cols > 0 && rows <= 32767 && cols <= 65534 && stride >= (size_t)cols * 3 && stride < (size_t)1 << 32,
                 "micv_draw_match_lines: bad size %dx%d or stride", rows, cols);
    if (cap == 0 || na == 0 || nb == 0) return MICV_OK;  // nothing can be drawn
    MICV_REQUIRE(kp_a && kp_b && matches_qt && count, "micv_draw_match_lines: null argument");
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t npix = (size_t)rows * cols;
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need(npix, 4) + 2 * Carver::need((size_t)cap, 4), &scratch));
    Carver carve(scratch);
    unsigned *owner = carve.take<unsigned>(npix);
    uint32_t *table = carve.take<uint32_t>((size_t)cap);
    int32_t *rank = carve.take<int32_t>((size_t)cap);
    MICV_HIP(hipMemsetAsync(owner, 0, npix * 4, s));
    line_ranks_kernel<<<1, kWave, 0, s>>>(matches_qt, count, cap, mask, na, nb, seed, rank, table);
    MICV_LAUNCH_CHECK();
    line_claim_kernel<<<stroke_waves(cap), kWave, 0, s>>>(owner, rows, cols, kp_a, kp_b, matches_qt, count, cap, rank, (float)x_offset);
    MICV_LAUNCH_CHECK();
    glyph_resolve_kernel<<<dim3(cdiv(cols, 64), cdiv(rows, 4)), 256, 0, s>>>(nullptr, 3, 0, rows, cols, owner, table, canvas, stride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_ps4_harris_display_dev(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                                double sigma, float alpha, int flags, double threshold, int min_distance, float *fields,
                                int32_t *locs_yx, int64_t cap, int64_t *count, uint8_t *grad_panel, size_t gstride,
                                uint8_t *resp_u8, size_t rstride, uint8_t *dots, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && img && fields && grad_panel && resp_u8 && dots, "micv_ps4_harris_display: null argument");
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide) && stride_ok(stride, cols, 4) && gstride >= (size_t)2 * cols && gstride < (size_t)1 << 32 &&
                     rstride >= (size_t)cols && dstride >= (size_t)cols * 3,
                 "micv_ps4_harris_display: bad size %dx%d or stride", rows, cols);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)rows * cols, rb = (size_t)cols * 4;
    float *gx = fields, *gy = fields + n, *resp = fields + 2 * n, *corners = fields + 3 * n;
    MICV_TRY(micv_harris_corners_dev(ctx, img, rows, cols, stride, sobel_ksize, win, sigma, alpha, flags, threshold, min_distance, gx,
                                     gy, rb, resp, rb, corners, rb, locs_yx, cap, count, stream));
    void *pool;
    MICV_TRY(ctx->reserve_chain(Carver::need(4 * n, 1), &pool));
    uint8_t *norm = static_cast<uint8_t *>(pool);
    // the four ranges in one min-max launch, the four images in one apply launch
    MICV_TRY(micv_normalize_minmax_batch_dev(ctx, fields, n * 4, MICV_DEPTH_32F, 4, rows, cols, rb, norm, n, (size_t)cols, nullptr, 0, 0,
                                             nullptr, 0, 0, nullptr, stream));
    MICV_TRY(micv_hconcat_dev(ctx, norm, (size_t)cols, cols, norm + n, (size_t)cols, cols, rows, 1, grad_panel, gstride, stream));
    MICV_HIP(hipMemcpy2DAsync(resp_u8, rstride, norm + 2 * n, (size_t)cols, (size_t)cols, rows, hipMemcpyDeviceToDevice, s));
    return dots_from_mask(s, img, MICV_DEPTH_32F, stride, norm + 3 * n, (size_t)cols, rows, cols, dots, dstride);
}

int micv_ps4_match_panels_dev(micv_ctx *ctx, const uint8_t *img_a, size_t astride, int cols_a, const uint8_t *img_b, size_t bstride,
                              int cols_b, int rows, const float *kp_a, const int64_t *count_a, int64_t cap_a, const float *kp_b,
                              const int64_t *count_b, int64_t cap_b, const int32_t *matches_qt, const int64_t *match_count,
                              int64_t match_cap, const uint8_t *mask, int flags, uint64_t seed, uint64_t *rng_state,
                              uint8_t *keypoint_panel, uint8_t *match_panel, size_t pstride, micv_stream stream) {
    MICV_REQUIRE(ctx && img_a && img_b && match_panel && rng_state, "micv_ps4_match_panels: null argument");
    MICV_REQUIRE((flags & ~MICV_PS4_NO_GLYPHS) == 0, "micv_ps4_match_panels: unknown flag in %d", flags);
    MICV_REQUIRE(draw::size_ok(rows, cols_a, kMaxSide) && draw::size_ok(rows, cols_b, kMaxSide) && astride >= (size_t)cols_a && bstride >= (size_t)cols_b,
                 "micv_ps4_match_panels: bad size %d x (%d + %d) or stride", rows, cols_a, cols_b);
    MICV_REQUIRE(keypoint_panel != match_panel, "micv_ps4_match_panels: the two panels alias");
    const bool glyphs = !(flags & MICV_PS4_NO_GLYPHS);
    const int cols = cols_a + cols_b;
    MICV_REQUIRE(pstride >= (size_t)cols * 3 && pstride < (size_t)1 << 32, "micv_ps4_match_panels: stride %zu does not hold %d columns",
                 pstride, cols);
    uint8_t *first = glyphs && keypoint_panel ? keypoint_panel : match_panel;
    MICV_TRY(micv_draw_keypoints_dev(ctx, img_a, 1, rows, cols_a, astride, first, cols, pstride, 0, kp_a, count_a, glyphs ? cap_a : 0,
                                     rng_state, stream));
    MICV_TRY(micv_draw_keypoints_dev(ctx, img_b, 1, rows, cols_b, bstride, first, cols, pstride, cols_a, kp_b, count_b,
                                     glyphs ? cap_b : 0, rng_state, stream));
    if (first != match_panel)
        MICV_HIP(hipMemcpy2DAsync(match_panel, pstride, first, pstride, (size_t)cols * 3, rows, hipMemcpyDeviceToDevice,
                                  static_cast<hipStream_t>(stream)));
    return micv_draw_match_lines_dev(ctx, match_panel, rows, cols, pstride, kp_a, cap_a, kp_b, cap_b, matches_qt, match_count, match_cap,
                                     mask, cols_a, seed, stream);
}

}  // extern "C"
