// ps5.hip -- what the ps5 driver (ProblemSets/ps5_cpp/src/Solution.cpp) does around lk:: and pyr:::
//   * drawVelocityVectors (:13-37) on the flow fields where they lie, with the prevImg.clone() + GRAY2RGB step in front;
//   * savePyramid (:86-99): four levels, each normalised by its own range, scaled back with INTER_NEAREST, tiled 2 x 2;
//   * warpHelper (:101-128): per consecutive pair naive LK -> lk::warp -> prev - warped -> cv::normalize;
//   * denseLKWrapper (:40-84) as one call: grey conversion, flow, arrows, the JET maps of u and v.
// The contract of the drawing and of the montage is shim/micv_viz.hpp (drawVelocityVectors, arrowed_line, line,
// savePyramid, resize_nearest, normalize_minmax_u8), which restates OpenCV 3.4, PARITY UNPINNED.
// Nothing here synchronises the host.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "draw.hpp"
#include "kernels.hpp"
#include "lk_device.hpp"
#include "minmax_keys.hpp"
#include "pixmap.hpp"

namespace micv {
namespace {

// ---- drawVelocityVectors.  blockIdx.x = the arrow (lattice point), blockIdx.y = the image of the batch; the wave walks
// the arrow's three strokes one after the other, a lane is one step along a stroke's major axis, and only the steps whose
// major coordinate lies inside the image are dealt out: an arrow of 10^6 pixels costs what its in-image part costs.
// Every stroke of every arrow stores the same colour, so pixels that several strokes or arrows share need no ordering.
constexpr int kArrowThreads = 64;

struct ArrowArgs {
    uint8_t *img;
    size_t img_pitch, stride;  // bytes
    const float *u, *v;
    size_t field_pitch, fstride;  // bytes
    int rows, cols, row_step, col_step, nx;
    uint32_t colour;  // B, G, R in bits 0, 8, 16
};

// micv_viz::line(p1, p2): the in-image steps of the walk (draw.hpp), dealt out to the wave's lanes.  Every coordinate is
// below 1e6 + cols + a tip of a tenth of the shaft, far inside the narrow walk's bound.
__device__ __forceinline__ void stroke(const draw::Target &t, long long x1, long long y1, long long x2, long long y2, uint32_t colour) {
    const draw::LineWalk w = draw::line_walk(t.rows, t.cols, x1, y1, x2, y2);
    draw::walk_steps(w, threadIdx.x, kArrowThreads, draw::narrow_minor(w), [&](long long x, long long y) { draw::put(t, x, y, colour); });
}

__global__ __launch_bounds__(kArrowThreads) void velocity_vectors_kernel(const ArrowArgs g) {
    const int ay = blockIdx.x / g.nx, ax = blockIdx.x - ay * g.nx;
    const int y = ay * g.row_step, x = ax * g.col_step;
    const size_t foff = (size_t)blockIdx.y * g.field_pitch + (size_t)y * g.fstride;
    const float uVal = reinterpret_cast<const float *>(reinterpret_cast<const char *>(g.u) + foff)[x];
    const float vVal = reinterpret_cast<const float *>(reinterpret_cast<const char *>(g.v) + foff)[x];
    if (!isfinite(uVal) || !isfinite(vVal) || fabsf(uVal) > 1e6f || fabsf(vVal) > 1e6f) return;
    const draw::Target img{g.img + (size_t)blockIdx.y * g.img_pitch, g.stride, g.rows, g.cols, 3};
    // micv_viz::arrowed_line(x, y, x + u, y + v): the float32 sums, rounded half to even (|value| <= 1e6 + cols: an int)
    const float x2f = (float)x + uVal, y2f = (float)y + vVal;
    const long long p1x = x, p1y = y, p2x = (long long)rintf(x2f), p2y = (long long)rintf(y2f);
    const double ddx = (double)p1x - (double)p2x, ddy = (double)p1y - (double)p2y;
    const double tip = sqrt(ddx * ddx + ddy * ddy) * 0.1;
    stroke(img, p1x, p1y, p2x, p2y, g.colour);
    const double angle = atan2(ddy, ddx), q = 3.14159265358979323846 / 4;
    long long px = (long long)rint((double)p2x + tip * cos(angle + q)), py = (long long)rint((double)p2y + tip * sin(angle + q));
    stroke(img, px, py, p2x, p2y, g.colour);
    px = (long long)rint((double)p2x + tip * cos(angle - q));
    py = (long long)rint((double)p2y + tip * sin(angle - q));
    stroke(img, px, py, p2x, p2y, g.colour);
}

// ---- savePyramid.  Launch 1: the ranges of the four levels (blockIdx.y = level), kept as display.hip keeps them: order-
// preserving keys, the complement of the minimum's, atomic max into a pair of words per level in a cache line of its own.
// Launch 2: one pass over the 2R x 2C montage.
constexpr int kLevels = 4;
constexpr int kKeyStride = micv_ctx::kDisplayKeyStride;  // words between two levels' pairs
struct MontageArgs {
    const void *lvl[kLevels];
    int rows[kLevels], cols[kLevels];
    size_t stride[kLevels];  // bytes
    double fy[kLevels], fx[kLevels];  // micv_viz::resize_nearest: (double)src.rows / R, (double)src.cols / C
    unsigned *keys;
    uint8_t *dst;
    size_t dstride;
    int R, C;
};

__global__ __launch_bounds__(256) void montage_ranges_kernel(const MontageArgs g) {
    const int l = blockIdx.y, rows = g.rows[l], cols = g.cols[l];
    const char *base = static_cast<const char *>(g.lvl[l]);
    const size_t n = (size_t)rows * cols;
    unsigned kmax = 0, kmin = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t y = i / cols, x = i - y * cols;
        const float f = reinterpret_cast<const float *>(base + y * g.stride[l])[x];
        if (f == f) {
            const unsigned k = key_of(f);
            kmax = max(kmax, k);
            kmin = max(kmin, ~k);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off));
        kmin = max(kmin, (unsigned)__shfl_xor((int)kmin, off));
    }
    __shared__ unsigned part[4][2];
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = kmin;
        part[threadIdx.x >> 6][1] = kmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            kmin = max(kmin, part[w][0]);
            kmax = max(kmax, part[w][1]);
        }
        if (kmax) {  // (a workgroup that saw NaNs only, or nothing, has nothing to say)
            atomicMax(g.keys + kKeyStride * l, kmin);
            atomicMax(g.keys + kKeyStride * l + 1, kmax);
        }
    }
}

template <bool F32>
__global__ __launch_bounds__(256) void montage_kernel(const MontageArgs g) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= 2 * g.C || Y >= 2 * g.R) return;
    const int ty = Y >= g.R, tx = X >= g.C, k = 2 * ty + tx, y = Y - ty * g.R, x = X - tx * g.C;
    // resize_nearest (level 0 has the factor 1.0: the pixel itself)
    const int sy = min((int)floor(y * g.fy[k]), g.rows[k] - 1), sx = min((int)floor(x * g.fx[k]), g.cols[k] - 1);
    const char *row = static_cast<const char *>(g.lvl[k]) + (size_t)sy * g.stride[k];
    uint8_t out;
    if (F32) {
        // the constants of micv_normalize_minmax_* (display.hip, apply_kernel), expression for expression
        const unsigned kmin = g.keys[kKeyStride * k], kmax = g.keys[kKeyStride * k + 1];
        float a = 0.f, b = 0.f;
        if (kmax) {
            const double lo = value_of(~kmin), hi = value_of(kmax);
            const double scale = 255.0 * (hi - lo > DBL_EPSILON ? 1.0 / (hi - lo) : 0.0), shift = 0.0 - lo * scale;
            a = (float)scale;
            b = (float)shift;
        }
        const float t = reinterpret_cast<const float *>(row)[sx] * a + b;
        const float r = fminf(fmaxf(rintf(t), 0.f), 255.f);
        out = isfinite(t) ? (uint8_t)(int)r : (uint8_t)0;
    } else {
        out = reinterpret_cast<const uint8_t *>(row)[sx];
    }
    g.dst[(size_t)Y * g.dstride + X] = out;
}

// ---- warpHelper's `prev - warped`: lk_warp_kernel's sample (warp_sample, lk_device.hpp), then one f32 subtraction
__global__ __launch_bounds__(256) void warp_diff_kernel(const float *__restrict__ prev, int pstride, const float *__restrict__ next,
                                                         int nstride, const float *__restrict__ du, const float *__restrict__ dv,
                                                         int fstride, int rows, int cols, float *__restrict__ diff, int dstride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const float w = warp_sample(next, rows, cols, nstride, x, y, du[(size_t)y * fstride + x], dv[(size_t)y * fstride + x]);
    diff[(size_t)y * dstride + x] = prev[(size_t)y * pstride + x] - w;
}

constexpr int kMaxSide = 32767;

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_draw_velocity_vectors_dev(micv_ctx *ctx, uint8_t *img, size_t img_pitch, size_t stride, const float *u, const float *v,
                                   size_t field_pitch, size_t fstride, int batch, int rows, int cols, const uint8_t *color,
                                   micv_stream stream) {
    MICV_REQUIRE(ctx && img && u && v && color, "micv_draw_velocity_vectors: null argument");
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide), "micv_draw_velocity_vectors: bad size %dx%d (1..32767)", rows, cols);
    MICV_REQUIRE(stride >= (size_t)cols * 3 && stride < (size_t)1 << 32 && stride_ok(fstride, cols, 4),
                 "micv_draw_velocity_vectors: the image's stride %zu or the fields' stride %zu does not hold %d columns", stride,
                 fstride, cols);
    MICV_REQUIRE(batch >= 0 && batch <= 65535, "micv_draw_velocity_vectors: batch %d out of 0..65535", batch);
    MICV_REQUIRE(batch <= 1 || (img_pitch >= (size_t)(rows - 1) * stride + (size_t)cols * 3 && field_pitch % 4 == 0 &&
                                field_pitch >= (size_t)(rows - 1) * fstride + (size_t)cols * 4),
                 "micv_draw_velocity_vectors: a pitch is smaller than an image or a field");
    if (batch == 0) return MICV_OK;
    MICV_HIP(hipSetDevice(ctx->device));
    ArrowArgs g;
    g.img = img; g.img_pitch = img_pitch; g.stride = stride;
    g.u = u; g.v = v; g.field_pitch = field_pitch; g.fstride = fstride;
    g.rows = rows; g.cols = cols;
    g.row_step = rows / 30 > 1 ? rows / 30 : 1;  // Solution.cpp:22-23; images under 30 pixels: 1, as micv_viz
    g.col_step = cols / 30 > 1 ? cols / 30 : 1;
    g.nx = (int)cdiv(cols, g.col_step);
    g.colour = (uint32_t)color[0] | (uint32_t)color[1] << 8 | (uint32_t)color[2] << 16;
    const unsigned arrows = cdiv(rows, g.row_step) * (unsigned)g.nx;  // at most 59 * 59
    velocity_vectors_kernel<<<dim3(arrows, batch), kArrowThreads, 0, static_cast<hipStream_t>(stream)>>>(g);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_gray_or_bgr_to_bgr8_dev(micv_ctx *ctx, const void *src, int depth, int channels, int rows, int cols, size_t sstride,
                                 uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_gray_or_bgr_to_bgr8: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U, "micv_gray_or_bgr_to_bgr8: depth %d not supported (8U, as micv_viz::drawVelocityVectors)", depth);
    MICV_REQUIRE(channels == 1 || channels == 3, "micv_gray_or_bgr_to_bgr8: %d channels not supported (1 or 3)", channels);
    MICV_REQUIRE(rows > 0 && cols > 0 && sstride >= (size_t)cols * channels && dstride >= (size_t)cols * 3,
                 "micv_gray_or_bgr_to_bgr8: bad size %dx%d or stride", rows, cols);
    MICV_REQUIRE(src != dst, "micv_gray_or_bgr_to_bgr8: src and dst alias");
    MICV_HIP(hipSetDevice(ctx->device));
    // prevImg.clone() and, for a grey frame, cv::cvtColor(GRAY2RGB): the image the arrows are drawn on
    return launch_to_bgr8(static_cast<hipStream_t>(stream), src, depth, channels, sstride, rows, cols, dst, dstride);
}

int micv_pyramid_montage_dev(micv_ctx *ctx, const void *const *levels, const int *level_rows, const int *level_cols,
                             const size_t *level_strides, int depth, uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && levels && level_rows && level_cols && level_strides && dst, "micv_pyramid_montage: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_32F || depth == MICV_DEPTH_8U, "micv_pyramid_montage: depth %d not supported (32F, 8U)", depth);
    const size_t e = depth == MICV_DEPTH_32F ? 4 : 1;
    MontageArgs g;
    for (int l = 0; l < kLevels; l++) {
        MICV_REQUIRE(levels[l] != nullptr, "micv_pyramid_montage: level %d is null", l);
        MICV_REQUIRE(level_rows[l] > 0 && level_cols[l] > 0 && level_rows[l] <= 16383 && level_cols[l] <= 16383 &&
                         stride_ok(level_strides[l], level_cols[l], e),
                     "micv_pyramid_montage: level %d: bad size %dx%d (1..16383) or stride", l, level_rows[l], level_cols[l]);
        g.lvl[l] = levels[l];
        g.rows[l] = level_rows[l];
        g.cols[l] = level_cols[l];
        g.stride[l] = level_strides[l];
    }
    g.R = level_rows[0];
    g.C = level_cols[0];
    for (int l = 0; l < kLevels; l++) {
        g.fy[l] = (double)g.rows[l] / g.R;
        g.fx[l] = (double)g.cols[l] / g.C;
    }
    MICV_REQUIRE(dstride >= (size_t)2 * g.C, "micv_pyramid_montage: stride %zu does not hold %d columns", dstride, 2 * g.C);
    g.dst = dst;
    g.dstride = dstride;
    g.keys = static_cast<unsigned *>(ctx->display_state) + 256;  // the key words of display.hip, reset by every call
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(cdiv(2 * g.C, 64), cdiv(2 * g.R, 4));
    if (depth == MICV_DEPTH_32F) {
        MICV_HIP(hipMemsetAsync(g.keys, 0, (size_t)kLevels * kKeyStride * 4, s));
        // about 4096 pixels per workgroup, at most 64 workgroups per level (128 atomics on a line)
        const unsigned bx = std::min(std::max(cdiv((unsigned)g.R * (unsigned)g.C, 4096u), 1u), 64u);
        montage_ranges_kernel<<<dim3(bx, kLevels), 256, 0, s>>>(g);
        MICV_LAUNCH_CHECK();
        montage_kernel<true><<<grid, 256, 0, s>>>(g);
    } else {
        montage_kernel<false><<<grid, 256, 0, s>>>(g);
    }
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_lk_warp_diff_dev(micv_ctx *ctx, const float *prev, size_t pstride, const float *next, size_t nstride, const float *du,
                          const float *dv, size_t fstride, int rows, int cols, float *diff, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && prev && next && du && dv && diff, "micv_lk_warp_diff: null argument");
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide), "micv_lk_warp_diff: bad size %dx%d", rows, cols);
    MICV_REQUIRE(stride_ok(pstride, cols, 4) && stride_ok(nstride, cols, 4) && stride_ok(fstride, cols, 4) && stride_ok(dstride, cols, 4),
                 "micv_lk_warp_diff: bad stride");
    // (the kernel promises __restrict__ on every pointer; next is read at other pixels than the one written)
    MICV_REQUIRE(next != diff && prev != diff && du != diff && dv != diff, "micv_lk_warp_diff: diff must not alias an input");
    MICV_HIP(hipSetDevice(ctx->device));
    warp_diff_kernel<<<dim3(cdiv(cols, 64), cdiv(rows, 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        prev, (int)(pstride / 4), next, (int)(nstride / 4), du, dv, (int)(fstride / 4), rows, cols, diff, (int)(dstride / 4));
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_ps5_warp_diff_seq_dev(micv_ctx *ctx, const float *frames, size_t frame_pitch, int nframes, int rows, int cols,
                               size_t stride, int win, uint8_t *diff_u8, size_t u8_pitch, size_t u8_stride, float *diff_f32,
                               float *u, float *v, micv_stream stream) {
    MICV_REQUIRE(ctx && frames && diff_u8, "micv_ps5_warp_diff_seq: null argument");
    MICV_REQUIRE(nframes >= 2 && nframes <= 1025, "micv_ps5_warp_diff_seq: %d frames (2..1025: at least one pair)", nframes);
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide) && stride_ok(stride, cols, 4), "micv_ps5_warp_diff_seq: bad size %dx%d or stride", rows, cols);
    MICV_REQUIRE(frame_pitch % 4 == 0 && frame_pitch >= (size_t)(rows - 1) * stride + (size_t)cols * 4,
                 "micv_ps5_warp_diff_seq: the frame pitch is smaller than a frame");
    MICV_REQUIRE((u == nullptr) == (v == nullptr), "micv_ps5_warp_diff_seq: give both flow outputs or none");
    MICV_REQUIRE(u8_stride >= (size_t)cols && u8_stride < (size_t)1 << 32 && u8_pitch >= (size_t)(rows - 1) * u8_stride + (size_t)cols,
                 "micv_ps5_warp_diff_seq: the 8-bit output's stride or pitch is smaller than its rows or images");
    MICV_REQUIRE(win >= 1 && win <= kMaxWin && (win & 1), "micv_ps5_warp_diff_seq: window %d (odd, 1..%d)", win, kMaxWin);
    MICV_HIP(hipSetDevice(ctx->device));
    const int pairs = nframes - 1;
    const size_t n = (size_t)rows * cols, rb = (size_t)cols * 4;
    // temporaries from the context's chain pool (micv_lk_flow_dev carves the arena itself): every difference, because the
    // normalisation takes them all at once, and ONE pair of flow fields, used by the pairs in turn (stream order)
    const size_t need = (diff_f32 ? 0 : Carver::need(n * pairs, 4)) + (u ? 0 : 2 * Carver::need(n, 4));
    Carver carve(nullptr);
    if (need) {
        void *pool;
        MICV_TRY(ctx->reserve_chain(need, &pool));
        carve = Carver(pool);
    }
    float *diffs = diff_f32 ? diff_f32 : carve.take<float>(n * pairs);
    float *tu = u ? nullptr : carve.take<float>(n), *tv = u ? nullptr : carve.take<float>(n);
    for (int p = 0; p < pairs; p++) {
        const float *prev = reinterpret_cast<const float *>(reinterpret_cast<const char *>(frames) + (size_t)p * frame_pitch);
        const float *next = reinterpret_cast<const float *>(reinterpret_cast<const char *>(frames) + (size_t)(p + 1) * frame_pitch);
        float *pu = u ? u + (size_t)p * n : tu, *pv = v ? v + (size_t)p * n : tv;
        MICV_TRY(micv_lk_flow_dev(ctx, prev, next, rows, cols, stride, win, pu, pv, rb, stream));
        MICV_TRY(micv_lk_warp_diff_dev(ctx, prev, stride, next, stride, pu, pv, rb, rows, cols, diffs + (size_t)p * n, rb, stream));
    }
    return micv_normalize_minmax_batch_dev(ctx, diffs, n * 4, MICV_DEPTH_32F, pairs, rows, cols, rb, diff_u8, u8_pitch, u8_stride,
                                           nullptr, 0, 0, nullptr, 0, 0, nullptr, stream);
}

int micv_dense_lk_display_dev(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols, size_t stride, int channels,
                              int depth, int mode, int win, int levels, const uint8_t *color, float *u, float *v, size_t ostride,
                              uint8_t *arrows, size_t astride, uint8_t *jet_u, uint8_t *jet_v, size_t jstride,
                              micv_stream stream) {
    MICV_REQUIRE(ctx && prev && next && color && u && v && arrows, "micv_dense_lk_display: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U, "micv_dense_lk_display: depth %d not supported (8-bit frames)", depth);
    MICV_REQUIRE(channels == 1 || channels == 3, "micv_dense_lk_display: %d channels not supported (1 or 3)", channels);
    MICV_REQUIRE(mode == MICV_LK_NAIVE || mode == MICV_LK_PYRAMIDAL, "micv_dense_lk_display: mode %d is neither naive (0) nor pyramidal (1)", mode);
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide) && stride >= (size_t)cols * channels && stride_ok(ostride, cols, 4) &&
                     astride >= (size_t)cols * 3 && astride < (size_t)1 << 32,
                 "micv_dense_lk_display: bad size %dx%d or stride", rows, cols);
    MICV_REQUIRE((jet_u == nullptr) == (jet_v == nullptr) && (!jet_u || (jstride >= (size_t)cols * 3 && jstride < (size_t)1 << 32)),
                 "micv_dense_lk_display: give both colour maps or none, with a stride that holds %d columns", cols);
    MICV_REQUIRE(u != v && (!jet_u || jet_u != jet_v), "micv_dense_lk_display: outputs alias");
    // (what the flow entries would refuse, refused before the conversions are launched)
    MICV_REQUIRE(win >= 1 && win <= kMaxWin && (win & 1), "micv_dense_lk_display: window %d must be odd and <= %d", win, kMaxWin);
    MICV_REQUIRE(mode == MICV_LK_NAIVE || (levels >= 1 && levels <= 16 && (rows >> (levels - 1)) > 0 && (cols >> (levels - 1)) > 0),
                 "micv_dense_lk_display: %d levels do not fit a %dx%d image", levels, rows, cols);
    MICV_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols, rb = (size_t)cols * 4;
    void *pool;
    MICV_TRY(ctx->reserve_chain(2 * Carver::need(n, 4), &pool));
    Carver carve(pool);
    float *gp = carve.take<float>(n), *gn = carve.take<float>(n);
    // Solution.cpp:48-61 converts before the naive flow; :63 hands the frames to lk::calcOpticalFlowPyr, whose
    // makeGaussianPyramid converts (Pyramids.cpp:9-15): the same conversion, as micv_lk_flow_pyr_frames_host runs it
    MICV_TRY(micv_to_gray_f32_dev(ctx, prev, rows, cols, stride, channels, depth, gp, rb, stream));
    MICV_TRY(micv_to_gray_f32_dev(ctx, next, rows, cols, stride, channels, depth, gn, rb, stream));
    if (mode == MICV_LK_NAIVE)
        MICV_TRY(micv_lk_flow_dev(ctx, gp, gn, rows, cols, rb, win, u, v, ostride, stream));
    else
        MICV_TRY(micv_lk_flow_pyr_dev(ctx, gp, gn, rows, cols, rb, win, levels, u, v, ostride, stream));
    MICV_TRY(micv_gray_or_bgr_to_bgr8_dev(ctx, prev, depth, channels, rows, cols, stride, arrows, astride, stream));
    MICV_TRY(micv_draw_velocity_vectors_dev(ctx, arrows, 0, astride, u, v, 0, ostride, 1, rows, cols, color, stream));
    if (!jet_u) return MICV_OK;
    // The two fields as a batch of two where v lies behind u and jet_v behind jet_u, as the Python and shim callers and the
    // _host twin allocate them; otherwise one call per field, which gives the same bytes (each field has its own range
    // either way).  The addresses are compared as integers: the buffers may be separate allocations.
    const uintptr_t ua = reinterpret_cast<uintptr_t>(u), va = reinterpret_cast<uintptr_t>(v);
    const uintptr_t ja = reinterpret_cast<uintptr_t>(jet_u), jb = reinterpret_cast<uintptr_t>(jet_v);
    if (va > ua && (va - ua) % 4 == 0 && va - ua >= (size_t)(rows - 1) * ostride + rb && jb > ja &&
        jb - ja >= (size_t)(rows - 1) * jstride + (size_t)cols * 3)
        return micv_normalize_minmax_batch_dev(ctx, u, (size_t)(va - ua), MICV_DEPTH_32F, 2, rows, cols, ostride, nullptr, 0, 0, nullptr, 0,
                                               0, jet_u, (size_t)(jb - ja), jstride, nullptr, stream);
    MICV_TRY(micv_normalize_minmax_dev(ctx, u, MICV_DEPTH_32F, rows, cols, ostride, nullptr, 0, nullptr, 0, jet_u, jstride, nullptr, stream));
    return micv_normalize_minmax_dev(ctx, v, MICV_DEPTH_32F, rows, cols, ostride, nullptr, 0, nullptr, 0, jet_v, jstride, nullptr, stream);
}

// denseLKWrapper in pyramidal mode over consecutive frames (Solution.cpp:254-285): the flows of all pairs from
// micv_lk_flow_seq_async, the arrow pictures in one launch, the colour maps of all u and of all v in one batch each.
int micv_dense_lk_display_seq_async(micv_ctx *ctx, const void *frames, size_t frame_pitch, int nframes, int rows, int cols,
                                    size_t stride, int channels, int depth, int win, int levels, const uint8_t *color, float *u,
                                    float *v, size_t opair_pitch, size_t ostride, uint8_t *arrows, size_t apitch, size_t astride,
                                    uint8_t *jet_u, uint8_t *jet_v, size_t jpitch, size_t jstride, micv_stream stream) {
    MICV_REQUIRE(ctx && frames && color && u && v && arrows, "micv_dense_lk_display_seq: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U, "micv_dense_lk_display_seq: depth %d not supported (8-bit frames)", depth);
    MICV_REQUIRE(channels == 1 || channels == 3, "micv_dense_lk_display_seq: %d channels not supported (1 or 3)", channels);
    MICV_REQUIRE(nframes >= 2 && nframes <= 32768, "micv_dense_lk_display_seq: %d frames (2 .. 32768)", nframes);
    const size_t irb = (size_t)cols * 3;
    MICV_REQUIRE(draw::size_ok(rows, cols, kMaxSide) && astride >= irb && astride < (size_t)1 << 32 &&
                     (nframes == 2 || apitch >= (size_t)(rows - 1) * astride + irb),
                 "micv_dense_lk_display_seq: bad size %dx%d, arrow stride or arrow pitch", rows, cols);
    MICV_REQUIRE((jet_u == nullptr) == (jet_v == nullptr) &&
                     (!jet_u || (jstride >= irb && jstride < (size_t)1 << 32 && (nframes == 2 || jpitch >= (size_t)(rows - 1) * jstride + irb))),
                 "micv_dense_lk_display_seq: give both colour maps or none, with a stride and a pitch that hold %d columns", cols);
    MICV_REQUIRE(u != v && (!jet_u || jet_u != jet_v), "micv_dense_lk_display_seq: outputs alias");
    // the rest of what a step below would refuse is refused by the first of them, before anything is enqueued
    MICV_TRY(micv_lk_flow_seq_async(ctx, frames, frame_pitch, nframes, rows, cols, stride, channels, depth, win, levels, 0, u, v, opair_pitch,
                                    ostride, stream));
    const int pairs = nframes - 1;
    for (int p = 0; p < pairs; p++)
        MICV_TRY(micv_gray_or_bgr_to_bgr8_dev(ctx, static_cast<const char *>(frames) + (size_t)p * frame_pitch, depth, channels, rows, cols, stride,
                                              arrows + (size_t)p * apitch, astride, stream));
    MICV_TRY(micv_draw_velocity_vectors_dev(ctx, arrows, apitch, astride, u, v, opair_pitch, ostride, pairs, rows, cols, color, stream));
    if (!jet_u) return MICV_OK;
    MICV_TRY(micv_normalize_minmax_batch_dev(ctx, u, opair_pitch, MICV_DEPTH_32F, pairs, rows, cols, ostride, nullptr, 0, 0, nullptr, 0, 0, jet_u,
                                             jpitch, jstride, nullptr, stream));
    return micv_normalize_minmax_batch_dev(ctx, v, opair_pitch, MICV_DEPTH_32F, pairs, rows, cols, ostride, nullptr, 0, 0, nullptr, 0, 0, jet_v,
                                           jpitch, jstride, nullptr, stream);
}

}  // extern "C"
