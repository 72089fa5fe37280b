// ps1.hip -- what the ps1 driver (ProblemSets/ps1_cpp/src/main.cpp) does around the Hough functions of hough.hip:
//   * before the edges: sol::gaussianBlur on 8-bit and float images, sol::generateEdge on float images, cv::erode with
//     the elliptic footprint (main.cpp:246-248);
//   * after the peaks: sol::findParallelLines, cv::cvtColor(GRAY2RGB), sol::drawLinesParametric, sol::drawCircles, all on
//     peak lists that stay in device memory (the lists and their counts are read by the kernels, never by the host).
// The OpenCV calls behind them are restated, PARITY UNPINNED (DESIGN.md sections 2 and 3).
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "draw.hpp"
#include "kernels.hpp"
#include "pixmap.hpp"

namespace micv {

template <typename T>
__device__ __forceinline__ T *row_ptr(T *base, size_t stride_bytes, int y) {
    return reinterpret_cast<T *>(reinterpret_cast<char *>(const_cast<typename std::remove_const<T>::type *>(base)) +
                                 (size_t)y * stride_bytes);
}

// ---- blur on CV_32FC1: gauss_u8_tiled_kernel (canny.hip) with float pixels; TO_U8 appends convertTo(CV_8U)
constexpr int GF_TW = 64, GF_TH = 16, GF_AMAX = 15;
template <bool TO_U8>
__global__ __launch_bounds__(256) void gauss_f32_tiled_kernel(const float *__restrict__ src, size_t stride, int rows, int cols,
                                                               Taps t, void *__restrict__ dst, size_t dstride) {
    __shared__ float S[(GF_TH + 2 * GF_AMAX) * (GF_TW + 2 * GF_AMAX)];
    __shared__ float R[(GF_TH + 2 * GF_AMAX) * GF_TW];
    const int a = t.n / 2, RW = GF_TW + 2 * a, RH = GF_TH + 2 * a;
    const int x0 = blockIdx.x * GF_TW, y0 = blockIdx.y * GF_TH;
    for (int i = threadIdx.x; i < RH * RW; i += 256) {  // the reflected source pixels, once
        const int ly = i / RW, lx = i - ly * RW;
        S[i] = row_ptr(src, stride, reflect101(y0 - a + ly, rows))[reflect101(x0 - a + lx, cols)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RH * GF_TW; i += 256) {  // row pass on every staged row
        const int ly = i / GF_TW, lx = i - ly * GF_TW;
        const float *s = S + ly * RW + lx;
        float acc = 0.f;
        for (int k = 0; k < t.n; k++) acc = fmaf(s[k], t.k[k], acc);
        R[i] = acc;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
    if (x >= cols) return;
    for (int ly = threadIdx.x >> 6; ly < GF_TH; ly += 4) {
        const int y = y0 + ly;
        if (y >= rows) break;
        float acc = 0.f;
        for (int k = 0; k < t.n; k++) acc = fmaf(R[(ly + k) * GF_TW + lx], t.k[k], acc);
        if (TO_U8)
            row_ptr(static_cast<uint8_t *>(dst), dstride, y)[x] = draw::f32_to_u8(acc);
        else
            row_ptr(static_cast<float *>(dst), dstride, y)[x] = acc;
    }
}

// ---- cv::erode, elliptic footprint up to 7 x 7: one LDS tile with a 3-cell halo (the footprint is not separable, so
// there is no plane between two passes); taps outside the image hold the border value.
struct EllipseRows {
    int hw[7];  // half-width of footprint row i
    int k;
};
constexpr int ER_TW = 64, ER_TH = 16, ER_HALO = 3;
template <typename T>
__global__ __launch_bounds__(256) void erode_ellipse_kernel(const T *__restrict__ src, size_t stride, int rows, int cols,
                                                             EllipseRows e, T border, T *__restrict__ dst, size_t dstride) {
    __shared__ T S[(ER_TH + 2 * ER_HALO) * (ER_TW + 2 * ER_HALO)];
    const int r = e.k / 2, RW = ER_TW + 2 * r, RH = ER_TH + 2 * r;
    const int x0 = blockIdx.x * ER_TW, y0 = blockIdx.y * ER_TH;
    for (int i = threadIdx.x; i < RH * RW; i += 256) {
        const int ly = i / RW, lx = i - ly * RW, y = y0 - r + ly, x = x0 - r + lx;
        S[i] = ((unsigned)y < (unsigned)rows && (unsigned)x < (unsigned)cols) ? row_ptr(src, stride, y)[x] : border;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
    if (x >= cols) return;
    for (int ly = threadIdx.x >> 6; ly < ER_TH; ly += 4) {
        const int y = y0 + ly;
        if (y >= rows) break;
        // v = first tap; v = (t < v) ? t : v in raster order (row 0 of the footprint is never empty)
        T v = S[ly * RW + lx + r - e.hw[0]];
        for (int i = 0; i < e.k; i++) {
            const T *s = S + (ly + i) * RW + lx + r;
            for (int dx = -e.hw[i]; dx <= e.hw[i]; dx++) {
                const T t = s[dx];
                v = (t < v) ? t : v;  // (the first tap against itself: t < v is false)
            }
        }
        row_ptr(dst, dstride, y)[x] = v;
    }
}

// ---- sol::findParallelLines: one workgroup, all pairs.  keep[i] = some j != i has the key of i; the kept pairs leave in
// input order (four consecutive peaks per thread, a scan over the 1024 thread counts).
constexpr int PL_MAX = 4096;
__global__ __launch_bounds__(1024) void parallel_lines_kernel(const uint32_t *__restrict__ peaks_rc, const int64_t *__restrict__ count_p,
                                                               unsigned max_peaks, unsigned delta_rho, unsigned delta_theta,
                                                               uint32_t *__restrict__ out_rc, int64_t *__restrict__ out_count) {
    __shared__ unsigned long long key[PL_MAX];
    __shared__ unsigned char keep[PL_MAX];
    __shared__ int scan[1024];
    const int tid = threadIdx.x;
    const int64_t c = *count_p;
    const int n = (int)(c < 0 ? 0 : (c < (int64_t)max_peaks ? c : (int64_t)max_peaks));
    for (int i = tid; i < n; i += 1024) {
        const uint32_t rb = peaks_rc[2 * i] / delta_rho * delta_rho, tb = peaks_rc[2 * i + 1] / delta_theta * delta_theta;
        key[i] = ((unsigned long long)rb << 32) | tb;  // Solution.cpp:146-150
    }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const unsigned long long k = key[i];
        bool any = false;
        for (int j = 0; j < n; j++) any = any || (j != i && key[j] == k);
        keep[i] = any;
    }
    __syncthreads();
    int mine = 0;
    for (int q = 0; q < 4; q++) mine += (4 * tid + q < n && keep[4 * tid + q]) ? 1 : 0;
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan
        const int v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int at = scan[tid] - mine;
    for (int q = 0; q < 4; q++) {
        const int i = 4 * tid + q;
        if (i < n && keep[i]) {
            out_rc[2 * at] = peaks_rc[2 * i];
            out_rc[2 * at + 1] = peaks_rc[2 * i + 1];
            at++;
        }
    }
    if (tid == 1023) *out_count = scan[1023];
}

// ---- sol::drawLinesParametric.  blockIdx.y = the peak; a thread is one step along the segment's major axis, and only
// the steps whose major coordinate lies inside the image are dealt out (the end points of a near-vertical line lie up to
// ~115 image diagonals outside, far inside the narrow walk's bound): draw.hpp.
struct LineTrig {
    float c[180], s[180];  // cos / sin of the float radian of theta = -90 + i
};
__global__ __launch_bounds__(256) void draw_lines_parametric_kernel(uint8_t *__restrict__ pixels, int rows, int cols, size_t stride,
                                                                     const uint32_t *__restrict__ peaks_rc,
                                                                     const int64_t *__restrict__ count_p, unsigned max_peaks,
                                                                     unsigned rho_bin, unsigned theta_bin, long long diag,
                                                                     LineTrig trig, uint32_t colour) {
    const draw::Target img{pixels, stride, rows, cols, 3};  // (3 where put can see it: its byte loop unrolls)
    const int64_t cnt = *count_p;
    if ((int64_t)blockIdx.y >= cnt || blockIdx.y >= max_peaks) return;
    const uint32_t row = peaks_rc[2 * blockIdx.y], col = peaks_rc[2 * blockIdx.y + 1];
    const unsigned long long tcol = (unsigned long long)col * theta_bin;
    if (tcol >= 180) return;
    const int theta = (int)tcol - 90;                                                   // Solution.cpp:87
    const int rho = (int)(uint32_t)((unsigned long long)row * rho_bin - (unsigned long long)diag);  // :86
    const float frho = (float)rho;
    float fx1, fy1, fx2, fy2;
    if (theta != 0) {  // thetaRad = theta * PI / 180.f is zero only for theta = 0
        const float cs = trig.c[theta + 90], sn = trig.s[theta + 90];
        const float slope = (-1.f * cs) / sn, c = frho / sn;  // :102-103
        fx1 = 0.f;
        fx2 = (float)img.cols;
        fy1 = slope * fx1 + c;
        fy2 = slope * fx2 + c;
    } else {
        fy1 = 0.f;
        fy2 = (float)img.rows;
        fx1 = fx2 = frho / trig.c[90];
    }
    const draw::LineWalk w = draw::line_walk(img.rows, img.cols, lrintf(fx1), lrintf(fy1), lrintf(fx2), lrintf(fy2));  // Point2f -> Point
    draw::walk_steps(w, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, draw::narrow_minor(w),
                     [&](long long x, long long y) { draw::put(img, x, y, colour); });
}

// ---- sol::drawCircles: cv::circle, thickness 1 (draw.hpp, circle_walk); a thread is a circle.
__global__ __launch_bounds__(64) void draw_circles_kernel(uint8_t *__restrict__ pixels, int rows, int cols, size_t stride,
                                                           const uint32_t *__restrict__ peaks_rc, const int64_t *__restrict__ counts,
                                                           unsigned n_radii, unsigned num_peaks, unsigned min_radius, uint32_t colour) {
    const draw::Target img{pixels, stride, rows, cols, 3};
    const unsigned long long t = (unsigned long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= (unsigned long long)n_radii * num_peaks) return;
    const unsigned ri = (unsigned)(t / num_peaks), k = (unsigned)(t - (unsigned long long)ri * num_peaks);
    if ((int64_t)k >= counts[ri]) return;
    const uint32_t cy_u = peaks_rc[2 * t], cx_u = peaks_rc[2 * t + 1];
    if (cy_u > 65535u || cx_u > 65535u) return;
    const long long cx = cx_u, cy = cy_u, radius = (long long)min_radius + ri;
    if (!draw::circle_reaches(cx, cy, radius, img.rows, img.cols)) return;
    draw::circle_walk(radius, [&](long long dx, long long dy) {
        draw::put(img, cx + dx, cy + dy, colour);
        draw::put(img, cx - dx, cy + dy, colour);
        draw::put(img, cx + dx, cy - dy, colour);
        draw::put(img, cx - dx, cy - dy, colour);
        draw::put(img, cx + dy, cy + dx, colour);
        draw::put(img, cx - dy, cy + dx, colour);
        draw::put(img, cx + dy, cy - dx, colour);
        draw::put(img, cx - dy, cy - dx, colour);
    });
}

// cv::getStructuringElement(MORPH_ELLIPSE, Size(k, k)): the half-width of every row, in double as OpenCV computes it
static bool ellipse_rows(int ksize, EllipseRows *e) {
    static const int want[4][7] = {{0}, {0, 1, 0}, {0, 2, 2, 2, 0}, {0, 2, 3, 3, 3, 2, 0}};
    const int r = ksize / 2, c = ksize / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    e->k = ksize;
    for (int i = 0; i < 7; i++) e->hw[i] = 0;
    for (int i = 0; i < ksize; i++) {
        const int dy = i - r;
        const long hw = std::lrint(c * std::sqrt((r * r - dy * dy) * inv_r2));
        if (hw < 0 || hw > c || hw != want[r][i]) return false;
        e->hw[i] = (int)hw;
    }
    return true;
}

// three colour bytes as put takes them
static uint32_t bgr_word(const uint8_t *c) { return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16; }

static bool gauss_ok(int n, double sigma) { return n >= 1 && n <= 31 && (n & 1) && sigma > 0; }

int launch_gauss_f32_to_u8(hipStream_t s, const float *src, size_t stride, int rows, int cols, const Taps &t, uint8_t *dst, size_t dstride) {
    gauss_f32_tiled_kernel<true><<<dim3(cdiv(cols, GF_TW), cdiv(rows, GF_TH)), 256, 0, s>>>(src, stride, rows, cols, t, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace micv

using namespace micv;

extern "C" {

int micv_gaussian_blur_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int gauss_size,
                              double gauss_sigma, uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_gaussian_blur_u8: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols, "micv_gaussian_blur_u8: bad size / stride");
    MICV_REQUIRE(gauss_ok(gauss_size, gauss_sigma), "micv_gaussian_blur_u8: gaussian %d / sigma %g not supported (odd size <= 31, sigma > 0)",
                 gauss_size, gauss_sigma);
    MICV_HIP(hipSetDevice(ctx->device));
    Taps t;
    gaussian_taps(gauss_size, gauss_sigma, &t);
    return launch_gauss_u8(static_cast<hipStream_t>(stream), src, sstride, rows, cols, t, dst, dstride);
}

int micv_gaussian_blur_f32_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int gauss_size,
                               double gauss_sigma, float *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_gaussian_blur_f32: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride_ok(sstride, cols, 4) && stride_ok(dstride, cols, 4),
                 "micv_gaussian_blur_f32: bad size / stride");
    MICV_REQUIRE(gauss_ok(gauss_size, gauss_sigma), "micv_gaussian_blur_f32: gaussian %d / sigma %g not supported (odd size <= 31, sigma > 0)",
                 gauss_size, gauss_sigma);
    MICV_HIP(hipSetDevice(ctx->device));
    Taps t;
    gaussian_taps(gauss_size, gauss_sigma, &t);
    gauss_f32_tiled_kernel<false><<<dim3(cdiv(cols, GF_TW), cdiv(rows, GF_TH)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        src, sstride, rows, cols, t, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_generate_edge_f32_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t stride, int gauss_size,
                               double gauss_sigma, double low_thresh, double high_thresh, uint8_t *edges, size_t estride,
                               micv_stream stream) {
    MICV_REQUIRE(ctx && src && edges, "micv_generate_edge_f32: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride_ok(stride, cols, 4) && estride >= (size_t)cols, "micv_generate_edge_f32: bad size / stride");
    MICV_REQUIRE(gauss_ok(gauss_size, gauss_sigma), "micv_generate_edge_f32: gaussian %d / sigma %g not supported (odd size <= 31, sigma > 0)",
                 gauss_size, gauss_sigma);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)rows * cols, nwords = (size_t)rows * cdiv(cols, 64);
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need(n, 1) + Carver::need(nwords, 8) * 2 + 256, &scratch));
    Carver c(scratch);
    uint8_t *blur = c.take<uint8_t>(n);
    unsigned long long *weak = c.take<unsigned long long>(nwords), *strong = c.take<unsigned long long>(nwords);
    Taps t;
    gaussian_taps(gauss_size, gauss_sigma, &t);  // (a 1-tap Gaussian is the tap 1.0: the kernel is then the conversion alone)
    gauss_f32_tiled_kernel<true><<<dim3(cdiv(cols, GF_TW), cdiv(rows, GF_TH)), 256, 0, s>>>(src, stride, rows, cols, t, blur, (size_t)cols);
    MICV_LAUNCH_CHECK();
    return canny_from_u8(ctx, s, blur, (size_t)cols, rows, cols, low_thresh, high_thresh, weak, strong, edges, estride);
}

int micv_erode_ellipse_f32_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int ksize, float *dst,
                               size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_erode_ellipse_f32: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride_ok(sstride, cols, 4) && stride_ok(dstride, cols, 4),
                 "micv_erode_ellipse_f32: bad size / stride");
    MICV_REQUIRE(src != dst, "micv_erode_ellipse_f32: in-place not supported");
    EllipseRows e;
    MICV_REQUIRE(ksize >= 1 && ksize <= 7 && (ksize & 1) && ellipse_rows(ksize, &e), "micv_erode_ellipse_f32: ksize %d not supported (odd, 1..7)", ksize);
    MICV_HIP(hipSetDevice(ctx->device));
    erode_ellipse_kernel<float><<<dim3(cdiv(cols, ER_TW), cdiv(rows, ER_TH)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        src, sstride, rows, cols, e, FLT_MAX, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_erode_ellipse_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int ksize,
                              uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_erode_ellipse_u8: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols, "micv_erode_ellipse_u8: bad size / stride");
    MICV_REQUIRE(src != dst, "micv_erode_ellipse_u8: in-place not supported");
    EllipseRows e;
    MICV_REQUIRE(ksize >= 1 && ksize <= 7 && (ksize & 1) && ellipse_rows(ksize, &e), "micv_erode_ellipse_u8: ksize %d not supported (odd, 1..7)", ksize);
    MICV_HIP(hipSetDevice(ctx->device));
    erode_ellipse_kernel<uint8_t><<<dim3(cdiv(cols, ER_TW), cdiv(rows, ER_TH)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        src, sstride, rows, cols, e, (uint8_t)255, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_parallel_lines_dev(micv_ctx *ctx, const uint32_t *peaks_rc, const int64_t *count, unsigned max_peaks,
                            unsigned delta_rho, unsigned delta_theta, uint32_t *out_rc, int64_t *out_count,
                            micv_stream stream) {
    MICV_REQUIRE(ctx && count && out_count && ((peaks_rc && out_rc) || max_peaks == 0), "micv_parallel_lines: null argument");
    MICV_REQUIRE(max_peaks <= (unsigned)PL_MAX, "micv_parallel_lines: %u peaks > 4096 not supported", max_peaks);
    MICV_REQUIRE(delta_rho > 0 && delta_theta > 0, "micv_parallel_lines: delta_rho and delta_theta must be positive");
    MICV_HIP(hipSetDevice(ctx->device));
    parallel_lines_kernel<<<1, 1024, 0, static_cast<hipStream_t>(stream)>>>(peaks_rc, count, max_peaks, delta_rho, delta_theta,
                                                                            out_rc, out_count);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_gray_to_rgb8_dev(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride, uint8_t *dst,
                          size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_gray_to_rgb8: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_gray_to_rgb8: depth %d not supported (8U, 32F)", depth);
    MICV_REQUIRE(rows > 0 && cols > 0 && dstride >= (size_t)cols * 3 &&
                     (depth == MICV_DEPTH_8U ? sstride >= (size_t)cols : stride_ok(sstride, cols, 4)),
                 "micv_gray_to_rgb8: bad size / stride");
    MICV_HIP(hipSetDevice(ctx->device));
    return launch_to_bgr8(static_cast<hipStream_t>(stream), src, depth, 1, sstride, rows, cols, dst, dstride);
}

int micv_draw_lines_parametric_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride,
                                   const uint32_t *peaks_rc, const int64_t *count, unsigned max_peaks, unsigned rho_bin,
                                   unsigned theta_bin, const uint8_t *color, micv_stream stream) {
    MICV_REQUIRE(ctx && img && count && color && (peaks_rc || max_peaks == 0), "micv_draw_lines_parametric: null argument");
    MICV_REQUIRE(draw::image_ok(rows, cols, 3, stride, 32767), "micv_draw_lines_parametric: bad size / stride");
    MICV_REQUIRE(max_peaks <= 4096 && rho_bin > 0 && theta_bin > 0, "micv_draw_lines_parametric: bad peak count / bin size");
    if (max_peaks == 0) return MICV_OK;
    MICV_HIP(hipSetDevice(ctx->device));
    LineTrig trig;
    for (int i = 0; i < 180; i++) {
        const float rad = (float)(-90 + i) * 3.14159265f / 180.f;  // Solution.cpp:95, float throughout
        trig.c[i] = (float)std::cos((double)rad);
        trig.s[i] = (float)std::sin((double)rad);
    }
    const int longest = rows > cols ? rows : cols;
    draw_lines_parametric_kernel<<<dim3(cdiv(longest, 256), max_peaks), 256, 0, static_cast<hipStream_t>(stream)>>>(
        img, rows, cols, stride, peaks_rc, count, max_peaks, rho_bin, theta_bin, (long long)hough_diag(rows, cols), trig,
        bgr_word(color));
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_draw_circles_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride, const uint32_t *peaks_rc,
                          const int64_t *counts, unsigned n_radii, unsigned num_peaks, unsigned min_radius,
                          const uint8_t *color, micv_stream stream) {
    MICV_REQUIRE(ctx && img && color, "micv_draw_circles: null argument");
    MICV_REQUIRE(draw::image_ok(rows, cols, 3, stride, 32767), "micv_draw_circles: bad size / stride");
    MICV_REQUIRE(num_peaks <= 4096 && (unsigned long long)n_radii * num_peaks < (1ull << 31), "micv_draw_circles: too many circles");
    if (n_radii == 0 || num_peaks == 0) return MICV_OK;
    MICV_REQUIRE(peaks_rc && counts, "micv_draw_circles: null argument");
    MICV_HIP(hipSetDevice(ctx->device));
    const unsigned total = n_radii * num_peaks;
    draw_circles_kernel<<<cdiv(total, 64), 64, 0, static_cast<hipStream_t>(stream)>>>(img, rows, cols, stride, peaks_rc, counts,
                                                                                     n_radii, num_peaks, min_radius, bgr_word(color));
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // extern "C"
