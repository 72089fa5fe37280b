// ps0.hip -- ps0 of the reference (ProblemSets/ps0_cpp/main.cpp) on the device: swapRedBlue and cv::extractChannel
// (:17-23, :118-129), pixelReplacement (:25-42), cv::minMaxLoc + cv::meanStdDev (:135-138), doArithmeticOperations
// (:47-56), `a -= b` on 8-bit images (:156-157), addGaussianNoise (:64-79) and main's whole solution (:110-171) as one
// call.  OpenCV's behaviour is restated, PARITY UNPINNED ("ps0"); the statement of the contract is
// the host loops of shim/micv_ps0.hpp and include/mi_cv.h, "ps0".  No `_dev` entry synchronises the host; mean and
// stddev are read where the reduction left them.
//
// The reduction: every thread sums at most 8192 pixels in 32 bits (8192 * 255^2 < 2^32), the workgroup joins its 256
// partials in 64 bits and writes ONE partial record; whichever kernel runs next adds the (at most 1024) partials, again in
// integers, and forms mean and stddev.  No workgroup waits for another and the sums do not depend on the grid.
#include <climits>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "host_io.hpp"

namespace micv {
namespace {

constexpr int kT = 256, kMaxBlocks = 1024;

struct Part {
    unsigned long long sum, sq;
    int mn, mx;
};

__device__ __forceinline__ int cv_round_d(double v) {  // cvRound(double): half to even, INT_MIN outside int and for NaN
    const double r = rint(v);
    return (r >= -2147483648.0 && r < 2147483648.0) ? (int)r : INT_MIN;
}
__device__ __forceinline__ int cv_round_f(float v) {
    return (v >= -2147483648.f && v < 2147483648.f) ? (int)rintf(v) : INT_MIN;
}
__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the four saturating steps of doArithmeticOperations; a = (float)(1.0 / stddev)
__device__ __forceinline__ uint8_t arith_px(int p, double mean, float a) {
    const int t1 = sat8(cv_round_d((double)p - mean));
    const int t2 = sat8(cv_round_f((float)t1 * a));
    const int t3 = sat8(cv_round_f((float)t2 * 10.f));
    return (uint8_t)sat8(cv_round_d((double)t3 + mean));
}

// addGaussianNoise: both operands as CV_8SC1 (the image clipped at 127), the sum saturated to s8, then to u8
__device__ __forceinline__ uint8_t noise_px(int p, float z) {
    int n = cv_round_f(z);
    n = n < -128 ? -128 : (n > 127 ? 127 : n);
    int s = (p > 127 ? 127 : p) + n;
    s = s < -128 ? -128 : (s > 127 ? 127 : s);
    return (uint8_t)(s < 0 ? 0 : s);
}

// Joins the workgroup's values; the result is valid in every thread.
__device__ Part block_join(unsigned long long sum, unsigned long long sq, int mn, int mx) {
    __shared__ Part sh[kT];
    const int t = threadIdx.x;
    sh[t] = Part{sum, sq, mn, mx};
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[t].sum += sh[t + s].sum;
            sh[t].sq += sh[t + s].sq;
            sh[t].mn = min(sh[t].mn, sh[t + s].mn);
            sh[t].mx = max(sh[t].mx, sh[t + s].mx);
        }
        __syncthreads();
    }
    const Part out = sh[0];
    __syncthreads();
    return out;
}

__device__ Part join_parts(const Part *parts, int nparts) {
    unsigned long long sum = 0, sq = 0;
    int mn = 255, mx = 0;
    for (int i = threadIdx.x; i < nparts; i += kT) {
        sum += parts[i].sum, sq += parts[i].sq;
        mn = min(mn, parts[i].mn), mx = max(mx, parts[i].mx);
    }
    return block_join(sum, sq, mn, mx);
}

__device__ __forceinline__ micv_ps0_stats stats_of(const Part &p, long long n) {
    micv_ps0_stats s;
    const double inv = 1.0 / (double)n;
    s.mean = (double)p.sum * inv;
    const double var = (double)p.sq * inv - s.mean * s.mean;
    s.stddev = sqrt(var > 0.0 ? var : 0.0);
    s.sum = p.sum, s.sqsum = p.sq, s.min = p.mn, s.max = p.mx;
    return s;
}

__global__ void __launch_bounds__(kT) mix_kernel(const uint8_t *src, size_t sstride, int scn, uint8_t *dst, size_t dstride, int dcn,
                                                 int m0, int m1, int m2, int m3, int rows, int cols) {
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const int y = (int)(i / cols), x = (int)(i % cols);
        const uint8_t *s = src + (size_t)y * sstride + (size_t)x * scn;
        uint8_t *d = dst + (size_t)y * dstride + (size_t)x * dcn;
        d[0] = s[m0];
        if (dcn > 1) d[1] = s[m1];
        if (dcn > 2) d[2] = s[m2];
        if (dcn > 3) d[3] = s[m3];
    }
}

// dst = b, with the size x size square of a at (ax, ay) pasted at (bx, by); cn bytes per pixel are copied, the pixels of
// a and b lie apx and bpx bytes apart (a plane of an interleaved image: cn = 1, px = channels)
struct Paste {
    const uint8_t *a, *b;
    uint8_t *dst;
    size_t astride, bstride, dstride;
    int apx, bpx, cn, rows, cols, ax, ay, bx, by, size;
};
__global__ void __launch_bounds__(kT) paste_kernel(const Paste p) {
    const long long n = (long long)p.rows * p.cols;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const int y = (int)(i / p.cols), x = (int)(i % p.cols);
        const bool in = x >= p.bx && x < p.bx + p.size && y >= p.by && y < p.by + p.size;
        const uint8_t *s = in ? p.a + (size_t)(y - p.by + p.ay) * p.astride + (size_t)(x - p.bx + p.ax) * p.apx
                              : p.b + (size_t)y * p.bstride + (size_t)x * p.bpx;
        uint8_t *d = p.dst + (size_t)y * p.dstride + (size_t)x * p.cn;
        for (int k = 0; k < p.cn; k++) d[k] = s[k];
    }
}

// One partial per workgroup of a single-channel image whose pixels lie px bytes apart.  With `swapped` (pass one of the
// run) src is B, G, R: the swapped image and the green and red planes are written and green is what is reduced.
__global__ void __launch_bounds__(kT) stats_kernel(const uint8_t *src, size_t sstride, int px, int rows, int cols, Part *parts,
                                                   uint8_t *swapped, size_t wstride, uint8_t *green, uint8_t *red, size_t pstride) {
    const long long n = (long long)rows * cols;
    unsigned sum = 0, sq = 0;
    int mn = 255, mx = 0;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const int y = (int)(i / cols), x = (int)(i % cols);
        const uint8_t *s = src + (size_t)y * sstride + (size_t)x * px;
        unsigned v = s[0];
        if (swapped) {
            const uint8_t b = s[0], g = s[1], r = s[2];
            uint8_t *w = swapped + (size_t)y * wstride + 3 * (size_t)x;
            w[0] = r, w[1] = g, w[2] = b;
            green[(size_t)y * pstride + x] = g;
            red[(size_t)y * pstride + x] = r;
            v = g;
        }
        sum += v, sq += v * v;
        mn = min(mn, (int)v), mx = max(mx, (int)v);
    }
    const Part p = block_join(sum, sq, mn, mx);
    if (threadIdx.x == 0) parts[blockIdx.x] = p;
}

__global__ void __launch_bounds__(kT) stats_finish_kernel(const Part *parts, int nparts, long long n, micv_ps0_stats *out) {
    const Part p = join_parts(parts, nparts);
    if (threadIdx.x == 0) *out = stats_of(p, n);
}

__global__ void __launch_bounds__(kT) arith_kernel(const uint8_t *src, size_t sstride, int rows, int cols, const double *ms, uint8_t *dst,
                                                   size_t dstride) {
    const double mean = ms[0];
    const float a = (float)(1.0 / ms[1]);
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const int y = (int)(i / cols), x = (int)(i % cols);
        dst[(size_t)y * dstride + x] = arith_px(src[(size_t)y * sstride + x], mean, a);
    }
}

__global__ void __launch_bounds__(kT) subtract_kernel(const uint8_t *a, size_t astride, const uint8_t *b, size_t bstride, int rows, int cols,
                                                      uint8_t *dst, size_t dstride) {
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const int y = (int)(i / cols), x = (int)(i % cols);
        const int d = (int)a[(size_t)y * astride + x] - (int)b[(size_t)y * bstride + x];
        dst[(size_t)y * dstride + x] = (uint8_t)(d < 0 ? 0 : d);
    }
}

__global__ void __launch_bounds__(kT) noise_kernel(const uint8_t *src, size_t sstride, const float *noise, size_t nstride, int rows, int cols,
                                                   uint8_t *dst, size_t dstride) {
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const int y = (int)(i / cols), x = (int)(i % cols);
        const float z = reinterpret_cast<const float *>(reinterpret_cast<const char *>(noise) + (size_t)y * nstride)[x];
        dst[(size_t)y * dstride + x] = noise_px(src[(size_t)y * sstride + x], z);
    }
}

// Pass two of the run: mean and stddev from the partials in the prologue, then everything that depends on green.
struct Pass2 {
    const Part *parts;
    int nparts, rows, cols;
    const uint8_t *img1;  // B, G, R: blue is read here
    size_t s1;
    const uint8_t *green;
    const float *ng, *nb;
    size_t nstride, pstride;
    uint8_t *arith, *trans, *diff, *noisy_g, *noisy_b;
    micv_ps0_stats *stats;
};
__global__ void __launch_bounds__(kT) pass2_kernel(const Pass2 p) {
    const long long n = (long long)p.rows * p.cols;
    const micv_ps0_stats st = stats_of(join_parts(p.parts, p.nparts), n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *p.stats = st;
    const float a = (float)(1.0 / st.stddev);
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const int y = (int)(i / p.cols), x = (int)(i % p.cols);
        const size_t o = (size_t)y * p.pstride + x;
        const int g = p.green[o];
        const int t = x + 2 < p.cols ? p.green[o + 2] : 0;  // warpAffine by (-2, 0), zero fill
        const size_t no = (size_t)y * p.nstride;
        p.arith[o] = arith_px(g, st.mean, a);
        p.trans[o] = (uint8_t)t;
        p.diff[o] = (uint8_t)(g - t < 0 ? 0 : g - t);
        p.noisy_g[o] = noise_px(g, reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.ng) + no)[x]);
        p.noisy_b[o] = noise_px(p.img1[(size_t)y * p.s1 + 3 * (size_t)x],
                                reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.nb) + no)[x]);
    }
}

unsigned grid_for(long long n) {  // at most 8192 pixels per thread up to n = 2^31
    const long long b = (n + kT * 8 - 1) / (kT * 8);
    return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

bool plane_ok(const void *p, int rows, int cols, int cn, size_t stride) {
    return p && rows > 0 && cols > 0 && (long long)rows * cols < (1LL << 31) && stride >= (size_t)cols * cn;
}

// the square's corners; false when it leaves either image (OpenCV throws there)
bool squares(int r1, int c1, int r2, int c2, int size, Paste *p) {
    if (size < 0) return false;
    p->ax = c1 / 2 - size / 2, p->ay = r1 / 2 - size / 2, p->bx = c2 / 2 - size / 2, p->by = r2 / 2 - size / 2, p->size = size;
    return p->ax >= 0 && p->ay >= 0 && p->bx >= 0 && p->by >= 0 && p->ax + size <= c1 && p->ay + size <= r1 && p->bx + size <= c2 &&
           p->by + size <= r2;
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_mix_channels_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, int scn, size_t sstride, const int *map, uint8_t *dst,
                             int dcn, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && map && scn >= 1 && scn <= 4 && dcn >= 1 && dcn <= 4, "micv_mix_channels_u8: null argument or channels outside 1..4");
    MICV_REQUIRE(plane_ok(src, rows, cols, scn, sstride) && plane_ok(dst, rows, cols, dcn, dstride), "micv_mix_channels_u8: bad image");
    int m[4] = {0, 0, 0, 0};
    for (int k = 0; k < dcn; k++) {
        MICV_REQUIRE(map[k] >= 0 && map[k] < scn, "micv_mix_channels_u8: map[%d] = %d outside the source's %d channels", k, map[k], scn);
        m[k] = map[k];
    }
    MICV_HIP(hipSetDevice(ctx->device));
    mix_kernel<<<grid_for((long long)rows * cols), kT, 0, static_cast<hipStream_t>(stream)>>>(src, sstride, scn, dst, dstride, dcn, m[0], m[1],
                                                                                             m[2], m[3], rows, cols);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_mix_channels_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, int scn, size_t sstride, const int *map, uint8_t *dst,
                              int dcn, size_t dstride) {
    MICV_REQUIRE(ctx && scn >= 1 && scn <= 4 && dcn >= 1 && dcn <= 4 && plane_ok(src, rows, cols, scn, sstride) &&
                     plane_ok(dst, rows, cols, dcn, dstride),
                 "micv_mix_channels_u8_host: bad argument");
    HostCall h(ctx, "micv_mix_channels_u8_host");
    const size_t sb = (size_t)cols * scn, db = (size_t)cols * dcn;
    uint8_t *s = h.up<uint8_t>(src, sstride, sb, rows), *d = h.alloc<uint8_t>(db * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mix_channels_u8_dev(ctx, s, rows, cols, scn, sb, map, d, dcn, db, h.s));
    h.down(dst, dstride, d, db, rows);
    return h.finish();
}

int micv_pixel_replacement_u8_dev(micv_ctx *ctx, const uint8_t *img1, int rows1, int cols1, size_t stride1, const uint8_t *img2, int rows2,
                                  int cols2, size_t stride2, int channels, int size, uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && channels >= 1 && channels <= 4 && plane_ok(img1, rows1, cols1, channels, stride1) &&
                     plane_ok(img2, rows2, cols2, channels, stride2) && plane_ok(dst, rows2, cols2, channels, dstride),
                 "micv_pixel_replacement_u8: bad argument");
    MICV_REQUIRE(dst != img1 && dst != img2, "micv_pixel_replacement_u8: dst must not alias an input");
    Paste p{};
    MICV_REQUIRE(squares(rows1, cols1, rows2, cols2, size, &p), "micv_pixel_replacement_u8: the %d x %d square leaves %dx%d or %dx%d", size,
                 size, rows1, cols1, rows2, cols2);
    p.a = img1, p.b = img2, p.dst = dst, p.astride = stride1, p.bstride = stride2, p.dstride = dstride;
    p.apx = p.bpx = p.cn = channels, p.rows = rows2, p.cols = cols2;
    MICV_HIP(hipSetDevice(ctx->device));
    paste_kernel<<<grid_for((long long)rows2 * cols2), kT, 0, static_cast<hipStream_t>(stream)>>>(p);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_pixel_replacement_u8_host(micv_ctx *ctx, const uint8_t *img1, int rows1, int cols1, size_t stride1, const uint8_t *img2, int rows2,
                                   int cols2, size_t stride2, int channels, int size, uint8_t *dst, size_t dstride) {
    MICV_REQUIRE(ctx && channels >= 1 && channels <= 4 && plane_ok(img1, rows1, cols1, channels, stride1) &&
                     plane_ok(img2, rows2, cols2, channels, stride2) && plane_ok(dst, rows2, cols2, channels, dstride),
                 "micv_pixel_replacement_u8_host: bad argument");
    Paste q{};
    MICV_REQUIRE(squares(rows1, cols1, rows2, cols2, size, &q), "micv_pixel_replacement_u8_host: the %d x %d square leaves an image", size, size);
    HostCall h(ctx, "micv_pixel_replacement_u8_host");
    const size_t b1 = (size_t)cols1 * channels, b2 = (size_t)cols2 * channels;
    uint8_t *a = h.up<uint8_t>(img1, stride1, b1, rows1), *b = h.up<uint8_t>(img2, stride2, b2, rows2), *d = h.alloc<uint8_t>(b2 * rows2);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_pixel_replacement_u8_dev(ctx, a, rows1, cols1, b1, b, rows2, cols2, b2, channels, size, d, b2, h.s));
    h.down(dst, dstride, d, b2, rows2);
    return h.finish();
}

int micv_mean_stddev_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride, micv_ps0_stats *stats, micv_stream stream) {
    MICV_REQUIRE(ctx && stats && plane_ok(src, rows, cols, 1, stride), "micv_mean_stddev_u8: bad argument (rows * cols < 2^31)");
    MICV_HIP(hipSetDevice(ctx->device));
    const long long n = (long long)rows * cols;
    const unsigned grid = grid_for(n);
    void *scratch;
    MICV_TRY(ctx->reserve(grid * sizeof(Part), &scratch));
    hipStream_t s = static_cast<hipStream_t>(stream);
    stats_kernel<<<grid, kT, 0, s>>>(src, stride, 1, rows, cols, static_cast<Part *>(scratch), nullptr, 0, nullptr, nullptr, 0);
    MICV_LAUNCH_CHECK();
    stats_finish_kernel<<<1, kT, 0, s>>>(static_cast<const Part *>(scratch), (int)grid, n, stats);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_mean_stddev_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride, micv_ps0_stats *stats) {
    MICV_REQUIRE(ctx && stats && plane_ok(src, rows, cols, 1, stride), "micv_mean_stddev_u8_host: bad argument (rows * cols < 2^31)");
    HostCall h(ctx, "micv_mean_stddev_u8_host");
    uint8_t *s = h.up<uint8_t>(src, stride, (size_t)cols, rows);
    micv_ps0_stats *d = h.alloc<micv_ps0_stats>(sizeof(micv_ps0_stats));
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mean_stddev_u8_dev(ctx, s, rows, cols, (size_t)cols, d, h.s));
    h.down(stats, d, sizeof(micv_ps0_stats));
    return h.finish();
}

int micv_ps0_arithmetic_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, const double *mean_stddev, uint8_t *dst,
                               size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && mean_stddev && plane_ok(src, rows, cols, 1, sstride) && plane_ok(dst, rows, cols, 1, dstride),
                 "micv_ps0_arithmetic_u8: bad argument");
    MICV_HIP(hipSetDevice(ctx->device));
    arith_kernel<<<grid_for((long long)rows * cols), kT, 0, static_cast<hipStream_t>(stream)>>>(src, sstride, rows, cols, mean_stddev, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_ps0_arithmetic_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, double mean, double stddev, uint8_t *dst,
                                size_t dstride) {
    MICV_REQUIRE(ctx && plane_ok(src, rows, cols, 1, sstride) && plane_ok(dst, rows, cols, 1, dstride), "micv_ps0_arithmetic_u8_host: bad argument");
    HostCall h(ctx, "micv_ps0_arithmetic_u8_host");
    const double ms[2] = {mean, stddev};
    uint8_t *s = h.up<uint8_t>(src, sstride, (size_t)cols, rows), *d = h.alloc<uint8_t>((size_t)cols * rows);
    double *m = h.up<double>(ms, 16);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_ps0_arithmetic_u8_dev(ctx, s, rows, cols, (size_t)cols, m, d, (size_t)cols, h.s));
    h.down(dst, dstride, d, (size_t)cols, rows);
    return h.finish();
}

int micv_subtract_sat_u8_dev(micv_ctx *ctx, const uint8_t *a, size_t astride, const uint8_t *b, size_t bstride, int rows, int cols, uint8_t *dst,
                             size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && plane_ok(a, rows, cols, 1, astride) && plane_ok(b, rows, cols, 1, bstride) && plane_ok(dst, rows, cols, 1, dstride),
                 "micv_subtract_sat_u8: bad argument");
    MICV_HIP(hipSetDevice(ctx->device));
    subtract_kernel<<<grid_for((long long)rows * cols), kT, 0, static_cast<hipStream_t>(stream)>>>(a, astride, b, bstride, rows, cols, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_subtract_sat_u8_host(micv_ctx *ctx, const uint8_t *a, size_t astride, const uint8_t *b, size_t bstride, int rows, int cols, uint8_t *dst,
                              size_t dstride) {
    MICV_REQUIRE(ctx && plane_ok(a, rows, cols, 1, astride) && plane_ok(b, rows, cols, 1, bstride) && plane_ok(dst, rows, cols, 1, dstride),
                 "micv_subtract_sat_u8_host: bad argument");
    HostCall h(ctx, "micv_subtract_sat_u8_host");
    const size_t rb = (size_t)cols;
    uint8_t *da = h.up<uint8_t>(a, astride, rb, rows), *db = h.up<uint8_t>(b, bstride, rb, rows), *d = h.alloc<uint8_t>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_subtract_sat_u8_dev(ctx, da, rb, db, rb, rows, cols, d, rb, h.s));
    h.down(dst, dstride, d, rb, rows);
    return h.finish();
}

int micv_add_noise_s8_u8_dev(micv_ctx *ctx, const uint8_t *src, size_t sstride, const float *noise, size_t nstride, int rows, int cols,
                             uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && plane_ok(src, rows, cols, 1, sstride) && plane_ok(noise, rows, cols, 4, nstride) && nstride % 4 == 0 &&
                     plane_ok(dst, rows, cols, 1, dstride),
                 "micv_add_noise_s8_u8: bad argument");
    MICV_HIP(hipSetDevice(ctx->device));
    noise_kernel<<<grid_for((long long)rows * cols), kT, 0, static_cast<hipStream_t>(stream)>>>(src, sstride, noise, nstride, rows, cols, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_add_noise_s8_u8_host(micv_ctx *ctx, const uint8_t *src, size_t sstride, const float *noise, size_t nstride, int rows, int cols,
                              uint8_t *dst, size_t dstride) {
    MICV_REQUIRE(ctx && plane_ok(src, rows, cols, 1, sstride) && plane_ok(noise, rows, cols, 4, nstride) && plane_ok(dst, rows, cols, 1, dstride),
                 "micv_add_noise_s8_u8_host: bad argument");
    HostCall h(ctx, "micv_add_noise_s8_u8_host");
    const size_t rb = (size_t)cols;
    uint8_t *s = h.up<uint8_t>(src, sstride, rb, rows), *d = h.alloc<uint8_t>(rb * rows);
    float *z = h.up<float>(noise, nstride, rb * 4, rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_add_noise_s8_u8_dev(ctx, s, rb, z, rb * 4, rows, cols, d, rb, h.s));
    h.down(dst, dstride, d, rb, rows);
    return h.finish();
}

int micv_ps0_run_dev(micv_ctx *ctx, const uint8_t *image1, int rows1, int cols1, size_t stride1, const uint8_t *image2, int rows2, int cols2,
                     size_t stride2, int size, const float *noise_green, const float *noise_blue, size_t nstride, uint8_t *swapped,
                     size_t wstride, uint8_t *planes, size_t pstride, size_t plane_pitch, uint8_t *replaced, size_t rstride,
                     micv_ps0_stats *stats, micv_stream stream) {
    MICV_REQUIRE(ctx && stats && plane_ok(image1, rows1, cols1, 3, stride1) && plane_ok(image2, rows2, cols2, 3, stride2) &&
                     plane_ok(noise_green, rows1, cols1, 4, nstride) && plane_ok(noise_blue, rows1, cols1, 4, nstride) && nstride % 4 == 0 &&
                     plane_ok(swapped, rows1, cols1, 3, wstride) && plane_ok(planes, rows1, cols1, 1, pstride) &&
                     plane_pitch >= pstride * (size_t)rows1 && plane_ok(replaced, rows2, cols2, 1, rstride),
                 "micv_ps0_run: bad argument");
    Paste ps{};
    MICV_REQUIRE(squares(rows1, cols1, rows2, cols2, size, &ps), "micv_ps0_run: the %d x %d square leaves %dx%d or %dx%d", size, size, rows1, cols1,
                 rows2, cols2);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long n = (long long)rows1 * cols1;
    const unsigned grid = grid_for(n);
    void *scratch;
    MICV_TRY(ctx->reserve(grid * sizeof(Part), &scratch));
    uint8_t *green = planes, *red = planes + plane_pitch;
    stats_kernel<<<grid, kT, 0, s>>>(image1, stride1, 3, rows1, cols1, static_cast<Part *>(scratch), swapped, wstride, green, red, pstride);
    MICV_LAUNCH_CHECK();
    ps.a = image1 + 2, ps.b = image2 + 2, ps.dst = replaced, ps.astride = stride1, ps.bstride = stride2, ps.dstride = rstride;
    ps.apx = ps.bpx = 3, ps.cn = 1, ps.rows = rows2, ps.cols = cols2;
    paste_kernel<<<grid_for((long long)rows2 * cols2), kT, 0, s>>>(ps);
    MICV_LAUNCH_CHECK();
    Pass2 p{};
    p.parts = static_cast<const Part *>(scratch), p.nparts = (int)grid, p.rows = rows1, p.cols = cols1, p.img1 = image1, p.s1 = stride1;
    p.green = green, p.ng = noise_green, p.nb = noise_blue, p.nstride = nstride, p.pstride = pstride;
    p.arith = planes + 2 * plane_pitch, p.trans = planes + 3 * plane_pitch, p.diff = planes + 4 * plane_pitch;
    p.noisy_g = planes + 5 * plane_pitch, p.noisy_b = planes + 6 * plane_pitch, p.stats = stats;
    pass2_kernel<<<grid, kT, 0, s>>>(p);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_ps0_run_host(micv_ctx *ctx, const uint8_t *image1, int rows1, int cols1, size_t stride1, const uint8_t *image2, int rows2, int cols2,
                      size_t stride2, int size, uint64_t *rng_state, float noise_mean, float noise_sigma, uint8_t *swapped, size_t wstride,
                      uint8_t *planes, size_t pstride, size_t plane_pitch, uint8_t *replaced, size_t rstride, micv_ps0_stats *stats) {
    MICV_REQUIRE(ctx && rng_state && stats && plane_ok(image1, rows1, cols1, 3, stride1) && plane_ok(image2, rows2, cols2, 3, stride2) &&
                     plane_ok(swapped, rows1, cols1, 3, wstride) && plane_ok(planes, rows1, cols1, 1, pstride) &&
                     plane_pitch >= pstride * (size_t)rows1 && plane_ok(replaced, rows2, cols2, 1, rstride),
                 "micv_ps0_run_host: bad argument");
    Paste q{};
    MICV_REQUIRE(squares(rows1, cols1, rows2, cols2, size, &q), "micv_ps0_run_host: the %d x %d square leaves an image", size, size);
    std::vector<float> noise(2 * (size_t)rows1 * cols1);  // green's plane, then blue's, one generator
    const size_t n = (size_t)rows1 * cols1, rb = (size_t)cols1;
    MICV_TRY(micv_cv_randn_f32_host(rng_state, noise_mean, noise_sigma, rows1, cols1, noise.data(), rb * 4));
    MICV_TRY(micv_cv_randn_f32_host(rng_state, noise_mean, noise_sigma, rows1, cols1, noise.data() + n, rb * 4));
    HostCall h(ctx, "micv_ps0_run_host");
    uint8_t *d1 = h.up<uint8_t>(image1, stride1, rb * 3, rows1), *d2 = h.up<uint8_t>(image2, stride2, (size_t)cols2 * 3, rows2);
    float *dn = h.up<float>(noise.data(), 2 * n * 4);
    uint8_t *dw = h.alloc<uint8_t>(3 * n), *dp = h.alloc<uint8_t>(7 * n), *dr = h.alloc<uint8_t>((size_t)rows2 * cols2);
    micv_ps0_stats *ds = h.alloc<micv_ps0_stats>(sizeof(micv_ps0_stats));
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_ps0_run_dev(ctx, d1, rows1, cols1, rb * 3, d2, rows2, cols2, (size_t)cols2 * 3, size, dn, dn + n, rb * 4, dw, rb * 3, dp, rb,
                              n, dr, (size_t)cols2, ds, h.s));
    h.down(swapped, wstride, dw, rb * 3, rows1);
    for (int k = 0; k < 7; k++) h.down(planes + k * plane_pitch, pstride, dp + k * n, rb, rows1);
    h.down(replaced, rstride, dr, (size_t)cols2, rows2);
    h.down(stats, ds, sizeof(micv_ps0_stats));
    return h.finish();
}

}  // extern "C"
