// moments.hip -- ps7 moments::centralMoment (ps7_cpp/lib/Moments.cpp) for a batch of single-channel images.
//
// The arithmetic contract is in include/mi_cv.h ("ps7: central moments") and DESIGN.md section 2.  Every sum is
// exact, then rounded once to double and once to f32 (exact_sum.hpp), so no result depends on the grid or the
// schedule.  Launches, all on the caller's stream, none of them with a host sync:
//   moments_max_kernel        (MICV_MOMENTS_NORM_INF only) per-workgroup u8 maxima
//   moments_pass_kernel<0>    per-workgroup bins of M00, M10, M01 (the workgroup first folds the maxima into the
//                             cv::normalize scale when NORM_INF is set)
//   moments_finish_kernel<0>  one workgroup per image: raw[] and the centroid
//   moments_pass_kernel<1>    per-workgroup bins of every requested (p, q)
//   moments_finish_kernel<1>  one workgroup per image: mu and eta
// A workgroup owns 4096 consecutive pixels of one image (16 per lane), keeps their values and coordinates in
// registers and runs one sum at a time over them.  A lane adds its term into its own slot of an LDS bin array
// (bins x lanes, int64) -- no two lanes share a slot, so the adds are plain integer accumulation, exact and
// order-independent -- then the workgroup folds the 256 slots of each bin and writes 16 int64 + flags per sum.
// No float atomics, no global atomics.
#include <cmath>

#include "common.hpp"
#include "exact_sum.hpp"

namespace micv {

namespace {

constexpr int kMomThreads = 256, kMomPix = 16, kMomChunk = kMomThreads * kMomPix;
constexpr int kPartWords = kSumBins + 1;  // 16 bins + the flags word, per (image, sum, workgroup)

struct MomOrders {
    int p[MICV_MOMENTS_MAX_ORDERS], q[MICV_MOMENTS_MAX_ORDERS];
    int n;
};

struct MomImg {
    const uint8_t *base;
    size_t pitch, stride;  // bytes between images / rows
    int rows, cols, f32;
};

__device__ __forceinline__ float load_px(const MomImg &im, int b, int r, int c) {
    const uint8_t *row = im.base + (size_t)b * im.pitch + (size_t)r * im.stride;
    return im.f32 ? reinterpret_cast<const float *>(row)[c] : (float)row[c];
}

// cv::pow(src, p, dst) on f32 with an integer power (mi_cv.h: powers)
__device__ __forceinline__ float ipow_cv(float d, int p) {
    if (p == 0) return 1.f;
    if (p == 1) return d;
    float a = 1.f, b = d;
    while (p > 1) {
        if (p & 1) a *= b;
        b *= b;
        p >>= 1;
    }
    return a * b;
}

__global__ __launch_bounds__(kMomThreads) void moments_max_kernel(MomImg im, unsigned *__restrict__ pmax, int nwg) {
    const int b = blockIdx.y, wg = blockIdx.x;
    const int npix = im.rows * im.cols;
    unsigned m = 0;
    for (int k = 0; k < kMomPix; k++) {
        const int i = wg * kMomChunk + k * kMomThreads + threadIdx.x;
        if (i < npix) {
            const int r = i / im.cols, c = i - r * im.cols;
            const unsigned v = im.base[(size_t)b * im.pitch + (size_t)r * im.stride + c];
            m = v > m ? v : m;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_xor(m, o, 64);
        m = t > m ? t : m;
    }
    __shared__ unsigned wm[kMomThreads / 64];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMomThreads / 64; w++) m = wm[w] > m ? wm[w] : m;
        pmax[(size_t)b * nwg + wg] = m;
    }
}

// Folds the 256 lane slots of every bin and writes this workgroup's partial; ends with the LDS free again.
__device__ __forceinline__ void flush_sum(long long (*acc)[kMomThreads], unsigned flags, long long *__restrict__ out) {
    __shared__ unsigned wflags[kMomThreads / 64];
    const unsigned long long nan = __ballot((flags & kSumNaN) != 0), pinf = __ballot((flags & kSumPosInf) != 0),
                             ninf = __ballot((flags & kSumNegInf) != 0);
    if ((threadIdx.x & 63) == 0)
        wflags[threadIdx.x >> 6] = (nan ? kSumNaN : 0u) | (pinf ? kSumPosInf : 0u) | (ninf ? kSumNegInf : 0u);
    __syncthreads();
    const int bin = threadIdx.x >> 4, part = threadIdx.x & 15;
    long long s = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) s += acc[bin][part * 16 + j];
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    if (part == 0) out[bin] = s;
    if (threadIdx.x == 0) {
        unsigned f = 0;
        for (int w = 0; w < kMomThreads / 64; w++) f |= wflags[w];
        out[kSumBins] = (long long)f;
    }
    __syncthreads();
}

__device__ __forceinline__ void add_term(long long (*acc)[kMomThreads], float t, unsigned &flags) {
    int bin;
    long long v;
    split_term(t, bin, v, flags);
    if (v != 0) __hip_atomic_fetch_add(&acc[bin][threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// PASS 0: M00, M10, M01.  PASS 1: the central terms of every order.
// part: [image][sum][workgroup][kPartWords]; cent: [image][8] = M00, M10, M01, xbar, ybar (pass 0's finish).
template <int PASS>
__global__ __launch_bounds__(kMomThreads) void moments_pass_kernel(MomImg im, int nwg, const unsigned *__restrict__ pmax,
                                                                    const float *__restrict__ cent, MomOrders ord,
                                                                    int y_fixed, long long *__restrict__ part) {
    __shared__ long long acc[kSumBins][kMomThreads];
    __shared__ float s_scale;
    const int b = blockIdx.y, wg = blockIdx.x, tid = threadIdx.x;
    const int npix = im.rows * im.cols;
    if (pmax) {  // cv::normalize(.., 1.0, 0.0, NORM_INF, CV_32FC1): scale = max > DBL_EPSILON ? 1.0 / max : 0
        unsigned m = 0;
        for (int i = tid; i < nwg; i += kMomThreads) {
            const unsigned v = pmax[(size_t)b * nwg + i];
            m = v > m ? v : m;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned t = __shfl_xor(m, o, 64);
            m = t > m ? t : m;
        }
        __shared__ unsigned wm[kMomThreads / 64];
        if ((tid & 63) == 0) wm[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kMomThreads / 64; w++) m = wm[w] > m ? wm[w] : m;
            s_scale = m ? (float)(1.0 / (double)m) : 0.f;
        }
        __syncthreads();
    }
    const float scale = pmax ? s_scale : 1.f;
    float v[kMomPix], xs[kMomPix], ys[kMomPix];
    bool in[kMomPix];
#pragma unroll
    for (int k = 0; k < kMomPix; k++) {
        const int i = wg * kMomChunk + k * kMomThreads + tid;
        in[k] = i < npix;
        const int r = in[k] ? i / im.cols : 0, c = in[k] ? i - r * im.cols : 0;
        const float raw = in[k] ? load_px(im, b, r, c) : 0.f;
        v[k] = pmax ? raw * scale : raw;  // (u8 only) fl(v * s)
        xs[k] = (float)c;
        ys[k] = (float)r;
    }
    const int nsum = PASS == 0 ? 3 : ord.n;
    float xbar = 0.f, ybar = 0.f;
    if (PASS == 1) {
        xbar = cent[(size_t)b * 8 + 3];
        ybar = cent[(size_t)b * 8 + 4];
    }
    for (int j = 0; j < nsum; j++) {
#pragma unroll
        for (int k = 0; k < kSumBins; k++) acc[k][tid] = 0;  // (own slots only: no barrier needed)
        unsigned flags = 0;
        int p = 0, q = 0;
        if (PASS == 1) {
            p = ord.p[j];
            q = ord.q[j];
        }
#pragma unroll
        for (int k = 0; k < kMomPix; k++) {
            if (!in[k]) continue;
            float t;
            if (PASS == 0) {
                t = j == 0 ? v[k] : (j == 1 ? xs[k] * v[k] : ys[k] * v[k]);
            } else {
                const float dx = xs[k] - xbar;
                const float dy = (y_fixed ? ys[k] : xs[k]) - ybar;  // Moments.cpp:59 uses xFull - yBar
                const float xp = ipow_cv(dx, p), yq = ipow_cv(dy, q);
                t = yq * (xp * v[k]);
            }
            add_term(acc, t, flags);
        }
        flush_sum(acc, flags, part + (((size_t)b * nsum + j) * nwg + wg) * kPartWords);
    }
}

// Sums the workgroup partials of one (image, sum) into `bins` / `flags` (thread 0 holds the result).
__device__ __forceinline__ float finish_one(const long long *__restrict__ part, int nwg) {
    __shared__ long long fold[kMomThreads];
    __shared__ unsigned fflags[kMomThreads / 64];
    __shared__ float result;
    const int tid = threadIdx.x, bin = tid & 15;
    long long s = 0;
    unsigned f = 0;
    for (int w = tid >> 4; w < nwg; w += kMomThreads / 16) {
        s += part[(size_t)w * kPartWords + bin];
        if (bin == 0) f |= (unsigned)part[(size_t)w * kPartWords + kSumBins];
    }
    fold[tid] = s;
    const unsigned long long a = __ballot((f & kSumNaN) != 0), bb = __ballot((f & kSumPosInf) != 0),
                             c = __ballot((f & kSumNegInf) != 0);
    if ((tid & 63) == 0) fflags[tid >> 6] = (a ? kSumNaN : 0u) | (bb ? kSumPosInf : 0u) | (c ? kSumNegInf : 0u);
    __syncthreads();
    if (tid == 0) {
        long long bins[kSumBins];
        for (int k = 0; k < kSumBins; k++) {
            long long t = 0;
            for (int g = 0; g < kMomThreads / 16; g++) t += fold[g * 16 + k];
            bins[k] = t;
        }
        unsigned fl = 0;
        for (int w = 0; w < kMomThreads / 64; w++) fl |= fflags[w];
        result = finish_sum(bins, fl);
    }
    __syncthreads();
    const float r = result;
    __syncthreads();
    return r;
}

__device__ __forceinline__ float canon(float v) { return v != v ? __builtin_bit_cast(float, 0x7FC00000u) : v; }

// pow(M00, 1 + (p+q)/2) from IEEE basic operations only (mi_cv.h): left-to-right product, times sqrt for a half.
__host__ __device__ inline double eta_denominator(float m00, int pq) {
    const double d = (double)m00;
    const int whole = 1 + pq / 2;
    double P = d;
    for (int i = 1; i < whole; i++) P = P * d;
    if (pq & 1) P = P * sqrt(d);
    return P;
}

template <int PASS>
__global__ __launch_bounds__(kMomThreads) void moments_finish_kernel(const long long *__restrict__ part, int nwg,
                                                                      MomOrders ord, float *__restrict__ cent,
                                                                      float *__restrict__ raw, float *__restrict__ mu,
                                                                      float *__restrict__ eta) {
    const int b = blockIdx.x;
    const int nsum = PASS == 0 ? 3 : ord.n;
    if (PASS == 0) {
        float m[3];
        for (int j = 0; j < 3; j++) m[j] = finish_one(part + ((size_t)b * 3 + j) * nwg * kPartWords, nwg);
        if (threadIdx.x == 0) {
            float *c = cent + (size_t)b * 8;
            c[0] = m[0];
            c[1] = m[1];
            c[2] = m[2];
            c[3] = m[1] / m[0];  // xBar = M10 / M00 (Moments.cpp:49), f32, correctly rounded
            c[4] = m[2] / m[0];
            if (raw)
                for (int j = 0; j < 3; j++) raw[(size_t)b * 3 + j] = m[j];
        }
    } else {
        const float m00 = cent[(size_t)b * 8];
        for (int j = 0; j < nsum; j++) {
            const float u = finish_one(part + ((size_t)b * nsum + j) * nwg * kPartWords, nwg);
            if (threadIdx.x == 0) {
                mu[(size_t)b * nsum + j] = u;
                eta[(size_t)b * nsum + j] = canon((float)((double)u / eta_denominator(m00, ord.p[j] + ord.q[j])));
            }
        }
    }
}

}  // namespace

}  // namespace micv

using namespace micv;

extern "C" {

int micv_central_moments_dev(micv_ctx *ctx, const void *imgs, int batch, size_t img_pitch, size_t stride, int rows,
                             int cols, int type, const int *orders, int n, uint32_t flags, float *mu, float *eta,
                             float *raw, micv_stream stream) {
    MICV_REQUIRE(ctx && imgs && orders && mu && eta, "micv_central_moments: null argument");
    MICV_REQUIRE(type == MICV_MOMENTS_U8 || type == MICV_MOMENTS_F32, "micv_central_moments: unknown type %d", type);
    const size_t elem = type == MICV_MOMENTS_F32 ? 4 : 1;
    MICV_REQUIRE(batch > 0 && rows > 0 && cols > 0, "micv_central_moments: empty batch or image");
    MICV_REQUIRE((uint64_t)rows * (uint64_t)cols <= kMaxExactTerms,
                 "micv_central_moments: %d x %d exceeds the %llu-pixel limit of the exact sums", rows, cols,
                 (unsigned long long)kMaxExactTerms);
    MICV_REQUIRE(stride % elem == 0 && stride >= (size_t)cols * elem, "micv_central_moments: bad row stride");
    MICV_REQUIRE(batch == 1 || img_pitch >= stride * (size_t)rows, "micv_central_moments: image pitch below rows * stride");
    MICV_REQUIRE((uintptr_t)imgs % elem == 0 && (batch == 1 || img_pitch % elem == 0),
                 "micv_central_moments: misaligned f32 images");
    MICV_REQUIRE(n >= 1 && n <= MICV_MOMENTS_MAX_ORDERS, "micv_central_moments: %d orders (1..%d)", n,
                 MICV_MOMENTS_MAX_ORDERS);
    MICV_REQUIRE((flags & ~(uint32_t)(MICV_MOMENTS_NORM_INF | MICV_MOMENTS_Y_FIXED)) == 0,
                 "micv_central_moments: unknown flags %#x", flags);
    MICV_REQUIRE(!(flags & MICV_MOMENTS_NORM_INF) || type == MICV_MOMENTS_U8,
                 "micv_central_moments: MICV_MOMENTS_NORM_INF needs u8 input");
    MomOrders ord{};
    ord.n = n;
    for (int j = 0; j < n; j++) {
        const int p = orders[2 * j], q = orders[2 * j + 1];
        MICV_REQUIRE(p >= 0 && q >= 0 && p + q <= MICV_MOMENTS_MAX_ORDER,
                     "micv_central_moments: order (%d, %d) outside p, q >= 0, p + q <= %d", p, q, MICV_MOMENTS_MAX_ORDER);
        ord.p[j] = p;
        ord.q[j] = q;
    }
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nwg = (int)cdiv((unsigned)(rows * cols), kMomChunk);
    const bool norm = flags & MICV_MOMENTS_NORM_INF;
    const size_t need = Carver::need((size_t)batch * nwg, 4) + Carver::need((size_t)batch * 8, 4) +
                        Carver::need((size_t)batch * 3 * nwg * kPartWords, 8) +
                        Carver::need((size_t)batch * n * nwg * kPartWords, 8);
    void *scratch;
    MICV_TRY(ctx->reserve(need, &scratch));
    Carver cv(scratch);
    unsigned *pmax = cv.take<unsigned>((size_t)batch * nwg);
    float *cent = cv.take<float>((size_t)batch * 8);
    long long *part1 = cv.take<long long>((size_t)batch * 3 * nwg * kPartWords);
    long long *part2 = cv.take<long long>((size_t)batch * n * nwg * kPartWords);
    const MomImg im{static_cast<const uint8_t *>(imgs), img_pitch, stride, rows, cols, type == MICV_MOMENTS_F32};
    const dim3 grid(nwg, batch);
    if (norm) {
        moments_max_kernel<<<grid, kMomThreads, 0, s>>>(im, pmax, nwg);
        MICV_LAUNCH_CHECK();
    }
    moments_pass_kernel<0><<<grid, kMomThreads, 0, s>>>(im, nwg, norm ? pmax : nullptr, cent, ord, 0, part1);
    MICV_LAUNCH_CHECK();
    moments_finish_kernel<0><<<batch, kMomThreads, 0, s>>>(part1, nwg, ord, cent, raw, nullptr, nullptr);
    MICV_LAUNCH_CHECK();
    moments_pass_kernel<1><<<grid, kMomThreads, 0, s>>>(im, nwg, norm ? pmax : nullptr, cent, ord,
                                                         (flags & MICV_MOMENTS_Y_FIXED) ? 1 : 0, part2);
    MICV_LAUNCH_CHECK();
    moments_finish_kernel<1><<<batch, kMomThreads, 0, s>>>(part2, nwg, ord, cent, nullptr, mu, eta);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // extern "C"
