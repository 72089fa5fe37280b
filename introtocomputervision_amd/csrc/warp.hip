// warp.hip -- ps4 registration on the device: the tail of Solution::runProblem3
// (ps4_cpp/src/Solution.cpp:315-325 and :344-354): cv::invertAffineTransform, cv::warpAffine
// (INTER_LINEAR or INTER_NEAREST, BORDER_CONSTANT 0) and the 0.5 / 0.5 blend (cv::addWeighted), for
// single-channel u8 and f32 images.  The contract is in include/mi_cv.h ("ps4: registration") and
// DESIGN.md section 2; tests/_warp_ref.py restates it in numpy.
//
// One kernel does every warp.  A lane produces four adjacent destination pixels of one row and
// stores them as one dword (u8) or one dwordx4 (f32) where the destination is aligned for it; a
// 256-thread workgroup covers 128 x 8 pixels and blockIdx.z counts the images of a batch.  The
// transform is read from DEVICE memory (micv_ransac_solve_*_dev's `transforms` goes straight in)
// and every lane inverts it for itself in double: the lanes of a wave do that in the same
// instructions, so sharing it through LDS would save nothing but the other three waves' copies and
// cost a barrier.  The row terms X0 / Y0 and the column terms adelta / bdelta are cvRound's of
// doubles, formed once per lane; everything else per pixel is int32.  A pixel's bits depend on its
// coordinates, the transform and the source only -- not on the grid.  Source taps come through the
// vector cache, the two taps of a source row as one two-element load (load_pair; nothing outside the
// image is addressed): the kernel is bound by the number of tap loads, not by bytes or arithmetic, and
// halving them took 4K from 44 to 27 us, while four rows per lane (the column terms formed once for
// four pixels) changed nothing, and staging source tiles in LDS was not built (profiles/ps4_warp/README.md).
// The blend form (micv_register_blend) applies cv::addWeighted to the warped pixel in registers.
// -ffp-contract=off: no fused multiply-add anywhere here.
#include <climits>

#include "common.hpp"

namespace micv {
namespace {

constexpr int kTileW = 128, kTileH = 8;  // 32 lanes x 4 pixels, 8 rows
constexpr int kMaxDim = 32767;           // the int16 cell of cv::remap

// cvRound(double) as x86's cvtsd2si gives it: ties to even; NaN or a ROUNDED value outside int32 is INT_MIN
// (the float form is cv_round_i32 of lk_device.hpp; a double can lie between INT_MAX and 2^31, so the range test is
// made on the rounded value).
__device__ __forceinline__ int cv_round_f64(double v) {
    const double r = rint(v);
    return (r >= -2147483648.0 && r < 2147483648.0) ? (int)r : INT_MIN;
}
__device__ __forceinline__ int cv_round_f32(float v) {
    const int r = __float2int_rn(v);
    return fabsf(v) < 2147483648.f ? r : INT_MIN;
}
__device__ __forceinline__ int wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

// cv::invertAffineTransform on a CV_32F 2x3: double arithmetic on the float entries, unfused.
__device__ __forceinline__ void invert_affine_f64(const float *m, double *o) {
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    double D = m0 * m4 - m1 * m3;
    D = D != 0 ? 1. / D : 0;
    const double A11 = m4 * D, A22 = m0 * D, A12 = -m1 * D, A21 = -m3 * D;
    const double b1 = -A11 * m2 - A12 * m5, b2 = -A21 * m2 - A22 * m5;
    o[0] = A11; o[1] = A12; o[2] = b1;
    o[3] = A21; o[4] = A22; o[5] = b2;
}

// The matrix cv::warpAffine walks: M widened to double and, without WARP_INVERSE_MAP, inverted in place.
__device__ __forceinline__ void warp_matrix(const float *m, bool inverse_map, double *M) {
    for (int i = 0; i < 6; i++) M[i] = m[i];
    if (inverse_map) return;
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D;
    M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
}

// cv::addWeighted for one pixel: (a * alpha + b * beta) + gamma in float, unfused.
__device__ __forceinline__ float weighted(float a, float alpha, float b, float beta, float gamma) {
    float t = a * alpha + b * beta;
    t = t + gamma;
    return t;
}
__device__ __forceinline__ uint8_t store_as(float t, uint8_t) { return (uint8_t)clampi(cv_round_f32(t), 0, 255); }
__device__ __forceinline__ float store_as(float t, float) { return t; }

template <typename T>
struct Vec4;
template <>
struct Vec4<uint8_t> {
    using type = uchar4;
};
template <>
struct Vec4<float> {
    using type = float4;
};

template <typename T>
__device__ __forceinline__ void store4(T *p, const T *v, int n, bool vec) {
    if (vec && n == 4) {
        typename Vec4<T>::type q;
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<typename Vec4<T>::type *>(p) = q;
    } else {
        for (int i = 0; i < 4; i++)
            if (i < n) p[i] = v[i];
    }
}
template <typename T>
__device__ __forceinline__ void load4(const T *p, T *v, int n, bool vec) {
    if (vec && n == 4) {
        const typename Vec4<T>::type q = *reinterpret_cast<const typename Vec4<T>::type *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int i = 0; i < 4; i++) v[i] = i < n ? p[i] : T(0);
    }
}

struct WarpArgs {
    const void *src;          // image z at src + z * src_pitch bytes (pitch 0: one shared source)
    size_t src_pitch;
    int srows, scols, sstride;  // stride in elements
    const float *m;           // transform z at m + 6 z
    void *dst;                // image z at dst + z * dst_pitch bytes
    size_t dst_pitch;
    int drows, dcols, dstride;
    int inverse_map;          // MICV_WARP_INVERSE_MAP
    int pre_invert;           // register_blend: cv::invertAffineTransform (rounded to float) first
    int vec;                  // destination (and `a`, `warped`) aligned for 4-pixel stores
    // blend form only
    const void *a;
    int astride;
    void *warped;             // optional
    int wstride;
};

// The two taps (sx, sy') and (sx + 1, sy') of one source row as ONE load of two adjacent elements at the column clamped
// into [0, cols - 2] (always inside the row; u8: two bytes at any address, f32: 8 bytes at a 4-byte boundary), then
// sorted into place: the pair sits at sx (both taps inside), one column to its right (sx = -1: the left tap is
// outside) or to its left (sx = cols - 1: the right one is); anything else is outside altogether.  Half the tap
// loads of the four separate ones; needs cols >= 2.
template <typename T>
struct Pair {
    T lo, hi;
};
template <typename T>
__device__ __forceinline__ void load_pair(const T *__restrict__ row, int sx, int cols, bool row_ok, T &v0, T &v1) {
    const int xa = clampi(sx, 0, cols - 2), d = sx - xa;
    Pair<T> q{T(0), T(0)};
    if (row_ok && d >= -1 && d <= 1) __builtin_memcpy(&q, row + xa, sizeof(q));
    v0 = d == 0 ? q.lo : (d == 1 ? q.hi : T(0));
    v1 = d == 0 ? q.hi : (d == -1 ? q.lo : T(0));
}

template <typename T, bool NEAREST, bool BLEND>
__global__ __launch_bounds__(256) void warp_affine_kernel(const WarpArgs g) {
    const int lane_x = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = blockIdx.x * kTileW + lane_x * 4, y = blockIdx.y * kTileH + ty;
    if (x0 >= g.dcols || y >= g.drows) return;
    const int z = blockIdx.z;
    const T *__restrict__ src = reinterpret_cast<const T *>(static_cast<const char *>(g.src) + (size_t)z * g.src_pitch);
    T *__restrict__ dst = reinterpret_cast<T *>(static_cast<char *>(g.dst) + (size_t)z * g.dst_pitch);

    float mf[6];
    for (int i = 0; i < 6; i++) mf[i] = g.m[6 * z + i];
    if (g.pre_invert) {
        double inv[6];
        invert_affine_f64(mf, inv);
        for (int i = 0; i < 6; i++) mf[i] = (float)inv[i];
    }
    double M[6];
    warp_matrix(mf, g.inverse_map != 0, M);

    constexpr int kDelta = NEAREST ? 512 : 16, kShift = NEAREST ? 10 : 5;
    const int n = min(4, g.dcols - x0);
    const bool pairs = g.scols >= 2;
    const int X0 = wrap_add(cv_round_f64((M[1] * y + M[2]) * 1024), kDelta);
    const int Y0 = wrap_add(cv_round_f64((M[4] * y + M[5]) * 1024), kDelta);
    T out[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = x0 + i;
        const int X = wrap_add(X0, cv_round_f64(M[0] * x * 1024)) >> kShift;
        const int Y = wrap_add(Y0, cv_round_f64(M[3] * x * 1024)) >> kShift;
        if constexpr (NEAREST) {
            const int sx = clampi(X, -32768, 32767), sy = clampi(Y, -32768, 32767);
            const bool in = (unsigned)sx < (unsigned)g.scols && (unsigned)sy < (unsigned)g.srows;
            out[i] = in ? src[(ptrdiff_t)sy * g.sstride + sx] : T(0);
        } else {
            const int sx = clampi(X >> 5, -32768, 32767), sy = clampi(Y >> 5, -32768, 32767);
            const int fx = X & 31, fy = Y & 31;
            const bool by0 = (unsigned)sy < (unsigned)g.srows, by1 = (unsigned)(sy + 1) < (unsigned)g.srows;
            T v0, v1, v2, v3;
            if (pairs) {
                const T *row = src + (ptrdiff_t)sy * g.sstride;
                load_pair(row, sx, g.scols, by0, v0, v1);
                load_pair(row + g.sstride, sx, g.scols, by1, v2, v3);
            } else {
                const bool bx0 = (unsigned)sx < (unsigned)g.scols, bx1 = (unsigned)(sx + 1) < (unsigned)g.scols;
                const T *p = src + (ptrdiff_t)sy * g.sstride + sx;
                v0 = (bx0 && by0) ? p[0] : T(0);
                v1 = (bx1 && by0) ? p[1] : T(0);
                v2 = (bx0 && by1) ? p[g.sstride] : T(0);
                v3 = (bx1 && by1) ? p[g.sstride + 1] : T(0);
            }
            if constexpr (sizeof(T) == 1) {
                // cv::remap's 15-bit table for INTER_LINEAR: exact entries, the four sum to 32768
                const int w0 = (32 - fx) * (32 - fy) * 32, w1 = fx * (32 - fy) * 32, w2 = (32 - fx) * fy * 32,
                          w3 = fx * fy * 32;
                out[i] = (T)((w0 * (int)v0 + w1 * (int)v1 + w2 * (int)v2 + w3 * (int)v3 + 16384) >> 15);
            } else {
                // the blend of warp_sample (lk_device.hpp), restated: tests tie the two together
                const float ax1 = (float)fx * 0.03125f, ax0 = 1.f - ax1;
                const float ay1 = (float)fy * 0.03125f, ay0 = 1.f - ay1;
                float s = v0 * (ay0 * ax0);
                s = s + v1 * (ay0 * ax1);
                s = s + v2 * (ay1 * ax0);
                s = s + v3 * (ay1 * ax1);
                out[i] = s;
            }
        }
    }
    if constexpr (BLEND) {
        if (g.warped) {
            T *w = reinterpret_cast<T *>(g.warped) + (size_t)y * g.wstride + x0;
            store4(w, out, n, g.vec != 0);
        }
        T av[4];
        load4(reinterpret_cast<const T *>(g.a) + (size_t)y * g.astride + x0, av, n, g.vec != 0);
#pragma unroll
        for (int i = 0; i < 4; i++) out[i] = store_as(weighted((float)av[i], 0.5f, (float)out[i], 0.5f, 0.f), T());
    }
    store4(dst + (size_t)y * g.dstride + x0, out, n, g.vec != 0);
}

// One lane per transform.
__global__ __launch_bounds__(64) void invert_affine_kernel(const float *__restrict__ m, int count, float *__restrict__ inv) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    float mf[6];
    for (int k = 0; k < 6; k++) mf[k] = m[6 * (size_t)i + k];
    double o[6];
    invert_affine_f64(mf, o);
    for (int k = 0; k < 6; k++) inv[6 * (size_t)i + k] = (float)o[k];
}

template <typename T>
__global__ __launch_bounds__(256) void add_weighted_kernel(const T *__restrict__ a, int astride, float alpha,
                                                           const T *__restrict__ b, int bstride, float beta, float gamma,
                                                           int rows, int cols, T *__restrict__ dst, int dstride, int vec) {
    const int x0 = (blockIdx.x * 32 + (threadIdx.x & 31)) * 4, y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x0 >= cols || y >= rows) return;
    const int n = min(4, cols - x0);
    T av[4], bv[4], out[4];
    load4(a + (size_t)y * astride + x0, av, n, vec != 0);
    load4(b + (size_t)y * bstride + x0, bv, n, vec != 0);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = store_as(weighted((float)av[i], alpha, (float)bv[i], beta, gamma), T());
    store4(dst + (size_t)y * dstride + x0, out, n, vec != 0);
}

inline bool aligned_for(const void *p, size_t stride_bytes, size_t elem) {
    return p == nullptr || ((reinterpret_cast<uintptr_t>(p) | stride_bytes) % (4 * elem)) == 0;
}
inline size_t elem_of(int depth) { return depth == MICV_DEPTH_8U ? 1 : 4; }
inline bool image_ok(int rows, int cols, size_t stride, size_t elem) {
    return rows > 0 && cols > 0 && rows <= kMaxDim && cols <= kMaxDim && stride_ok(stride, cols, elem);
}

template <typename T, bool BLEND>
int launch_warp_t(hipStream_t s, const WarpArgs &g, int count, bool nearest) {
    const dim3 grid(cdiv(g.dcols, kTileW), cdiv(g.drows, kTileH), count);
    if constexpr (!BLEND) {  // the blend form is always linear
        if (nearest) {
            warp_affine_kernel<T, true, false><<<grid, 256, 0, s>>>(g);
            MICV_LAUNCH_CHECK();
            return MICV_OK;
        }
    }
    warp_affine_kernel<T, false, BLEND><<<grid, 256, 0, s>>>(g);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_invert_affine_dev(micv_ctx *ctx, const float *m, int count, float *inv, micv_stream stream) {
    MICV_REQUIRE(ctx && m && inv, "micv_invert_affine: null argument");
    MICV_REQUIRE(count >= 0, "micv_invert_affine: count %d < 0", count);
    if (count == 0) return MICV_OK;
    MICV_HIP(hipSetDevice(ctx->device));
    invert_affine_kernel<<<cdiv(count, 64), 64, 0, static_cast<hipStream_t>(stream)>>>(m, count, inv);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_warp_affine_batch_dev(micv_ctx *ctx, const void *src, size_t src_pitch_bytes, int depth, int srows, int scols,
                               size_t sstride, const float *m, int count, int flags, void *dst, size_t dst_pitch_bytes,
                               int drows, int dcols, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && m && dst, "micv_warp_affine: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_warp_affine: depth %d is neither 8U nor 32F", depth);
    MICV_REQUIRE(!(flags & ~(MICV_WARP_INVERSE_MAP | MICV_WARP_NEAREST)), "micv_warp_affine: unknown flags 0x%x", flags);
    MICV_REQUIRE(count >= 0, "micv_warp_affine: count %d < 0", count);
    const size_t e = elem_of(depth);
    MICV_REQUIRE(image_ok(srows, scols, sstride, e), "micv_warp_affine: bad source %dx%d (1..%d), stride %zu", srows, scols,
                 kMaxDim, sstride);
    MICV_REQUIRE(image_ok(drows, dcols, dstride, e), "micv_warp_affine: bad destination %dx%d (1..%d), stride %zu", drows,
                 dcols, kMaxDim, dstride);
    MICV_REQUIRE(src != dst, "micv_warp_affine: src and dst must not alias");
    MICV_REQUIRE(src_pitch_bytes % e == 0 && dst_pitch_bytes % e == 0, "micv_warp_affine: image pitch not a multiple of the element");
    MICV_REQUIRE(src_pitch_bytes == 0 || src_pitch_bytes >= (size_t)(srows - 1) * sstride + (size_t)scols * e,
                 "micv_warp_affine: source pitch smaller than an image");
    MICV_REQUIRE(count <= 1 || dst_pitch_bytes >= (size_t)(drows - 1) * dstride + (size_t)dcols * e,
                 "micv_warp_affine: destination pitch smaller than an image");
    if (count == 0) return MICV_OK;
    MICV_HIP(hipSetDevice(ctx->device));
    WarpArgs g{};
    g.src_pitch = src_pitch_bytes;
    g.srows = srows; g.scols = scols; g.sstride = (int)(sstride / e);
    g.dst_pitch = dst_pitch_bytes;
    g.drows = drows; g.dcols = dcols; g.dstride = (int)(dstride / e);
    g.inverse_map = (flags & MICV_WARP_INVERSE_MAP) != 0;
    g.vec = aligned_for(dst, dstride, e) && dst_pitch_bytes % (4 * e) == 0;
    const bool nearest = (flags & MICV_WARP_NEAREST) != 0;
    for (int z0 = 0; z0 < count; z0 += 65535) {  // gridDim.z
        const int nz = count - z0 < 65535 ? count - z0 : 65535;
        g.src = static_cast<const char *>(src) + (size_t)z0 * src_pitch_bytes;
        g.dst = static_cast<char *>(dst) + (size_t)z0 * dst_pitch_bytes;
        g.m = m + 6 * (size_t)z0;
        MICV_TRY(depth == MICV_DEPTH_8U ? (launch_warp_t<uint8_t, false>(static_cast<hipStream_t>(stream), g, nz, nearest))
                                        : (launch_warp_t<float, false>(static_cast<hipStream_t>(stream), g, nz, nearest)));
    }
    return MICV_OK;
}

int micv_warp_affine_dev(micv_ctx *ctx, const void *src, int depth, int srows, int scols, size_t sstride, const float *m,
                         int flags, void *dst, int drows, int dcols, size_t dstride, micv_stream stream) {
    return micv_warp_affine_batch_dev(ctx, src, 0, depth, srows, scols, sstride, m, 1, flags, dst, 0, drows, dcols, dstride,
                                      stream);
}

int micv_add_weighted_dev(micv_ctx *ctx, const void *a, size_t astride, double alpha, const void *b, size_t bstride,
                          double beta, double gamma, int depth, int rows, int cols, void *dst, size_t dstride,
                          micv_stream stream) {
    MICV_REQUIRE(ctx && a && b && dst, "micv_add_weighted: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_add_weighted: depth %d is neither 8U nor 32F", depth);
    const size_t e = elem_of(depth);
    MICV_REQUIRE(image_ok(rows, cols, astride, e) && stride_ok(bstride, cols, e) && stride_ok(dstride, cols, e),
                 "micv_add_weighted: bad size %dx%d (1..%d) or stride", rows, cols, kMaxDim);
    MICV_HIP(hipSetDevice(ctx->device));
    const int vec = aligned_for(a, astride, e) && aligned_for(b, bstride, e) && aligned_for(dst, dstride, e);
    const dim3 grid(cdiv(cols, 128), cdiv(rows, 8));  // 32 lanes x 4 pixels, 8 rows
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (depth == MICV_DEPTH_8U)
        add_weighted_kernel<uint8_t><<<grid, 256, 0, s>>>(static_cast<const uint8_t *>(a), (int)astride, (float)alpha,
                                                          static_cast<const uint8_t *>(b), (int)bstride, (float)beta,
                                                          (float)gamma, rows, cols, static_cast<uint8_t *>(dst), (int)dstride,
                                                          vec);
    else
        add_weighted_kernel<float><<<grid, 256, 0, s>>>(static_cast<const float *>(a), (int)(astride / 4), (float)alpha,
                                                        static_cast<const float *>(b), (int)(bstride / 4), (float)beta,
                                                        (float)gamma, rows, cols, static_cast<float *>(dst), (int)(dstride / 4),
                                                        vec);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_register_blend_dev(micv_ctx *ctx, const void *a, size_t astride, const void *b, size_t bstride, int depth, int rows,
                            int cols, const float *m_a_to_b, void *warped, size_t wstride, void *blended, size_t ostride,
                            micv_stream stream) {
    MICV_REQUIRE(ctx && a && b && m_a_to_b && blended, "micv_register_blend: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_register_blend: depth %d is neither 8U nor 32F", depth);
    const size_t e = elem_of(depth);
    MICV_REQUIRE(image_ok(rows, cols, astride, e) && stride_ok(bstride, cols, e) && stride_ok(ostride, cols, e) &&
                     (!warped || stride_ok(wstride, cols, e)),
                 "micv_register_blend: bad size %dx%d (1..%d) or stride", rows, cols, kMaxDim);
    MICV_REQUIRE(b != blended && b != warped && (!warped || (warped != blended && warped != a)),
                 "micv_register_blend: b, warped and blended must not alias");
    MICV_HIP(hipSetDevice(ctx->device));
    WarpArgs g{};
    g.src = b;
    g.srows = rows; g.scols = cols; g.sstride = (int)(bstride / e);
    g.m = m_a_to_b;
    g.dst = blended;
    g.drows = rows; g.dcols = cols; g.dstride = (int)(ostride / e);
    g.pre_invert = 1;
    g.a = a;
    g.astride = (int)(astride / e);
    g.warped = warped;
    g.wstride = (int)(wstride / e);
    g.vec = aligned_for(a, astride, e) && aligned_for(blended, ostride, e) && aligned_for(warped, wstride, e);
    return depth == MICV_DEPTH_8U ? launch_warp_t<uint8_t, true>(static_cast<hipStream_t>(stream), g, 1, false)
                                  : launch_warp_t<float, true>(static_cast<hipStream_t>(stream), g, 1, false);
}

}  // extern "C"
