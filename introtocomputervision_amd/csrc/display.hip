// display.hip -- the display tail of the reference's drivers on the device, and ps2's driver around it:
//   cv::normalize(x, x, 0, 255, NORM_MINMAX, CV_8U), `ones * 255 - x`, cv::applyColorMap(COLORMAP_JET)
//   (ps2 main.cpp:94-320, ps4 Solution.cpp:67,108, ps5 Solution.cpp:74-77), addNoise (main.cpp:140-153), the contrast
//   gain (:191-193), disparitySSDPair / disparityNCorrPair (:21-78), cv::randn (host).
// The contract is in include/mi_cv.h ("display") and DESIGN.md section 2; tests/_display_ref.py restates it in numpy.
//
// Normalising is two launches for any number of images.  minmax_kernel: a lane reads 16 bytes at a time where the
// image is aligned for it, a capped grid strides over the image, lanes keep their extremes as order-preserving 32-bit
// keys (so NaNs drop out and every source depth shares the code), a wave reduces with shuffles, the four waves of a
// workgroup meet in LDS, and one lane issues at most two atomic max per workgroup and image: the maximum's key, and the
// COMPLEMENT of the minimum's, so that a zero word means "nothing seen" on both sides and one memset resets them.  An
// image has 16 such pairs of words, each in a cache line of its own, taken by its workgroups in turn and folded by the
// apply pass: atomics that meet in one line wait for each other (profiles/display/README.md).
// Minimum and maximum are exact: nothing depends on the grid or on the order of arrival.  apply_kernel: every lane
// forms the two float constants from the keys itself, in double with a correctly rounded division (the lanes of a wave
// do that in the same instructions), then maps four adjacent pixels and stores them as one dword (u8, inverted) and
// three dwords (JET, out of a 1 KiB table in LDS) where the destination is aligned for it.
// -ffp-contract=off: `src * a + b` is a multiply and an add.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "common.hpp"
#include "cv_rng.hpp"
#include "minmax_keys.hpp"

namespace micv {

// The JET ramp of shim/micv_viz.hpp (apply_colormap_jet), expression for expression: 255 * ramp is a half-integer on
// every sloped entry, so the rounding error of i / 255.0 decides the direction and no rearrangement is equivalent.
void jet_lut_packed(unsigned *lut256) {
    for (int i = 0; i < 256; i++) {
        const double x = i / 255.0;
        auto ramp = [](double t) { return t < 0 ? 0.0 : (t > 1 ? 1.0 : t); };
        const double r = ramp(1.5 - std::fabs(4 * x - 3)), g = ramp(1.5 - std::fabs(4 * x - 2)), b = ramp(1.5 - std::fabs(4 * x - 1));
        const unsigned bb = (unsigned)clampi((int)std::lrint(b * 255), 0, 255), gg = (unsigned)clampi((int)std::lrint(g * 255), 0, 255),
                       rr = (unsigned)clampi((int)std::lrint(r * 255), 0, 255);
        lut256[i] = bb | gg << 8 | rr << 16;
    }
}

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 128, kTileH = 8;  // apply: 32 lanes x 4 pixels, 8 rows
constexpr int kKeySlots = micv_ctx::kDisplayKeySlots, kKeyStride = micv_ctx::kDisplayKeyStride;  // (stride in words)
constexpr unsigned kMaxBlocksPerImage = 512;  // 32 workgroups, 64 atomics, per line

struct MinMaxArgs {
    const void *src;   // image z at src + z * pitch
    ptrdiff_t pitch;
    int rows, cols;
    size_t stride;     // bytes
    int vec;           // every row start is 16-byte aligned
    unsigned *keys;    // image z, slot k: [kKeyStride (z kKeySlots + k)]: ~key(min), [.. + 1]: key(max); zero before the launch
};

template <typename T>
__global__ __launch_bounds__(kThreads) void minmax_kernel(const MinMaxArgs g) {
    constexpr int V = 16 / (int)sizeof(T), U = 4;  // elements per 16-byte chunk; chunks in flight per lane
    const int z = blockIdx.y;
    const char *base = static_cast<const char *>(g.src) + (ptrdiff_t)z * g.pitch;
    const unsigned cpr = ((unsigned)g.cols + V - 1) / V, total = (unsigned)g.rows * cpr;  // 16-byte chunks per row, in all
    const unsigned step = gridDim.x * kThreads;
    unsigned kmax = 0, kmin = 0;
    for (unsigned w0 = blockIdx.x * kThreads + threadIdx.x; w0 < total; w0 += U * step) {
        T v[U][V];
#pragma unroll
        for (int j = 0; j < U; j++) {  // a chunk past the end reads the lane's first one again: harmless for min and max
            const unsigned wj = w0 + j * step, w = wj < total ? wj : w0;
            const unsigned y = w / cpr, c = w - y * cpr;
            const T *p = reinterpret_cast<const T *>(base + (size_t)y * g.stride) + (size_t)c * V;
            const int n = min(V, g.cols - (int)c * V);
            if (g.vec && n == V) {
                const uint4 q = *reinterpret_cast<const uint4 *>(p);
                __builtin_memcpy(v[j], &q, 16);
            } else {
                for (int i = 0; i < V; i++) v[j][i] = p[i < n ? i : 0];
            }
        }
#pragma unroll
        for (int j = 0; j < U; j++)
#pragma unroll
            for (int i = 0; i < V; i++) {
                const float f = (float)v[j][i];
                if (f == f) {
                    const unsigned k = key_of(f);
                    kmax = max(kmax, k);
                    kmin = max(kmin, ~k);
                }
            }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off));
        kmin = max(kmin, (unsigned)__shfl_xor((int)kmin, off));
    }
    __shared__ unsigned part[kThreads / 64][2];
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = kmin;
        part[threadIdx.x >> 6][1] = kmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; w++) {
            kmin = max(kmin, part[w][0]);
            kmax = max(kmax, part[w][1]);
        }
        // One image's workgroups spread over kKeySlots pairs of words, each pair in a 128-byte line of its own: atomics on
        // one line queue up behind each other at about 16 ns apiece (2025 workgroups on one pair of words: 48 us at 1080p,
        // and as much with 16 pairs inside one line), whichever words of the line they name.
        unsigned *slot = g.keys + kKeyStride * ((size_t)z * kKeySlots + (blockIdx.x % kKeySlots));
        if (kmax) {  // (a workgroup that saw NaNs only has nothing to say)
            atomicMax(slot, kmin);
            atomicMax(slot + 1, kmax);
        }
    }
}

struct Plane {
    uint8_t *p;  // image z at p + z * pitch; NULL: not wanted
    ptrdiff_t pitch;
    size_t stride;
    int vec;     // every row start is 4-byte aligned
};

struct ApplyArgs {
    const void *src;
    ptrdiff_t src_pitch;
    int rows, cols;
    size_t sstride;
    int src_vec;          // every row start aligned for a 4-pixel load
    Plane u8, inv, jet;
    int inv_images;       // images z < inv_images write `inv` (the ps2 chain inverts its left map only)
    const unsigned *keys, *lut;
    float *minmax_out;    // optional, [2 z], [2 z + 1]
};

__device__ __forceinline__ void store_px4(const Plane &pl, int z, int y, int x0, int n, const unsigned v[4]) {
    uint8_t *d = pl.p + (ptrdiff_t)z * pl.pitch + (size_t)y * pl.stride + x0;
    if (pl.vec && n == 4) {
        *reinterpret_cast<unsigned *>(d) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    } else {
        for (int i = 0; i < 4; i++)
            if (i < n) d[i] = (uint8_t)v[i];
    }
}

// NORMALIZE: t = src * a + b from the image's keys; otherwise (cv::applyColorMap alone) the u8 source is the value.
template <typename T, bool NORMALIZE>
__global__ __launch_bounds__(kThreads) void apply_kernel(const ApplyArgs g) {
    __shared__ unsigned lut[256];
    if (g.jet.p) {
        lut[threadIdx.x] = g.lut[threadIdx.x];
        __syncthreads();
    }
    const int z = blockIdx.z;
    float a = 0.f, b = 0.f;
    if constexpr (NORMALIZE) {
        unsigned kmin = 0, kmax = 0;  // (wave-uniform addresses: scalar loads)
        for (int k = 0; k < kKeySlots; k++) {
            kmin = max(kmin, g.keys[kKeyStride * ((size_t)z * kKeySlots + k)]);
            kmax = max(kmax, g.keys[kKeyStride * ((size_t)z * kKeySlots + k) + 1]);
        }
        float flo = __uint_as_float(0x7fc00000u), fhi = flo;
        if (kmax) {
            flo = value_of(~kmin);
            fhi = value_of(kmax);
            const double lo = flo, hi = fhi;
            const double scale = 255.0 * (hi - lo > DBL_EPSILON ? 1.0 / (hi - lo) : 0.0), shift = 0.0 - lo * scale;
            a = (float)scale;
            b = (float)shift;
        }
        if (g.minmax_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            g.minmax_out[2 * z] = flo;
            g.minmax_out[2 * z + 1] = fhi;
        }
    }
    const int x0 = blockIdx.x * kTileW + (threadIdx.x & 31) * 4;
    if (x0 >= g.cols) return;
    const int n = min(4, g.cols - x0);
    const char *sbase = static_cast<const char *>(g.src) + (ptrdiff_t)z * g.src_pitch;
    for (int y = blockIdx.y * kTileH + (threadIdx.x >> 5); y < g.rows; y += gridDim.y * kTileH) {
        const T *p = reinterpret_cast<const T *>(sbase + (size_t)y * g.sstride) + x0;
        T s[4];
        if (g.src_vec && n == 4) {
            __builtin_memcpy(s, __builtin_assume_aligned(p, 4 * sizeof(T)), 4 * sizeof(T));
        } else {
            for (int i = 0; i < 4; i++) s[i] = p[i < n ? i : 0];
        }
        unsigned v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if constexpr (NORMALIZE) {
                const float t = (float)s[i] * a + b;
                const float r = fminf(fmaxf(rintf(t), 0.f), 255.f);
                v[i] = isfinite(t) ? (unsigned)(int)r : 0u;
            } else {
                v[i] = (unsigned)s[i];
            }
        }
        if (NORMALIZE && g.u8.p) store_px4(g.u8, z, y, x0, n, v);
        if (NORMALIZE && g.inv.p && z < g.inv_images) {
            const unsigned w[4] = {255u - v[0], 255u - v[1], 255u - v[2], 255u - v[3]};
            store_px4(g.inv, z, y, x0, n, w);
        }
        if (g.jet.p) {
            const unsigned e0 = lut[v[0]], e1 = lut[v[1]], e2 = lut[v[2]], e3 = lut[v[3]];
            uint8_t *d = g.jet.p + (ptrdiff_t)z * g.jet.pitch + (size_t)y * g.jet.stride + 3 * (size_t)x0;
            if (g.jet.vec && n == 4) {  // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
                unsigned *q = reinterpret_cast<unsigned *>(d);
                q[0] = e0 | e1 << 24;
                q[1] = e1 >> 8 | e2 << 16;
                q[2] = e2 >> 16 | e3 << 8;
            } else {
                const unsigned e[4] = {e0, e1, e2, e3};
                for (int i = 0; i < 4; i++)
                    if (i < n) {
                        d[3 * i] = (uint8_t)e[i];
                        d[3 * i + 1] = (uint8_t)(e[i] >> 8);
                        d[3 * i + 2] = (uint8_t)(e[i] >> 16);
                    }
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void gain_noise_kernel(const float *src, int sstride, float gain,
                                                              const float *noise, int nstride, int rows, int cols,
                                                              float *dst, int dstride, int vec) {
    const int x0 = (blockIdx.x * 32 + (threadIdx.x & 31)) * 4;
    if (x0 >= cols) return;
    const int n = min(4, cols - x0);
    for (int y = blockIdx.y * kTileH + (threadIdx.x >> 5); y < rows; y += gridDim.y * kTileH) {
        float s[4], e[4] = {0.f, 0.f, 0.f, 0.f};
        const float *sp = src + (size_t)y * sstride + x0, *np = noise ? noise + (size_t)y * nstride + x0 : nullptr;
        float *dp = dst + (size_t)y * dstride + x0;
        if (vec && n == 4) {
            __builtin_memcpy(s, __builtin_assume_aligned(sp, 16), 16);
            if (np) __builtin_memcpy(e, __builtin_assume_aligned(np, 16), 16);
        } else {
            for (int i = 0; i < 4; i++) {
                s[i] = sp[i < n ? i : 0];
                if (np) e[i] = np[i < n ? i : 0];
            }
        }
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = s[i] * gain + e[i];
        if (vec && n == 4) {
            __builtin_memcpy(__builtin_assume_aligned(dp, 16), o, 16);
        } else {
            for (int i = 0; i < 4; i++)
                if (i < n) dp[i] = o[i];
        }
    }
}

inline size_t elem_of(int depth) { return depth == MICV_DEPTH_32F ? 4 : 1; }
inline bool depth_ok(int depth) { return depth == MICV_DEPTH_32F || depth == MICV_DEPTH_8U || depth == MICV_DEPTH_8S; }
inline bool aligned(const void *p, ptrdiff_t pitch, size_t stride, size_t to) {
    return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)pitch | stride) % to) == 0;
}
inline unsigned rows_grid(int rows) { return std::min(cdiv(rows, kTileH), 65535u); }

struct Out {
    uint8_t *p;
    ptrdiff_t pitch;
    size_t stride;
};
inline Plane plane_of(const Out &o, int z0) {
    return Plane{o.p ? o.p + (ptrdiff_t)z0 * o.pitch : nullptr, o.pitch, o.stride, aligned(o.p, o.pitch, o.stride, 4)};
}

template <typename T>
void launch_minmax(hipStream_t s, const MinMaxArgs &g, unsigned bx, int nz) {
    minmax_kernel<T><<<dim3(bx, nz), kThreads, 0, s>>>(g);
}
template <typename T, bool N>
void launch_apply(hipStream_t s, const ApplyArgs &g, int nz) {
    apply_kernel<T, N><<<dim3(cdiv(g.cols, kTileW), rows_grid(g.rows), nz), kThreads, 0, s>>>(g);
}

// The two launches per chunk of images.  Pitches are signed: the ps2 chain passes its two maps, wherever they lie, as
// a batch of two.  Arguments are checked by the callers.
int normalize_images(micv_ctx *ctx, const void *src, ptrdiff_t src_pitch, int depth, int batch, int rows, int cols,
                     size_t sstride, const Out &u8, const Out &inv, int inv_images, const Out &jet, float *minmax_out,
                     hipStream_t s) {
    const size_t e = elem_of(depth);
    const unsigned *lut = static_cast<const unsigned *>(ctx->display_state);
    unsigned *keys = static_cast<unsigned *>(ctx->display_state) + 256;
    const unsigned chunks = cdiv(cols, 16 / (unsigned)e) * (unsigned)rows;
    for (int z0 = 0; z0 < batch; z0 += micv_ctx::kDisplayMaxBatch) {
        const int nz = std::min(batch - z0, micv_ctx::kDisplayMaxBatch);
        const char *sz = static_cast<const char *>(src) + (ptrdiff_t)z0 * src_pitch;
        MICV_HIP(hipMemsetAsync(keys, 0, (size_t)nz * kKeySlots * kKeyStride * 4, s));
        MinMaxArgs m{sz, src_pitch, rows, cols, sstride, aligned(src, src_pitch, sstride, 16), keys};
        // a capped grid: about eight workgroups per compute unit over the whole batch and at most 512 per image, each lane
        // striding the rest; four chunks per lane and pass where that still leaves a workgroup per compute unit
        const unsigned cap = std::min(std::max(1u, (unsigned)ctx->wave_slots(2) / (unsigned)nz), kMaxBlocksPerImage);
        const unsigned bx = std::min(std::max(cdiv(chunks, 4 * kThreads), std::min(cdiv(chunks, kThreads), 256u)), cap);
        if (depth == MICV_DEPTH_32F) launch_minmax<float>(s, m, bx, nz);
        else if (depth == MICV_DEPTH_8U) launch_minmax<uint8_t>(s, m, bx, nz);
        else launch_minmax<int8_t>(s, m, bx, nz);
        MICV_LAUNCH_CHECK();
        ApplyArgs a{};
        a.src = sz; a.src_pitch = src_pitch;
        a.rows = rows; a.cols = cols; a.sstride = sstride;
        a.src_vec = aligned(src, src_pitch, sstride, 4 * e);
        a.u8 = plane_of(u8, z0); a.inv = plane_of(inv, z0); a.jet = plane_of(jet, z0);
        a.inv_images = inv_images - z0;
        a.keys = keys; a.lut = lut;
        a.minmax_out = minmax_out ? minmax_out + 2 * (size_t)z0 : nullptr;
        if (depth == MICV_DEPTH_32F) launch_apply<float, true>(s, a, nz);
        else if (depth == MICV_DEPTH_8U) launch_apply<uint8_t, true>(s, a, nz);
        else launch_apply<int8_t, true>(s, a, nz);
        MICV_LAUNCH_CHECK();
    }
    return MICV_OK;
}

inline bool out_ok(const uint8_t *p, size_t pitch, size_t stride, int batch, int rows, int cols, int bpp) {
    if (!p) return true;
    const size_t row = (size_t)cols * bpp;
    return stride >= row && stride < (size_t)1 << 32 && (batch <= 1 || pitch >= (size_t)(rows - 1) * stride + row);
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_normalize_minmax_batch_dev(micv_ctx *ctx, const void *src, size_t src_pitch, int depth, int batch, int rows, int cols,
                                    size_t sstride, uint8_t *dst_u8, size_t u8_pitch, size_t u8_stride,
                                    uint8_t *dst_inverted, size_t inverted_pitch, size_t inverted_stride, uint8_t *dst_jet,
                                    size_t jet_pitch, size_t jet_stride, float *minmax_out, micv_stream stream) {
    MICV_REQUIRE(ctx && src, "micv_normalize_minmax: null argument");
    MICV_REQUIRE(dst_u8 || dst_inverted || dst_jet, "micv_normalize_minmax: no output wanted (dst_u8, dst_inverted and dst_jet are NULL)");
    MICV_REQUIRE(depth_ok(depth), "micv_normalize_minmax: depth %d is none of 32F, 8U, 8S", depth);
    MICV_REQUIRE(batch >= 0, "micv_normalize_minmax: batch %d < 0", batch);
    const size_t e = elem_of(depth);
    MICV_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols < ((int64_t)1 << 31) && stride_ok(sstride, cols, e),
                 "micv_normalize_minmax: bad size %dx%d (rows * cols < 2^31) or stride %zu", rows, cols, sstride);
    MICV_REQUIRE(batch <= 1 || (src_pitch % e == 0 && src_pitch >= (size_t)(rows - 1) * sstride + (size_t)cols * e),
                 "micv_normalize_minmax: source pitch smaller than an image");
    MICV_REQUIRE(out_ok(dst_u8, u8_pitch, u8_stride, batch, rows, cols, 1) &&
                     out_ok(dst_inverted, inverted_pitch, inverted_stride, batch, rows, cols, 1) &&
                     out_ok(dst_jet, jet_pitch, jet_stride, batch, rows, cols, 3),
                 "micv_normalize_minmax: an output's stride or pitch is smaller than its rows or images");
    MICV_REQUIRE(src != dst_u8 && src != dst_inverted && src != dst_jet, "micv_normalize_minmax: src and an output alias");
    if (batch == 0) return MICV_OK;
    MICV_HIP(hipSetDevice(ctx->device));
    return normalize_images(ctx, src, (ptrdiff_t)src_pitch, depth, batch, rows, cols, sstride,
                            Out{dst_u8, (ptrdiff_t)u8_pitch, u8_stride}, Out{dst_inverted, (ptrdiff_t)inverted_pitch, inverted_stride},
                            batch, Out{dst_jet, (ptrdiff_t)jet_pitch, jet_stride}, minmax_out, static_cast<hipStream_t>(stream));
}

int micv_normalize_minmax_dev(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride,
                              uint8_t *dst_u8, size_t u8_stride, uint8_t *dst_inverted, size_t inverted_stride,
                              uint8_t *dst_jet, size_t jet_stride, float *minmax_out, micv_stream stream) {
    return micv_normalize_minmax_batch_dev(ctx, src, 0, depth, 1, rows, cols, sstride, dst_u8, 0, u8_stride, dst_inverted, 0,
                                           inverted_stride, dst_jet, 0, jet_stride, minmax_out, stream);
}

int micv_apply_colormap_jet_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, uint8_t *dst_jet,
                                size_t jet_stride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst_jet, "micv_apply_colormap_jet: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols < ((int64_t)1 << 31) && stride_ok(sstride, cols, 1) &&
                     out_ok(dst_jet, 0, jet_stride, 1, rows, cols, 3),
                 "micv_apply_colormap_jet: bad size %dx%d (rows * cols < 2^31) or stride", rows, cols);
    MICV_REQUIRE(src != dst_jet, "micv_apply_colormap_jet: src and dst_jet alias");
    MICV_HIP(hipSetDevice(ctx->device));
    ApplyArgs a{};
    a.src = src;
    a.rows = rows; a.cols = cols; a.sstride = sstride;
    a.src_vec = aligned(src, 0, sstride, 4);
    a.jet = plane_of(Out{dst_jet, 0, jet_stride}, 0);
    a.lut = static_cast<const unsigned *>(ctx->display_state);
    launch_apply<uint8_t, false>(static_cast<hipStream_t>(stream), a, 1);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_gain_noise_f32_dev(micv_ctx *ctx, const float *src, size_t sstride, float gain, const float *noise, size_t nstride,
                            int rows, int cols, float *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_gain_noise_f32: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride_ok(sstride, cols, 4) && stride_ok(dstride, cols, 4) &&
                     (!noise || stride_ok(nstride, cols, 4)),
                 "micv_gain_noise_f32: bad size %dx%d or stride", rows, cols);
    MICV_HIP(hipSetDevice(ctx->device));
    const int vec = aligned(src, 0, sstride, 16) && aligned(dst, 0, dstride, 16) && (!noise || aligned(noise, 0, nstride, 16));
    gain_noise_kernel<<<dim3(cdiv(cols, kTileW), rows_grid(rows)), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        src, (int)(sstride / 4), gain, noise, (int)(nstride / 4), rows, cols, dst, (int)(dstride / 4), vec);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_cv_randn_f32_host(uint64_t *state, float mean, float sigma, int rows, int cols, float *dst, size_t dstride) {
    MICV_REQUIRE(state && dst, "micv_cv_randn_f32_host: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride_ok(dstride, cols, 4), "micv_cv_randn_f32_host: bad size %dx%d or stride", rows, cols);
    CvRng rng(*state);
    for (int y = 0; y < rows; y++) {
        float *row = reinterpret_cast<float *>(reinterpret_cast<char *>(dst) + (size_t)y * dstride);
        for (int x = 0; x < cols; x++) {
            const float z = (float)rng.gaussian(1.0);  // (the draw itself: a float widened, times 1.0)
            row[x] = z * sigma + mean;
        }
    }
    *state = rng.state;
    return MICV_OK;
}

int micv_disparity_pair_dev(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                            int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                            int8_t *disp_right, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && left && right && disp_left && disp_right, "micv_disparity_pair: null argument");
    MICV_REQUIRE(metric == MICV_DISPARITY_SSD || metric == MICV_DISPARITY_NCC, "micv_disparity_pair: metric %d is neither SSD (0) nor NCC (1)", metric);
    MICV_REQUIRE(disparity_range >= 0 && disparity_range <= 127, "micv_disparity_pair: disparity range %d out of 0..127", disparity_range);
    MICV_REQUIRE(disp_left != disp_right, "micv_disparity_pair: the two maps alias");
    const auto search = metric == MICV_DISPARITY_NCC ? micv_disparity_ncorr_dev : micv_disparity_ssd_dev;
    MICV_TRY(search(ctx, left, right, rows, cols, stride, window_rad, -disparity_range, 0, flags, disp_left, dstride, stream));
    return search(ctx, right, left, rows, cols, stride, window_rad, 0, disparity_range, flags, disp_right, dstride, stream);
}

int micv_disparity_pair_display_dev(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                                    float gain, const float *noise_left, const float *noise_right, size_t nstride,
                                    int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                                    int8_t *disp_right, size_t dstride, uint8_t *image_left, uint8_t *image_left_inverted,
                                    uint8_t *image_right, size_t istride, float *work, micv_stream stream) {
    MICV_REQUIRE(ctx && left && right && disp_left && disp_right && image_left && image_right,
                 "micv_disparity_pair_display: null argument");
    MICV_REQUIRE(!noise_left == !noise_right, "micv_disparity_pair_display: one noise image without the other");
    MICV_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols < ((int64_t)1 << 31) && istride >= (size_t)cols &&
                     istride < (size_t)1 << 32 && dstride >= (size_t)cols && stride_ok(stride, cols, 4),
                 "micv_disparity_pair_display: bad size %dx%d (rows * cols < 2^31) or stride", rows, cols);
    MICV_REQUIRE(image_left != image_right && image_left != image_left_inverted && image_right != image_left_inverted,
                 "micv_disparity_pair_display: the images alias");
    const bool change = noise_left || gain != 1.f;
    MICV_REQUIRE(!change || work, "micv_disparity_pair_display: gain or noise need `work` (2 * rows * cols floats)");
    MICV_REQUIRE(!noise_left || stride_ok(nstride, cols, 4), "micv_disparity_pair_display: bad noise stride");
    const float *l = left, *r = right;
    size_t st = stride;
    if (change) {
        float *wl = work, *wr = work + (size_t)rows * cols;
        st = (size_t)cols * 4;
        MICV_TRY(micv_gain_noise_f32_dev(ctx, left, stride, gain, noise_left, nstride, rows, cols, wl, st, stream));
        MICV_TRY(micv_gain_noise_f32_dev(ctx, right, stride, gain, noise_right, nstride, rows, cols, wr, st, stream));
        l = wl;
        r = wr;
    }
    MICV_TRY(micv_disparity_pair_dev(ctx, l, r, rows, cols, st, window_rad, disparity_range, metric, flags, disp_left, disp_right,
                                     dstride, stream));
    // the two maps as a batch of two, wherever they lie: signed pitches
    const ptrdiff_t dp = reinterpret_cast<const char *>(disp_right) - reinterpret_cast<const char *>(disp_left);
    const ptrdiff_t ip = image_right - image_left;
    return normalize_images(ctx, disp_left, dp, MICV_DEPTH_8S, 2, rows, cols, dstride, Out{image_left, ip, istride},
                            Out{image_left_inverted, 0, istride}, 1, Out{nullptr, 0, 0}, nullptr, static_cast<hipStream_t>(stream));
}

}  // extern "C"
