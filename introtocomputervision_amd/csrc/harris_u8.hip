// harris_u8.hip -- the ps4 corner chain on byte images: micv_harris_corners_u8_{dev,host,batch_dev} (mi_cv.h).
//
// Fused form (3x3 Sobel, window 3 / 5 / 7): three launches for a whole piece of a batch, none of which waits for the host
//   harris_image_response_kernel      harris.hip: the f32 tile instantiated on a byte source, image = blockIdx.z
//   harris_nms_tiled_kernel           harris.hip: the f32 NMS tiles with an NmsBatch, image = blockIdx.z
//   harris_list_kernel                here: ONE workgroup per image walks that image's mask words in order, writes its list,
//                                     its own count and (when asked) the keypoint rows -- no workgroup waits for another,
//                                     no status words, no compact_state slot; the result does not depend on the grid
// Every other form converts image by image and calls micv_harris_corners_dev.
//
// Keypoints without planes: sift::getKeypoints reads ONE gradient sample per corner.  On bytes every 3x3 Sobel value is
// an integer with |g| <= 1020, exact in f32 in any evaluation order, and never -0 (the f32 chains start from +0, and
// x + (-x) is +0); so the sample is recomputed at the corner from its reflected 3x3 neighbourhood in integers and is the
// float the plane holds.
#include "host_io.hpp"
#include "kernels.hpp"

namespace micv {

constexpr size_t kHarrisU8BatchBytes = size_t(64) << 20;  // mi_cv.h: MICV_OPT_HARRIS_BATCH_MB
constexpr int kListThreads = 1024, kListPerThread = 4;
constexpr int64_t kHarrisListMaxWords = 1 << 16;  // mi_cv.h: the bound of the one-workgroup list kernel
// A launch of ONE image has one workgroup to walk all of its words, where the chained scan spreads them over many:
// measured at 1080p (32 400 words, 14 516 corners) 52 us for the call against 39 for the f32 entry, and 87 against 84 with
// the keypoints in the kernel's tail (profiles/harris_u8/single_1080p_before.jsonl); at 480 x 640 (4800 words) the list
// kernel is the faster one.  So a single image above this many words takes the per-image list step as well.
constexpr int64_t kHarrisListSingleWords = 1 << 13;

__global__ __launch_bounds__(256) void harris_u8_to_f32_kernel(const uint8_t *__restrict__ src, size_t pitch, int rows, int cols,
                                                               float *__restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    out[(size_t)y * cols + x] = (float)src[(size_t)y * pitch + x];
}

// harris::getGradients at (y, x) of a byte image: 3x3 Sobel, BORDER_REFLECT_101, in integers.
__device__ __forceinline__ void sobel3_at_u8(const uint8_t *__restrict__ img, size_t pitch, int rows, int cols, int y, int x, float *gxv,
                                             float *gyv) {
    const uint8_t *r0 = img + (size_t)reflect101(y - 1, rows) * pitch, *r1 = img + (size_t)y * pitch,
                  *r2 = img + (size_t)reflect101(y + 1, rows) * pitch;
    const int xl = reflect101(x - 1, cols), xr = reflect101(x + 1, cols);
    const int a = r0[xl], b = r0[x], c = r0[xr], d = r1[xl], f = r1[xr], g = r2[xl], h = r2[x], i = r2[xr];
    *gxv = (float)((c + 2 * f + i) - (a + 2 * d + g));
    *gyv = (float)((g + 2 * h + i) - (a + 2 * b + c));
}

// One workgroup per image (blockIdx.x).  Pass p takes the 4096 words [4096 p, 4096 p + 4096): a thread loads four
// consecutive words, the workgroup scans the popcounts (wave scan + the 16 wave totals in LDS), and every thread emits its
// words' corners at base + its exclusive prefix: row-major order, as the chained scan of compact.hpp gives it.  Rows at
// and past `cap` are not written.  Then, keypoints: the workgroup walks the rows it has just written.
__global__ __launch_bounds__(kListThreads) void harris_list_kernel(const unsigned long long *__restrict__ rowmask, size_t mask_words, int nseg,
                                                                   int tiles_x, int32_t *locs, int64_t cap, int64_t *__restrict__ count,
                                                                   const uint8_t *__restrict__ img, size_t img_dist, size_t pitch, int rows,
                                                                   int cols, float kp_size, float *__restrict__ kp) {
    __shared__ unsigned wave_total[kListThreads / 64];
    const size_t z = blockIdx.x;
    const unsigned long long *m = rowmask + z * mask_words;
    int32_t *L = locs + z * (size_t)cap * 2;  // (never dereferenced when cap == 0)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned base = 0;  // rows * cols < 2^31
    for (int w0 = 0; w0 < nseg; w0 += kListThreads * kListPerThread) {
        const int i0 = w0 + kListPerThread * (int)threadIdx.x;
        unsigned long long w[kListPerThread];
        unsigned pc = 0;
#pragma unroll
        for (int k = 0; k < kListPerThread; k++) {
            w[k] = i0 + k < nseg ? m[i0 + k] : 0ull;
            pc += __popcll(w[k]);
        }
        unsigned incl = pc;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < kListThreads / 64; j++) {
            const unsigned t = wave_total[j];
            before += j < wave ? t : 0u;
            total += t;
        }
        __syncthreads();  // wave_total is written again in the next pass
        int64_t pos = (int64_t)base + before + incl - pc;
#pragma unroll
        for (int k = 0; k < kListPerThread; k++) {
            unsigned long long bits = w[k];
            if (!bits) continue;
            const int y = (i0 + k) / tiles_x, xb = 64 * ((i0 + k) - y * tiles_x);
            while (bits) {
                const int b = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                if (pos < cap) {
                    L[2 * pos] = y;
                    L[2 * pos + 1] = xb + b;
                }
                pos++;
            }
        }
        base += total;
    }
    if (threadIdx.x == 0) count[z] = base;
    if (!kp) return;
    __syncthreads();  // the rows this workgroup wrote are read back by other waves of it
    const int64_t n = (int64_t)base < cap ? (int64_t)base : cap;
    const uint8_t *src = img + z * img_dist;
    float *K = kp + z * (size_t)cap * 4;
    for (int64_t i = threadIdx.x; i < n; i += kListThreads) {
        const int y = L[2 * i], x = L[2 * i + 1];
        float gxv, gyv;
        sobel3_at_u8(src, pitch, rows, cols, y, x, &gxv, &gyv);
        sift_keypoint_store(gxv, gyv, y, x, kp_size, K + 4 * i);
    }
}

// Keypoint rows 0 .. min(count, cap) - 1 of image blockIdx.y, the count read on the device: from the bytes (BYTES: the
// images too large for harris_list_kernel) or from gradient planes (the converted forms; sift_keypoints_kernel's row).
template <bool BYTES>
__global__ __launch_bounds__(256) void harris_keypoints_counted_kernel(const uint8_t *__restrict__ img, size_t img_dist, size_t pitch,
                                                                       const float *__restrict__ gx, const float *__restrict__ gy,
                                                                       size_t gstride, int rows, int cols, const int32_t *__restrict__ locs,
                                                                       int64_t cap, const int64_t *__restrict__ count, float kp_size,
                                                                       float *__restrict__ kp) {
    const size_t z = blockIdx.y;
    const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
    const int64_t n = count[z] < cap ? count[z] : cap;
    if (i >= n) return;
    const int32_t *L = locs + z * (size_t)cap * 2;
    const int y = L[2 * i], x = L[2 * i + 1];
    float gxv, gyv;
    if (BYTES) {
        sobel3_at_u8(img + z * img_dist, pitch, rows, cols, y, x, &gxv, &gyv);
    } else {
        gxv = gx[(size_t)y * gstride + x];
        gyv = gy[(size_t)y * gstride + x];
    }
    sift_keypoint_store(gxv, gyv, y, x, kp_size, kp + (z * (size_t)cap + i) * 4);
}

struct Span {
    uintptr_t p;
    size_t extent, dist;  // one image's bytes; distance between images (0: a dense array of the whole batch, extent = all of it)
    const char *name;
};
// Do the per-image extents of a and b share a byte anywhere in a batch?  Planes at one distance may interleave.
static bool spans_overlap(const Span &a, const Span &b, int batch) {
    const size_t ta = a.dist ? (size_t)(batch - 1) * a.dist + a.extent : a.extent, tb = b.dist ? (size_t)(batch - 1) * b.dist + b.extent : b.extent;
    if (a.p + ta <= b.p || b.p + tb <= a.p) return false;
    if (a.dist && a.dist == b.dist) {
        const Span &lo = a.p <= b.p ? a : b, &hi = a.p <= b.p ? b : a;
        const size_t off = (hi.p - lo.p) % a.dist;
        return !(off >= lo.extent && off + hi.extent <= a.dist);
    }
    return true;
}

static int harris_u8_common(const char *fn, micv_ctx *ctx, const uint8_t *img, size_t img_dist, int batch, int rows, int cols, size_t stride,
                            int sobel_ksize, int win, double sigma, float alpha, int flags, double threshold, int min_distance, float *gx,
                            float *gy, size_t g_dist, size_t gstride, float *resp, size_t r_dist, size_t rstride, float *corners,
                            size_t c_dist, size_t cstride, int32_t *locs_yx, int64_t cap, int64_t *count, float kp_size, float *kp_xysa,
                            micv_stream stream) {
    MICV_REQUIRE(ctx && img && count, "%s: null argument", fn);
    MICV_REQUIRE(batch >= 1, "%s: batch %d", fn, batch);
    MICV_REQUIRE((gx == nullptr) == (gy == nullptr), "%s: give both gradient outputs or neither", fn);
    MICV_REQUIRE(locs_yx || cap == 0, "%s: locs_yx is null", fn);
    MICV_REQUIRE(!kp_xysa || locs_yx, "%s: kp_xysa needs locs_yx", fn);
    MICV_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols < ((int64_t)1 << 31), "%s: bad size %dx%d", fn, rows, cols);
    MICV_REQUIRE(win >= 1 && (win & 1) && win <= kMaxWin, "%s: window %d must be odd and <= %d", fn, win, kMaxWin);
    MICV_REQUIRE(sigma > 0 && min_distance >= 0 && cap >= 0, "%s: bad sigma / min_distance / cap", fn);
    MICV_REQUIRE(stride >= (size_t)cols && stride < ((size_t)1 << 30) && (!gx || stride_ok(gstride, cols, 4)) &&
                     (!resp || stride_ok(rstride, cols, 4)) && (!corners || stride_ok(cstride, cols, 4)),
                 "%s: bad stride", fn);
    MICV_REQUIRE((flags & ~MICV_HARRIS_CPU) == 0, "%s: unknown flags %#x", fn, flags);
    Taps probe;
    MICV_REQUIRE(sobel_taps(sobel_ksize, 1, &probe) >= 0, "%s: Sobel size %d not supported", fn, sobel_ksize);
    if (batch > 1) {
        // the outputs of one batch: a plane's image is the (rows - 1) * stride + cols * 4 bytes from its first pixel
        Span sp[7];
        int ns = 0;
        const size_t row4 = (size_t)cols * 4;
        if (gx) {
            sp[ns++] = {reinterpret_cast<uintptr_t>(gx), (size_t)(rows - 1) * gstride + row4, g_dist, "gx"};
            sp[ns++] = {reinterpret_cast<uintptr_t>(gy), (size_t)(rows - 1) * gstride + row4, g_dist, "gy"};
        }
        if (resp) sp[ns++] = {reinterpret_cast<uintptr_t>(resp), (size_t)(rows - 1) * rstride + row4, r_dist, "resp"};
        if (corners) sp[ns++] = {reinterpret_cast<uintptr_t>(corners), (size_t)(rows - 1) * cstride + row4, c_dist, "corners"};
        const int nplanes = ns;
        if (locs_yx && cap) sp[ns++] = {reinterpret_cast<uintptr_t>(locs_yx), (size_t)batch * cap * 8, 0, "locs_yx"};
        sp[ns++] = {reinterpret_cast<uintptr_t>(count), (size_t)batch * 8, 0, "count"};
        if (kp_xysa && cap) sp[ns++] = {reinterpret_cast<uintptr_t>(kp_xysa), (size_t)batch * cap * 16, 0, "kp_xysa"};
        for (int i = 0; i < nplanes; i++)
            MICV_REQUIRE(sp[i].dist % 4 == 0 && sp[i].dist >= sp[i].extent, "%s: the %s planes of a batch overlap (image stride %zu)", fn,
                         sp[i].name, sp[i].dist);
        for (int i = 0; i < ns; i++)
            for (int j = i + 1; j < ns; j++)
                MICV_REQUIRE(!spans_overlap(sp[i], sp[j], batch), "%s: the outputs %s and %s of a batch overlap", fn, sp[i].name, sp[j].name);
    }
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int r = win / 2;
    const bool cpu = (flags & MICV_HARRIS_CPU) != 0;
    const size_t n = (size_t)rows * cols;
    // the condition of `fused` in micv_harris_corners_dev
    const bool fused = sobel_ksize == 3 && r >= 1 && r <= 3 && !ctx->opt[MICV_OPT_HARRIS_GENERIC] && !ctx->opt[MICV_OPT_SOBEL_GENERIC];
    if (!fused) {
        // The image as f32, and the gradient planes the keypoints are read from when the caller keeps none, in the context's
        // chain block (the f32 entry carves the arena itself); one image after the other.
        const bool own_planes = kp_xysa && !gx;
        void *pool = nullptr;
        MICV_TRY(ctx->reserve_chain((own_planes ? 3 : 1) * Carver::need(n, 4), &pool));
        Carver c(pool);
        float *f = c.take<float>(n), *px = own_planes ? c.take<float>(n) : nullptr, *py = own_planes ? c.take<float>(n) : nullptr;
        for (int i = 0; i < batch; i++) {
            harris_u8_to_f32_kernel<<<dim3(cdiv(cols, 64), cdiv(rows, 4)), 256, 0, s>>>(img + i * img_dist, stride, rows, cols, f);
            MICV_LAUNCH_CHECK();
            float *gxi = gx ? gx + i * (g_dist / 4) : px, *gyi = gy ? gy + i * (g_dist / 4) : py;
            const size_t gs = gx ? gstride : (size_t)cols * 4;
            int32_t *li = locs_yx ? locs_yx + (size_t)i * cap * 2 : nullptr;
            MICV_TRY(micv_harris_corners_dev(ctx, f, rows, cols, (size_t)cols * 4, sobel_ksize, win, sigma, alpha, flags, threshold,
                                             min_distance, gxi, gyi, gs, resp ? resp + i * (r_dist / 4) : nullptr, rstride,
                                             corners ? corners + i * (c_dist / 4) : nullptr, cstride, li, cap, count + i, stream));
            if (kp_xysa && cap > 0) {
                harris_keypoints_counted_kernel<false><<<dim3((unsigned)((cap + 255) / 256), 1), 256, 0, s>>>(
                    nullptr, 0, 0, gxi, gyi, gs / 4, rows, cols, li, cap, count + i, kp_size, kp_xysa + (size_t)i * cap * 4);
                MICV_LAUNCH_CHECK();
            }
        }
        return MICV_OK;
    }
    // Pieces: a piece's R (when the caller keeps none) and mask words stay within the bound -- one image at least, 65535
    // (grid.z) at most.
    const int tiles_x = cdiv(cols, 64);
    const int64_t nseg = (int64_t)rows * tiles_x;
    const size_t need_r = resp ? 0 : Carver::need(n, 4), need_m = Carver::need(nseg, 8), per_image = need_r + need_m;
    const size_t bound = ctx->opt[MICV_OPT_HARRIS_BATCH_MB] > 0 ? (size_t)ctx->opt[MICV_OPT_HARRIS_BATCH_MB] << 20 : kHarrisU8BatchBytes;
    size_t piece = bound / per_image < 1 ? 1 : bound / per_image;
    if (piece > 65535) piece = 65535;
    if (piece > (size_t)batch) piece = batch;
    const bool one_group = nseg <= (batch == 1 ? kHarrisListSingleWords : kHarrisListMaxWords);
    void *scratch;
    MICV_TRY(ctx->reserve(piece * per_image + (one_group ? 0 : harris_list_scratch_bytes(rows, cols)), &scratch));
    Carver c(scratch);
    float *rs_ = resp ? nullptr : c.take<float>(piece * (need_r / 4));
    unsigned long long *masks = c.take<unsigned long long>(piece * (need_m / 8));
    void *list_scratch = c.base + c.off;
    HarrisU8Launch a;
    a.pitch = stride; a.img_dist = img_dist;
    a.rows = rows; a.cols = cols;
    gaussian_taps(win, sigma, &a.g);  // cv::getGaussianKernel(win, sigma, CV_32F), Harris.cpp:61
    a.alpha = alpha;
    a.resp_dist = resp ? r_dist : need_r;
    a.rstride = resp ? rstride : (size_t)cols * 4;
    a.grad_dist = g_dist; a.gstride = gstride;
    for (int i = 0; i < batch; i += (int)piece) {
        const int ni = batch - i < (int)piece ? batch - i : (int)piece;
        a.images = ni;
        a.img = img + i * img_dist;
        a.resp = resp ? resp + i * (r_dist / 4) : rs_;
        a.gx = gx ? gx + i * (g_dist / 4) : nullptr;
        a.gy = gy ? gy + i * (g_dist / 4) : nullptr;
        // Tile height: 64x32 tiles carry a sixth less halo, 64x16 give twice the workgroups.  What decides is whether the
        // LAUNCH fills the device, so the count is the launch's: this piece's images times the 64x32 tiles of one image,
        // against the f32 entry's 1024.  (The bits do not depend on the tile height.)
        a.tall = (size_t)tiles_x * cdiv(rows, 32) * ni >= 1024;
        MICV_TRY(harris_image_u8_launch(s, a, r, cpu));
        MICV_TRY(harris_nms_batch_launch(ctx, s, a.resp, a.resp_dist, rows, cols, a.rstride, threshold, min_distance,
                                         corners ? corners + i * (c_dist / 4) : nullptr, c_dist, cstride, masks, need_m / 8, ni));
        int32_t *li = locs_yx ? locs_yx + (size_t)i * cap * 2 : nullptr;
        float *ki = kp_xysa ? kp_xysa + (size_t)i * cap * 4 : nullptr;
        if (one_group) {
            harris_list_kernel<<<ni, kListThreads, 0, s>>>(masks, need_m / 8, (int)nseg, tiles_x, li, cap, count + i, a.img, img_dist, stride,
                                                          rows, cols, kp_size, cap > 0 ? ki : nullptr);
            MICV_LAUNCH_CHECK();
            continue;
        }
        // more words than one workgroup should walk: the list step of micv_harris_refine_dev, image by image
        for (int k = 0; k < ni; k++)
            MICV_TRY(harris_list_run(ctx, s, masks + (size_t)k * (need_m / 8), rows, cols, li ? li + (size_t)k * cap * 2 : nullptr, cap,
                                     count + i + k, list_scratch));
        if (ki && cap > 0) {
            harris_keypoints_counted_kernel<true><<<dim3((unsigned)((cap + 255) / 256), ni), 256, 0, s>>>(
                a.img, img_dist, stride, nullptr, nullptr, 0, rows, cols, li, cap, count + i, kp_size, ki);
            MICV_LAUNCH_CHECK();
        }
    }
    return MICV_OK;
}

}  // namespace micv

using namespace micv;

extern "C" {

int micv_harris_corners_u8_dev(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                               double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                               size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                               int64_t cap, int64_t *count, float kp_size, float *kp_xysa, micv_stream stream) {
    return harris_u8_common("micv_harris_corners_u8", ctx, img, 0, 1, rows, cols, stride, sobel_ksize, win, sigma, alpha, flags, threshold,
                            min_distance, gx, gy, 0, gstride, resp, 0, rstride, corners, 0, cstride, locs_yx, cap, count, kp_size, kp_xysa,
                            stream);
}

int micv_harris_corners_u8_batch_dev(micv_ctx *ctx, const uint8_t *img, size_t image_stride, int batch, int rows, int cols, size_t stride,
                                     int sobel_ksize, int win, double sigma, float alpha, int flags, double threshold, int min_distance,
                                     float *gx, float *gy, size_t gimage_stride, size_t gstride, float *resp, size_t rimage_stride,
                                     size_t rstride, float *corners, size_t cimage_stride, size_t cstride, int32_t *locs_yx, int64_t cap,
                                     int64_t *count, float kp_size, float *kp_xysa, micv_stream stream) {
    return harris_u8_common("micv_harris_corners_u8_batch", ctx, img, image_stride, batch, rows, cols, stride, sobel_ksize, win, sigma, alpha,
                            flags, threshold, min_distance, gx, gy, gimage_stride, gstride, resp, rimage_stride, rstride, corners,
                            cimage_stride, cstride, locs_yx, cap, count, kp_size, kp_xysa, stream);
}

int micv_harris_corners_u8_host(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                                double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                                size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                                int64_t cap, int64_t *count, float kp_size, float *kp_xysa) {
    HostCall h(ctx, "micv_harris_corners_u8_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && count && rows > 0 && cols > 0 && cap >= 0 && (locs_yx || cap == 0) && (!kp_xysa || locs_yx),
                 "micv_harris_corners_u8_host: bad argument");
    MICV_REQUIRE((gx == nullptr) == (gy == nullptr), "micv_harris_corners_u8_host: give both gradient outputs or neither");
    MICV_REQUIRE(stride >= (size_t)cols && (!gx || stride_ok(gstride, cols, 4)) && (!resp || stride_ok(rstride, cols, 4)) &&
                     (!corners || stride_ok(cstride, cols, 4)),
                 "micv_harris_corners_u8_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    // 1 B per pixel up (micv_harris_corners_host: 4), every requested field down
    uint8_t *di = h.up<uint8_t>(img, stride, (size_t)cols, rows);
    float *dgx = gx ? h.alloc<float>(n) : nullptr, *dgy = gy ? h.alloc<float>(n) : nullptr;
    float *dr = resp ? h.alloc<float>(n) : nullptr, *dc = corners ? h.alloc<float>(n) : nullptr;
    int32_t *dl = h.alloc<int32_t>((size_t)cap * 8);
    float *dk = kp_xysa ? h.alloc<float>((size_t)cap * 16) : nullptr;
    int64_t *dn = h.alloc<int64_t>(8);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "harrisCornersChain",
               micv_harris_corners_u8_dev(ctx, di, rows, cols, (size_t)cols, sobel_ksize, win, sigma, alpha, flags, threshold, min_distance,
                                          dgx, dgy, rb, dr, rb, dc, rb, dl, cap, dn, kp_size, dk, h.s));
    if (gx) {
        h.down(gx, gstride, dgx, rb, rows);
        h.down(gy, gstride, dgy, rb, rows);
    }
    if (resp) h.down(resp, rstride, dr, rb, rows);
    if (corners) h.down(corners, cstride, dc, rb, rows);
    h.down(count, dn, 8);
    MICV_TRY(h.finish());  // the count is here now
    const int64_t take = *count < cap ? *count : cap;
    if (take > 0) {
        h.down(locs_yx, dl, (size_t)take * 8);
        if (kp_xysa) h.down(kp_xysa, dk, (size_t)take * 16);
    }
    return h.finish();
}

}  // extern "C"
