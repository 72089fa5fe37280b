// canny_uf.hip -- sol::generateEdge without a host wait: the hysteresis as connected-component labelling with a lock-free
// union-find (hyst_uf.hpp has the algorithm and why its loops end), in a FIXED sequence of launches whatever the pixels
// are.  No word is read on the host, so the entries only enqueue: they can sit in a captured stream, and the image can be
// a grid dimension -- the batch.  canny.hip's polled entries stay as they are and give the same bytes: 8-connected
// hysteresis has one fixed point.
//   single image   launch_gauss_u8 (or the float front end of ps1.hip), canny_gradmap_kernel: canny.hip's kernels as they are
//   batch          the same two kernels with the image as grid.z (gauss_u8_batch_kernel, canny_gradmap_batch_kernel below:
//                  canny.hip's bodies behind a per-image offset; canny.hip itself has no image dimension)
//   then           hyst_init_kernel    a thread per word: every run of weak | strong is its own parent
//                  hyst_union_kernel   a thread per word: its runs united with their left and upper neighbours
//                  hyst_mark_kernel    a thread per word: its runs jump to their roots, one with a strong bit marks its root
//                  hyst_emit_kernel    a wave per word, a lane per pixel: 255 where the run's root is marked
//   byte masks     hyst_pack_kernel    a wave per word: the two ballots are the planes, run starts become their own parents
//                                      (pack takes init's place: four launches)
// No workgroup ever waits for another: no flag, no counter, no grid barrier.  Scratch per image: the blur plane (n bytes),
// the two bit planes (rows * cdiv(cols, 64) words each) and the parent plane (4 n bytes; only the slots of run starts are
// ever touched, so it is never cleared).  Labels are pixel indices within the image, the planes of image i lie i
// distances on, and no kernel forms an address from another image's index: nothing of one image can reach another.
#include "hyst_uf.hpp"
#include "kernels.hpp"

namespace micv {

// canny.hip's kernel, launched from here as it is
__global__ void canny_gradmap_kernel(const uint8_t *__restrict__ src, size_t stride, int rows, int cols, int low, int high,
                                     unsigned long long *__restrict__ weak, unsigned long long *__restrict__ strong, int tiles_x);
constexpr int UF_GM_TH = 16;  // its tile height (GM_TH)

struct DevAtomics {
    static __device__ uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ uint32_t fetch_min(uint32_t *p, uint32_t v) { return atomicMin(p, v); }
    static __device__ uint32_t ld(const uint32_t *p) { return *p; }
    static __device__ void st(uint32_t *p, uint32_t v) { *p = v; }
};

// The planes of a piece of a batch: image blockIdx.z is words_dist words / parent_dist slots on.
struct UfPlanes {
    unsigned long long *weak, *strong;
    uint32_t *parent;
    size_t words_dist, parent_dist;
    int rows, cols, tiles_x;
};

// one thread per word; false past the image's last word
struct UfWord {
    const unsigned long long *weak, *strong;
    uint32_t *parent;
    int w, y, tx;
    uint32_t id0;
    __device__ bool locate(const UfPlanes &p) {
        w = blockIdx.x * blockDim.x + threadIdx.x;
        if (w >= p.rows * p.tiles_x) return false;
        y = w / p.tiles_x;
        tx = w - y * p.tiles_x;
        weak = p.weak + blockIdx.z * p.words_dist;
        strong = p.strong + blockIdx.z * p.words_dist;
        parent = p.parent + blockIdx.z * p.parent_dist;
        id0 = (uint32_t)y * p.cols + tx * 64;
        return true;
    }
    __device__ unsigned long long F(int word) const { return weak[word] | strong[word]; }
};

__global__ __launch_bounds__(64) void hyst_init_kernel(UfPlanes p) {
    UfWord u;
    if (u.locate(p)) hyst::init_word<DevAtomics>(u.parent, u.F(u.w), u.id0);
}

__global__ __launch_bounds__(64) void hyst_union_kernel(UfPlanes p) {
    UfWord u;
    if (!u.locate(p)) return;
    const unsigned long long F = u.F(u.w);
    if (!F) return;
    const bool l = u.tx > 0, r = u.tx + 1 < p.tiles_x, up = u.y > 0;
    const int a = u.w - p.tiles_x;
    hyst::union_word<DevAtomics>(u.parent, F, l ? u.F(u.w - 1) : 0, up && l ? u.F(a - 1) : 0, up ? u.F(a) : 0, up && r ? u.F(a + 1) : 0,
                                 u.id0, (uint32_t)p.cols);
}

__global__ __launch_bounds__(64) void hyst_mark_kernel(UfPlanes p) {
    UfWord u;
    if (!u.locate(p)) return;
    const unsigned long long S = u.strong[u.w], F = u.weak[u.w] | S;
    if (F) hyst::mark_word<DevAtomics>(u.parent, F, S, u.id0);
}

// a wave is one word (the lanes' loads of it are one address), a lane one pixel; lanes of one run chase the same root
__global__ __launch_bounds__(256) void hyst_emit_kernel(UfPlanes p, uint8_t *__restrict__ edges, size_t edges_dist, size_t estride) {
    const int lane = threadIdx.x & 63, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.cols || y >= p.rows) return;
    const size_t w = blockIdx.z * p.words_dist + (size_t)y * p.tiles_x + blockIdx.x;
    const unsigned long long F = p.weak[w] | p.strong[w];
    const bool keep = (F >> lane & 1) && hyst::kept_bit<DevAtomics>(p.parent + blockIdx.z * p.parent_dist, F,
                                                                    (uint32_t)y * p.cols + blockIdx.x * 64, lane);
    edges[blockIdx.z * edges_dist + (size_t)y * estride + x] = keep ? 255 : 0;
}

// two byte masks (non-zero = set) -> the planes, and every run start its own parent
__global__ __launch_bounds__(256) void hyst_pack_kernel(const uint8_t *__restrict__ cand, size_t cstride, const uint8_t *__restrict__ strong,
                                                         size_t sstride, UfPlanes p) {
    const int lane = threadIdx.x & 63, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= p.rows) return;  // (wave-uniform)
    const bool in = x < p.cols;
    const unsigned long long W = __ballot(in && cand[(size_t)y * cstride + x] != 0), S = __ballot(in && strong[(size_t)y * sstride + x] != 0);
    const unsigned long long F = W | S;
    const uint32_t id = (uint32_t)y * p.cols + x;
    if ((F & ~(F << 1)) >> lane & 1) p.parent[id] = id;
    if (lane == 0) {
        p.weak[(size_t)y * p.tiles_x + blockIdx.x] = W;
        p.strong[(size_t)y * p.tiles_x + blockIdx.x] = S;
    }
}

// ---- the front end of a batch: gauss_u8_tiled_kernel and canny_gradmap_kernel of canny.hip, statement for statement,
// behind the offset of image blockIdx.z (src_dist, dst_dist in bytes; words_dist in words)
constexpr int UB_TW = 64, UB_TH = 16, UB_AMAX = 15;
__global__ __launch_bounds__(256) void gauss_u8_batch_kernel(const uint8_t *__restrict__ src, size_t src_dist, size_t stride, int rows,
                                                              int cols, Taps t, uint8_t *__restrict__ dst, size_t dst_dist, size_t dstride) {
    __shared__ uint8_t S[(UB_TH + 2 * UB_AMAX) * (UB_TW + 2 * UB_AMAX)];
    __shared__ float R[(UB_TH + 2 * UB_AMAX) * UB_TW];
    src += blockIdx.z * src_dist;
    dst += blockIdx.z * dst_dist;
    const int a = t.n / 2, RW = UB_TW + 2 * a, RH = UB_TH + 2 * a;
    const int x0 = blockIdx.x * UB_TW, y0 = blockIdx.y * UB_TH;
    for (int i = threadIdx.x; i < RH * RW; i += 256) {
        const int ly = i / RW, lx = i - ly * RW;
        S[i] = src[(size_t)reflect101(y0 - a + ly, rows) * stride + reflect101(x0 - a + lx, cols)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RH * UB_TW; i += 256) {
        const int ly = i / UB_TW, lx = i - ly * UB_TW;
        const uint8_t *s = S + ly * RW + lx;
        float acc = 0.f;
        for (int k = 0; k < t.n; k++) acc = fmaf((float)s[k], t.k[k], acc);
        R[i] = acc;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
    if (x >= cols) return;
    for (int ly = threadIdx.x >> 6; ly < UB_TH; ly += 4) {
        const int y = y0 + ly;
        if (y >= rows) break;
        float acc = 0.f;
        for (int k = 0; k < t.n; k++) acc = fmaf(R[(ly + k) * UB_TW + lx], t.k[k], acc);
        const int r = __float2int_rn(acc);
        dst[(size_t)y * dstride + x] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
}

__global__ __launch_bounds__(256) void canny_gradmap_batch_kernel(const uint8_t *__restrict__ src, size_t src_dist, size_t stride, int low,
                                                                   int high, UfPlanes p) {
    constexpr int TW = 64, TH = UF_GM_TH, PW = TW + 4, MW = TW + 2;
    __shared__ uint8_t P[(TH + 4) * PW];
    __shared__ int Mg[(TH + 2) * MW];
    src += blockIdx.z * src_dist;
    const int rows = p.rows, cols = p.cols;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int i = threadIdx.x; i < (TH + 4) * PW; i += 256) {
        const int ly = i / PW, lx = i - ly * PW;
        P[i] = src[(size_t)clampi(y0 - 2 + ly, 0, rows - 1) * stride + clampi(x0 - 2 + lx, 0, cols - 1)];
    }
    __syncthreads();
    auto sobel = [&](int py, int px, int &gx, int &gy) {
        const uint8_t *r0 = P + (py - 1) * PW + px, *r1 = r0 + PW, *r2 = r1 + PW;
        gx = (r0[1] + 2 * r1[1] + r2[1]) - (r0[-1] + 2 * r1[-1] + r2[-1]);
        gy = (r2[-1] + 2 * r2[0] + r2[1]) - (r0[-1] + 2 * r0[0] + r0[1]);
    };
    for (int i = threadIdx.x; i < (TH + 2) * MW; i += 256) {
        const int my = i / MW, mx = i - my * MW;
        const int gy_ = y0 - 1 + my, gx_ = x0 - 1 + mx;
        int m = 0;
        if ((unsigned)gy_ < (unsigned)rows && (unsigned)gx_ < (unsigned)cols) {
            int gx, gy;
            sobel(my + 1, mx + 1, gx, gy);
            m = abs(gx) + abs(gy);
        }
        Mg[i] = m;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, x = x0 + lx;
    for (int ly = threadIdx.x >> 6; ly < TH; ly += 4) {
        const int y = y0 + ly;
        if (y >= rows) break;
        int out = 0;
        if (x < cols) {
            const int *mc = Mg + (ly + 1) * MW + lx + 1;
            const int m = mc[0];
            if (m > low) {
                int xs, ys;
                sobel(ly + 2, lx + 2, xs, ys);
                xs = (short)xs;
                const int ax = abs(xs), ay = abs(ys) << 15;
                const int TG22 = 13573;
                const int tg22x = ax * TG22;
                bool is_max;
                if (ay < tg22x) {
                    is_max = m > mc[-1] && m >= mc[1];
                } else {
                    const int tg67x = tg22x + (ax << 16);
                    if (ay > tg67x) {
                        is_max = m > mc[-MW] && m >= mc[MW];
                    } else {
                        const int sgn = (xs ^ ys) < 0 ? -1 : 1;
                        is_max = m > mc[-MW - sgn] && m > mc[MW + sgn];
                    }
                }
                if (is_max) out = m > high ? 2 : 1;
            }
        }
        const unsigned long long w = __ballot(out == 1), st = __ballot(out == 2);
        if (lx == 0) {
            const size_t o = blockIdx.z * p.words_dist + (size_t)y * p.tiles_x + blockIdx.x;
            p.weak[o] = w;
            p.strong[o] = st;
        }
    }
}

// ---- host side
namespace {

// One image's share of the arena, and a piece of `images` carved from it: [blur][weak][strong][parent], each an array over
// the piece's images.
struct UfScratch {
    uint8_t *blur;
    UfPlanes p;
    size_t blur_dist;
};
size_t uf_per_image(int rows, int cols, bool blur) {
    const size_t n = (size_t)rows * cols, nwords = (size_t)rows * cdiv(cols, 64);
    return (blur ? Carver::need(n, 1) : 0) + Carver::need(nwords, 8) * 2 + Carver::need(n, 4);
}
int uf_reserve(micv_ctx *ctx, int rows, int cols, int images, bool blur, UfScratch *u) {
    const size_t n = (size_t)rows * cols, nwords = (size_t)rows * cdiv(cols, 64);
    void *scratch;
    MICV_TRY(ctx->reserve(uf_per_image(rows, cols, blur) * images + 256, &scratch));
    Carver c(scratch);
    u->blur_dist = Carver::need(n, 1);
    u->blur = blur ? c.take<uint8_t>(u->blur_dist * images) : nullptr;
    u->p.words_dist = Carver::need(nwords, 8) / 8;
    u->p.weak = c.take<unsigned long long>(u->p.words_dist * images);
    u->p.strong = c.take<unsigned long long>(u->p.words_dist * images);
    u->p.parent_dist = Carver::need(n, 4) / 4;
    u->p.parent = c.take<uint32_t>(u->p.parent_dist * images);
    u->p.rows = rows;
    u->p.cols = cols;
    u->p.tiles_x = cdiv(cols, 64);
    return MICV_OK;
}

// the planes of `images` images -> their edge bytes; packed: hyst_pack_kernel has made the parents already
int uf_hysteresis(hipStream_t s, const UfPlanes &p, int images, bool packed, uint8_t *edges, size_t edges_dist, size_t estride) {
    const dim3 words(cdiv(p.rows * p.tiles_x, 64), 1, images);
    if (!packed) {
        hyst_init_kernel<<<words, 64, 0, s>>>(p);
        MICV_LAUNCH_CHECK();
    }
    hyst_union_kernel<<<words, 64, 0, s>>>(p);
    MICV_LAUNCH_CHECK();
    hyst_mark_kernel<<<words, 64, 0, s>>>(p);
    MICV_LAUNCH_CHECK();
    hyst_emit_kernel<<<dim3(p.tiles_x, cdiv(p.rows, 4), images), 256, 0, s>>>(p, edges, edges_dist, estride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

void thresholds(double low_thresh, double high_thresh, int *lo, int *hi) {  // canny_from_u8's
    if (low_thresh > high_thresh) std::swap(low_thresh, high_thresh);
    *lo = (int)std::floor(low_thresh);
    *hi = (int)std::floor(high_thresh);
}

// ids are pixel indices below 2^31
bool uf_size_ok(int rows, int cols) { return (int64_t)rows * cols < (int64_t)1 << 31; }

bool gauss_ok(int n, double sigma) { return n >= 1 && n <= 31 && (n & 1) && sigma > 0; }

// the Canny stages on one blurred plane
int uf_canny_single(hipStream_t s, const uint8_t *cin, size_t cstride, const UfPlanes &p, double low_thresh, double high_thresh,
                    uint8_t *edges, size_t estride) {
    int lo, hi;
    thresholds(low_thresh, high_thresh, &lo, &hi);
    canny_gradmap_kernel<<<dim3(p.tiles_x, cdiv(p.rows, UF_GM_TH)), 256, 0, s>>>(cin, cstride, p.rows, p.cols, lo, hi, p.weak, p.strong,
                                                                                p.tiles_x);
    MICV_LAUNCH_CHECK();
    return uf_hysteresis(s, p, 1, false, edges, 0, estride);
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_hysteresis_u8_async(micv_ctx *ctx, const uint8_t *cand, size_t cstride, const uint8_t *strong, size_t sstride, int rows,
                             int cols, uint8_t *edges, size_t estride, micv_stream stream) {
    MICV_REQUIRE(ctx && cand && strong && edges, "micv_hysteresis_u8: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && cstride >= (size_t)cols && sstride >= (size_t)cols && estride >= (size_t)cols,
                 "micv_hysteresis_u8: bad size / stride");
    MICV_REQUIRE(uf_size_ok(rows, cols), "micv_hysteresis_u8: %d x %d is 2^31 pixels or more", rows, cols);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    UfScratch u;
    MICV_TRY(uf_reserve(ctx, rows, cols, 1, false, &u));
    hyst_pack_kernel<<<dim3(u.p.tiles_x, cdiv(rows, 4)), 256, 0, s>>>(cand, cstride, strong, sstride, u.p);
    MICV_LAUNCH_CHECK();
    return uf_hysteresis(s, u.p, 1, true, edges, 0, estride);
}

int micv_generate_edge_async(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride, int gauss_size, double gauss_sigma,
                             double low_thresh, double high_thresh, uint8_t *edges, size_t estride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && edges, "micv_generate_edge: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride >= (size_t)cols && estride >= (size_t)cols, "micv_generate_edge: bad size / stride");
    MICV_REQUIRE(gauss_ok(gauss_size, gauss_sigma), "micv_generate_edge: gaussian %d / sigma %g not supported (odd size <= 31, sigma > 0)",
                 gauss_size, gauss_sigma);
    MICV_REQUIRE(uf_size_ok(rows, cols), "micv_generate_edge_async: %d x %d is 2^31 pixels or more", rows, cols);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    UfScratch u;
    MICV_TRY(uf_reserve(ctx, rows, cols, 1, true, &u));
    const uint8_t *cin = src;
    size_t cstride = stride;
    if (gauss_size > 1) {  // a 1-tap Gaussian is the identity
        Taps t;
        gaussian_taps(gauss_size, gauss_sigma, &t);
        MICV_TRY(launch_gauss_u8(s, src, stride, rows, cols, t, u.blur, (size_t)cols));
        cin = u.blur;
        cstride = cols;
    }
    return uf_canny_single(s, cin, cstride, u.p, low_thresh, high_thresh, edges, estride);
}

int micv_generate_edge_f32_async(micv_ctx *ctx, const float *src, int rows, int cols, size_t stride, int gauss_size, double gauss_sigma,
                                 double low_thresh, double high_thresh, uint8_t *edges, size_t estride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && edges, "micv_generate_edge_f32: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride_ok(stride, cols, 4) && estride >= (size_t)cols, "micv_generate_edge_f32: bad size / stride");
    MICV_REQUIRE(gauss_ok(gauss_size, gauss_sigma), "micv_generate_edge_f32: gaussian %d / sigma %g not supported (odd size <= 31, sigma > 0)",
                 gauss_size, gauss_sigma);
    MICV_REQUIRE(uf_size_ok(rows, cols), "micv_generate_edge_f32_async: %d x %d is 2^31 pixels or more", rows, cols);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    UfScratch u;
    MICV_TRY(uf_reserve(ctx, rows, cols, 1, true, &u));
    Taps t;
    gaussian_taps(gauss_size, gauss_sigma, &t);
    MICV_TRY(launch_gauss_f32_to_u8(s, src, stride, rows, cols, t, u.blur, (size_t)cols));
    return uf_canny_single(s, u.blur, (size_t)cols, u.p, low_thresh, high_thresh, edges, estride);
}

int micv_generate_edge_batch_async(micv_ctx *ctx, const uint8_t *src, int batch, size_t image_bytes, int rows, int cols, size_t stride,
                                   int gauss_size, double gauss_sigma, double low_thresh, double high_thresh, uint8_t *edges,
                                   size_t edges_image_bytes, size_t estride, int scratch_mb, micv_stream stream) {
    MICV_REQUIRE(ctx && src && edges, "micv_generate_edge_batch: null argument");
    MICV_REQUIRE(batch >= 1 && scratch_mb >= 0, "micv_generate_edge_batch: batch %d, scratch_mb %d", batch, scratch_mb);
    MICV_REQUIRE(rows > 0 && cols > 0 && stride >= (size_t)cols && estride >= (size_t)cols, "micv_generate_edge_batch: bad size / stride");
    MICV_REQUIRE(gauss_ok(gauss_size, gauss_sigma), "micv_generate_edge_batch: gaussian %d / sigma %g not supported (odd size <= 31, sigma > 0)",
                 gauss_size, gauss_sigma);
    MICV_REQUIRE(uf_size_ok(rows, cols), "micv_generate_edge_batch: %d x %d is 2^31 pixels or more", rows, cols);
    // an image is the (rows - 1) * pitch + cols bytes from its first pixel
    MICV_REQUIRE(batch == 1 || (image_bytes >= (size_t)(rows - 1) * stride + cols && edges_image_bytes >= (size_t)(rows - 1) * estride + cols),
                 "micv_generate_edge_batch: the images of a batch overlap (image_bytes %zu, edges_image_bytes %zu)", image_bytes,
                 edges_image_bytes);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // Pieces: a piece's scratch stays within the bound -- one image at least, 65535 (grid.z) at most.
    const size_t bound = (size_t)(scratch_mb ? scratch_mb : 64) << 20, per_image = uf_per_image(rows, cols, true);
    size_t piece = bound / per_image < 1 ? 1 : bound / per_image;
    if (piece > 65535) piece = 65535;
    if (piece > (size_t)batch) piece = batch;
    UfScratch u;
    MICV_TRY(uf_reserve(ctx, rows, cols, (int)piece, true, &u));
    Taps t;
    if (gauss_size > 1) gaussian_taps(gauss_size, gauss_sigma, &t);
    int lo, hi;
    thresholds(low_thresh, high_thresh, &lo, &hi);
    for (int i = 0; i < batch; i += (int)piece) {
        const int ni = batch - i < (int)piece ? batch - i : (int)piece;
        const uint8_t *cin = src + i * image_bytes;
        size_t cdist = image_bytes, cstride = stride;
        if (gauss_size > 1) {
            gauss_u8_batch_kernel<<<dim3(cdiv(cols, UB_TW), cdiv(rows, UB_TH), ni), 256, 0, s>>>(cin, cdist, cstride, rows, cols, t, u.blur,
                                                                                               u.blur_dist, (size_t)cols);
            MICV_LAUNCH_CHECK();
            cin = u.blur;
            cdist = u.blur_dist;
            cstride = cols;
        }
        canny_gradmap_batch_kernel<<<dim3(u.p.tiles_x, cdiv(rows, UF_GM_TH), ni), 256, 0, s>>>(cin, cdist, cstride, lo, hi, u.p);
        MICV_LAUNCH_CHECK();
        MICV_TRY(uf_hysteresis(s, u.p, ni, false, edges + i * edges_image_bytes, edges_image_bytes, estride));
    }
    return MICV_OK;
}

}  // extern "C"
