// ps3.hip -- the drawing that the ps3 driver does after the geometry (ProblemSets/ps3_cpp/src/Solution.cpp:122-158,
// drawEpipolarLines; called from runProblem2 and runExtraCredit, :323-481): cv::line from P_iL to P_iR for every epipolar
// line, on the device, from the end points where micv_epipolar_endpoints_dev left them.
// The contract is the host loop of the shim, micv_ps3::line_wide (shim/micv_ps3.hpp): micv_viz::line's walk with its
// integers as wide as they need to be, so that every pair of int32 end points is walked exactly; DESIGN.md section 2
// ("ps3 driver"), PARITY WITH OPENCV'S RASTERISER UNPINNED.  Nothing here synchronises the host or reads an end point on
// the host.
//
// One wave per segment, one lane per step of the walk whose major coordinate is in the image (ps3_lane.hpp, over the
// wide walk of draw.hpp).  All strokes
// share one colour, so crossing strokes store equal bytes: no owner plane and no atomics, as in ps6.hip.
#include <climits>
#include <cmath>
#include <initializer_list>

#include "common.hpp"
#include "host_io.hpp"
#include "epipolar.hpp"
#include "ps3_lane.hpp"

namespace micv {
namespace {

constexpr int kSegThreads = 256, kWave = 64, kSegWaves = kSegThreads / kWave;

// Segment k: (p[k pitch], p[k pitch + 1]) -> (p[k pitch + off2], p[k pitch + off2 + 1]).
struct SegJob {
    draw::Target t;
    uint32_t colour;  // draw::pack_colour
    const float *p;
    int n, pitch, off2;
};

__global__ void __launch_bounds__(kSegThreads) ps3_segments_kernel(const SegJob job) {
    const long long k = (long long)blockIdx.x * kSegWaves + threadIdx.x / kWave;
    if (k >= job.n) return;
    const float *e = job.p + (size_t)k * job.pitch;
    seg_lane(job.t, job.colour, e[0], e[1], e[job.off2], e[job.off2 + 1], threadIdx.x % kWave, kWave);
}

// Both pictures of runProblem2 / runExtraCredit in one launch: waves 0 .. n - 1 draw the lines of image B's points in
// image A (side 0), waves n .. 2n - 1 the lines of image A's points in image B (side 1).  Each wave computes its end points
// with the device function of micv_epipolar_endpoints_dev (every lane the same values) and walks them at once.
struct DisplayJob {
    draw::Target a, b;
    uint32_t colour;
    const float *F, *ptsA, *ptsB;  // F 3 x 3; the points n x {x, y}
    int n, f64;
    float *ends;  // [2][n][6] or null
};

__global__ void __launch_bounds__(kSegThreads) ps3_display_kernel(const DisplayJob job) {
    const long long k = (long long)blockIdx.x * kSegWaves + threadIdx.x / kWave;
    if (k >= 2LL * job.n) return;
    const int side = k >= job.n, lane = threadIdx.x % kWave;
    const size_t i = (size_t)(side ? k - job.n : k);
    const float *p = (side ? job.ptsA : job.ptsB) + 2 * i;
    const draw::Target &t = side ? job.b : job.a;
    float e[6];
    if (job.f64) epipolar_endpoints<double>(job.F, p[0], p[1], side, t.rows, t.cols, e);
    else epipolar_endpoints<float>(job.F, p[0], p[1], side, t.rows, t.cols, e);
    if (job.ends && lane == 0)
        for (int c = 0; c < 6; c++) job.ends[((size_t)side * job.n + i) * 6 + c] = e[c];
    seg_lane(t, job.colour, e[0], e[1], e[3], e[4], lane, kWave);
}

// draw.hpp's check with this file's largest side, and a stride that fits 32 bits
bool image_ok(int rows, int cols, int ch, size_t stride) {
    return draw::image_ok(rows, cols, ch, stride, 32768) && stride < (size_t)1 << 32;
}

int check_args(const char *fn, micv_ctx *ctx, const uint8_t *img, int rows, int cols, int ch, size_t stride, const float *p, int n,
               const double *color) {
    MICV_REQUIRE(ctx && img && color && n >= 0 && n <= 1 << 28 && (n == 0 || p), "%s: null argument or n = %d outside 0 .. 2^28", fn, n);
    MICV_REQUIRE(ch == 1 || ch == 3 || ch == 4, "%s: %d channels not supported (1, 3, 4)", fn, ch);
    MICV_REQUIRE(image_ok(rows, cols, ch, stride), "%s: bad size %dx%d (1..32768) or stride %zu", fn, rows, cols, stride);
    return MICV_OK;
}

int launch_segments(micv_ctx *ctx, uint8_t *img, int rows, int cols, int ch, size_t stride, const float *p, int n, int pitch, int off2,
                    const double *color, hipStream_t s) {
    if (n == 0) return MICV_OK;
    MICV_HIP(hipSetDevice(ctx->device));
    SegJob job{};
    job.t = draw::Target{img, stride, rows, cols, ch}, job.colour = draw::pack_colour(color);
    job.p = p, job.n = n, job.pitch = pitch, job.off2 = off2;
    ps3_segments_kernel<<<cdiv((unsigned)n, kSegWaves), kSegThreads, 0, s>>>(job);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

// upload, the same launch, download, synchronise; the padding of the caller's rows is never read or written
int segments_host(const char *fn, micv_ctx *ctx, uint8_t *img, int rows, int cols, int ch, size_t stride, const float *p, int n, int pitch, int off2,
                  const double *color) {
    if (n == 0) return MICV_OK;
    HostCall h(ctx, fn);
    const size_t rb = (size_t)cols * ch;
    uint8_t *di = h.up<uint8_t>(img, stride, rb, rows);
    float *dp = h.up<float>(p, (size_t)n * pitch * sizeof(float));
    if (!h.ok()) return h.finish();
    MICV_TRY(launch_segments(ctx, di, rows, cols, ch, rb, dp, n, pitch, off2, color, h.s));
    h.down(img, stride, di, rb, rows);
    return h.finish();
}

struct Picture {
    const uint8_t *src;
    size_t sstride;
    int rows, cols;
    uint8_t *out;
    size_t ostride;
};

int check_display(const char *fn, micv_ctx *ctx, const float *F, const float *ptsA, const float *ptsB, int n, const Picture &a,
                  const Picture &b, int ch, uint32_t flags, const double *color) {
    MICV_REQUIRE(ctx && F && ptsA && ptsB && a.src && a.out && b.src && b.out && color, "%s: null argument", fn);
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && n >= 1 && n <= 1 << 27, "%s: bad flags %u or n = %d outside 1 .. 2^27", fn, flags, n);
    MICV_REQUIRE(ch == 1 || ch == 3 || ch == 4, "%s: %d channels not supported (1, 3, 4)", fn, ch);
    for (const Picture *p : {&a, &b}) {
        MICV_REQUIRE(image_ok(p->rows, p->cols, ch, p->sstride) && image_ok(p->rows, p->cols, ch, p->ostride),
                     "%s: bad size %dx%d (1..32768) or stride %zu / %zu", fn, p->rows, p->cols, p->sstride, p->ostride);
        MICV_REQUIRE(p->out != p->src || p->ostride == p->sstride, "%s: in place, but the strides differ", fn);
    }
    MICV_REQUIRE(a.out != b.out, "%s: the two outputs are one image", fn);
    return MICV_OK;
}

// the copies first (unless in place), then the one launch
int enqueue_display(micv_ctx *ctx, const float *F, const float *ptsA, const float *ptsB, int n, const Picture &a, const Picture &b, int ch,
                    uint32_t flags, const double *color, float *ends, hipStream_t s) {
    MICV_HIP(hipSetDevice(ctx->device));
    for (const Picture *p : {&a, &b})
        if (p->out != p->src)
            MICV_HIP(hipMemcpy2DAsync(p->out, p->ostride, p->src, p->sstride, (size_t)p->cols * ch, p->rows, hipMemcpyDeviceToDevice, s));
    DisplayJob job{};
    job.a = draw::Target{a.out, a.ostride, a.rows, a.cols, ch};
    job.b = draw::Target{b.out, b.ostride, b.rows, b.cols, ch};
    job.colour = draw::pack_colour(color);
    job.F = F, job.ptsA = ptsA, job.ptsB = ptsB, job.n = n, job.f64 = (flags & MICV_GEOM_F64) ? 1 : 0, job.ends = ends;
    ps3_display_kernel<<<cdiv(2u * (unsigned)n, kSegWaves), kSegThreads, 0, s>>>(job);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_draw_segments_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *segments, int n,
                           const double *color, micv_stream stream) {
    MICV_TRY(check_args("micv_draw_segments_dev", ctx, img, rows, cols, channels, stride, segments, n, color));
    return launch_segments(ctx, img, rows, cols, channels, stride, segments, n, 4, 2, color, static_cast<hipStream_t>(stream));
}

int micv_draw_segments_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *segments, int n,
                            const double *color) {
    MICV_TRY(check_args("micv_draw_segments_host", ctx, img, rows, cols, channels, stride, segments, n, color));
    return segments_host("micv_draw_segments_host", ctx, img, rows, cols, channels, stride, segments, n, 4, 2, color);
}

int micv_draw_epipolar_lines_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *endpoints,
                                 int n, const double *color, micv_stream stream) {
    MICV_TRY(check_args("micv_draw_epipolar_lines_dev", ctx, img, rows, cols, channels, stride, endpoints, n, color));
    return launch_segments(ctx, img, rows, cols, channels, stride, endpoints, n, 6, 3, color, static_cast<hipStream_t>(stream));
}

int micv_draw_epipolar_lines_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *endpoints,
                                  int n, const double *color) {
    MICV_TRY(check_args("micv_draw_epipolar_lines_host", ctx, img, rows, cols, channels, stride, endpoints, n, color));
    return segments_host("micv_draw_epipolar_lines_host", ctx, img, rows, cols, channels, stride, endpoints, n, 6, 3, color);
}

int micv_ps3_epipolar_display_dev(micv_ctx *ctx, const float *F, const float *ptsA, const float *ptsB, int n, const uint8_t *imgA,
                                  size_t astride, int rowsA, int colsA, const uint8_t *imgB, size_t bstride, int rowsB, int colsB,
                                  int channels, uint32_t flags, const double *color, uint8_t *outA, size_t oastride, uint8_t *outB,
                                  size_t obstride, float *endpoints, micv_stream stream) {
    const Picture a{imgA, astride, rowsA, colsA, outA, oastride}, b{imgB, bstride, rowsB, colsB, outB, obstride};
    MICV_TRY(check_display("micv_ps3_epipolar_display_dev", ctx, F, ptsA, ptsB, n, a, b, channels, flags, color));
    return enqueue_display(ctx, F, ptsA, ptsB, n, a, b, channels, flags, color, endpoints, static_cast<hipStream_t>(stream));
}

int micv_ps3_epipolar_display_host(micv_ctx *ctx, const float *F, const float *ptsA, const float *ptsB, int n, const uint8_t *imgA,
                                   size_t astride, int rowsA, int colsA, const uint8_t *imgB, size_t bstride, int rowsB, int colsB,
                                   int channels, uint32_t flags, const double *color, uint8_t *outA, size_t oastride, uint8_t *outB,
                                   size_t obstride, float *endpoints) {
    const Picture a{imgA, astride, rowsA, colsA, outA, oastride}, b{imgB, bstride, rowsB, colsB, outB, obstride};
    MICV_TRY(check_display("micv_ps3_epipolar_display_host", ctx, F, ptsA, ptsB, n, a, b, channels, flags, color));
    HostCall h(ctx, "micv_ps3_epipolar_display_host");
    const size_t rba = (size_t)colsA * channels, rbb = (size_t)colsB * channels, pb = (size_t)n * 2 * sizeof(float),
                 eb = (size_t)n * 12 * sizeof(float);
    uint8_t *da = h.up<uint8_t>(imgA, astride, rba, rowsA), *db = h.up<uint8_t>(imgB, bstride, rbb, rowsB);
    float *dpa = h.up<float>(ptsA, pb), *dpb = h.up<float>(ptsB, pb), *dF = h.up<float>(F, 9 * sizeof(float));
    float *de = endpoints ? h.alloc<float>(eb) : nullptr;
    if (!h.ok()) return h.finish();
    const Picture ua{da, rba, rowsA, colsA, da, rba}, ub{db, rbb, rowsB, colsB, db, rbb};
    MICV_TRY(enqueue_display(ctx, dF, dpa, dpb, n, ua, ub, channels, flags, color, de, h.s));
    h.down(outA, oastride, da, rba, rowsA);
    h.down(outB, obstride, db, rbb, rowsB);
    if (endpoints) h.down(endpoints, de, eb);
    return h.finish();
}

}  // extern "C"
