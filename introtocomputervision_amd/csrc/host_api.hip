// host_api.hip -- `_host` flavours: host pointers in, host pointers out, synchronous.  Every one of them is its
// argument checks around upload -> `_dev` call -> download; the plumbing is HostCall (host_io.hpp).
#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "host_io.hpp"

namespace micv {
std::atomic<micv_kernel_log_fn> g_log_fn{nullptr};
std::atomic<void *> g_log_user{nullptr};
}  // namespace micv

using namespace micv;

extern "C" {

int micv_set_kernel_log(micv_kernel_log_fn fn, void *user) {
    g_log_user.store(user, std::memory_order_relaxed);
    g_log_fn.store(fn, std::memory_order_release);
    return MICV_OK;
}

int micv_lk_flow_pyr_host(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                          size_t stride, int win, int levels, float *u, float *v, size_t ostride) {
    HostCall h(ctx, "micv_lk_flow_pyr_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(prev && next && u && v && rows > 0 && cols > 0, "micv_lk_flow_pyr_host: bad argument");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && stride_ok(ostride, cols, 4),
                 "micv_lk_flow_pyr_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    float *dp = h.up<float>(prev, stride, rb, rows), *dn = h.up<float>(next, stride, rb, rows);
    float *du = h.alloc<float>(n), *dv = h.alloc<float>(n);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_lk_flow_pyr_dev(ctx, dp, dn, rows, cols, rb, win, levels, du, dv, rb, h.s));
    h.down(u, ostride, du, rb, rows);
    h.down(v, ostride, dv, rb, rows);
    return h.finish();
}

/* lk::calcOpticalFlowPyr on frames as the ps5 driver hands them over (denseLKWrapper passes the
 * COLOUR frames, Solution.cpp:63; makeGaussianPyramid converts, Pyramids.cpp:9-15): one upload of
 * the interleaved frames, grey conversion on the device, then the pyramid chain. */
int micv_lk_flow_pyr_frames_host(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols,
                                 size_t stride, int channels, int depth, int win, int levels, float *u,
                                 float *v, size_t ostride) {
    HostCall h(ctx, "micv_lk_flow_pyr_frames_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(prev && next && u && v && rows > 0 && cols > 0, "micv_lk_flow_pyr_frames_host: bad argument");
    MICV_REQUIRE((channels == 1 || channels == 3 || channels == 4) &&
                     (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F),
                 "micv_lk_flow_pyr_frames_host: frames must be 1/3/4-channel 8U or 32F");
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)cols * channels * es;
    MICV_REQUIRE(stride >= srb && stride_ok(ostride, cols, 4), "micv_lk_flow_pyr_frames_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    void *cp = h.up<void>(prev, stride, srb, rows), *cn = h.up<void>(next, stride, srb, rows);
    float *dp = h.alloc<float>(n), *dn = h.alloc<float>(n), *du = h.alloc<float>(n), *dv = h.alloc<float>(n);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_to_gray_f32_dev(ctx, cp, rows, cols, srb, channels, depth, dp, rb, h.s));
    MICV_TRY(micv_to_gray_f32_dev(ctx, cn, rows, cols, srb, channels, depth, dn, rb, h.s));
    MICV_TRY(micv_lk_flow_pyr_dev(ctx, dp, dn, rows, cols, rb, win, levels, du, dv, rb, h.s));
    h.down(u, ostride, du, rb, rows);
    h.down(v, ostride, dv, rb, rows);
    return h.finish();
}

/* lk::calcOpticalFlowPyr over a SEQUENCE of frames -- pairs (0, 1), (1, 2), ... as the ps5 driver walks a directory
 * (ps5_cpp/lib/Config.cpp:17-46, src/Solution.cpp:255-285: frame t is `next` of one call and `prev` of the following one).
 * A per-pair `_host` call moves four images over PCIe one after the other around its kernels (0.745 ms per 1080p pair,
 * r05).  Here every frame is uploaded ONCE, and the legs run side by side:
 *   upload     frame t + 2 -> raw block -> grey f32 (device conversion), ring of three frames; the calling thread
 *   compute    pair t + 1: the pyramid chain (micv_lk_flow_pyr_dev) on its own stream, ring of three flow outputs
 *   download   pair t: u, v -> the caller's buffers, a thread and a stream of their own
 * The caller's images are pageable memory, and a copy from / to pageable memory occupies the thread that issues it
 * (streams alone do not overlap such copies: tools/probes/pcie_probe.py) -- hence the download thread.  What r06 tried
 * instead and measured slower per 1080p f32 pair (profiles/r06/host_sequence.md): registering the caller's images in place
 * (hipHostRegister: a fresh registration costs 0.07 ms per image and serialises with the transfers in flight, 0.71 ms),
 * pinned staging rings with host copies on three threads (a host copy into / out of pinned memory runs at 30 GB/s here,
 * 0.27 ms per image: 0.65 ms).  Same bits as the per-pair calls.
 * The HostCall gives the blocks and the copy; the streams are the pipeline's own.  It is declared first, so it goes last:
 * the blocks return to the cache after Scope has drained every stream. */
int micv_lk_flow_seq_host(micv_ctx *ctx, const void *const *frames, int nframes, int rows, int cols, size_t stride,
                          int channels, int depth, int win, int levels, float *const *u, float *const *v,
                          size_t ostride) {
    MICV_REQUIRE(ctx != nullptr, "micv_lk_flow_seq_host: ctx is null");
    MICV_REQUIRE(frames && u && v && nframes >= 2 && rows > 0 && cols > 0, "micv_lk_flow_seq_host: bad argument");
    MICV_REQUIRE((channels == 1 || channels == 3 || channels == 4) && (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F),
                 "micv_lk_flow_seq_host: frames must be 1/3/4-channel 8U or 32F");
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)cols * channels * es;
    MICV_REQUIRE(stride >= srb && stride_ok(ostride, cols, 4), "micv_lk_flow_seq_host: bad stride");
    for (int t = 0; t < nframes; t++) MICV_REQUIRE(frames[t] != nullptr, "micv_lk_flow_seq_host: frame %d is null", t);
    for (int t = 0; t + 1 < nframes; t++) MICV_REQUIRE(u[t] && v[t], "micv_lk_flow_seq_host: output %d is null", t);
    HostCall h(ctx, "micv_lk_flow_seq_host");
    const bool convert = !(channels == 1 && depth == MICV_DEPTH_32F);
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    constexpr int RING = 3;
    void *raw = h.alloc<void>(convert ? srb * rows : 256);
    float *grey[RING], *du[RING], *dv[RING];
    for (auto *ring : {grey, du, dv})
        for (int i = 0; i < RING; i++) ring[i] = h.alloc<float>(n);
    if (!h.ok()) return h.finish();
    const int npairs = nframes - 1;
    auto copy = [rows](void *dst, size_t dstride, const void *src, size_t sstride, size_t row_bytes, hipMemcpyKind kind,
                       hipStream_t stream) -> int {
        MICV_HIP(HostCall::copy2d(dst, dstride, src, sstride, row_bytes, rows, kind, stream));
        return MICV_OK;
    };

    struct Scope {  // released on every way out, after everything enqueued has finished
        hipStream_t up = nullptr, run = nullptr, down[2] = {nullptr, nullptr};
        std::vector<hipEvent_t> ev;
        ~Scope() {
            for (hipStream_t st : {up, run, down[0], down[1]})
                if (st) (void)hipStreamSynchronize(st);
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
            for (hipStream_t st : {up, run, down[0], down[1]})
                if (st) (void)hipStreamDestroy(st);
        }
    } st;
    MICV_HIP(hipStreamCreateWithFlags(&st.up, hipStreamNonBlocking));
    MICV_HIP(hipStreamCreateWithFlags(&st.run, hipStreamNonBlocking));
    MICV_HIP(hipStreamCreateWithFlags(&st.down[0], hipStreamNonBlocking));
    MICV_HIP(hipStreamCreateWithFlags(&st.down[1], hipStreamNonBlocking));
    st.ev.reserve((size_t)nframes + (size_t)npairs);
    auto new_event = [&](hipEvent_t *e) -> int {
        MICV_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        st.ev.push_back(*e);
        return MICV_OK;
    };
    std::vector<hipEvent_t> ev_up(nframes), ev_pair(npairs);
    for (auto &e : ev_up) MICV_TRY(new_event(&e));
    for (auto &e : ev_pair) MICV_TRY(new_event(&e));

    // The download threads: pair p's field is copied out once its chain has finished.  `enqueued` / `done[]` order them
    // against the calling thread: a flow block is written again only after its previous content has reached the caller.
    std::mutex mu;
    std::condition_variable cv;
    int enqueued = 0, done[2] = {0, 0};
    bool stop = false, failed = false;
    char down_err[256] = "";
    auto download = [&](int which) {
        (void)hipSetDevice(ctx->device);
        for (int p = 0; p < npairs; p++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return enqueued > p || stop; });
                if (enqueued <= p) return;  // the calling thread gave up
            }
            int rc = hipStreamWaitEvent(st.down[which], ev_pair[p], 0) == hipSuccess ? MICV_OK : MICV_EHIP;
            if (rc == MICV_OK) rc = copy(u[p], ostride, du[p % RING], rb, rb, hipMemcpyDeviceToHost, st.down[which]);
            if (rc == MICV_OK) rc = copy(v[p], ostride, dv[p % RING], rb, rb, hipMemcpyDeviceToHost, st.down[which]);
            if (rc == MICV_OK && hipStreamSynchronize(st.down[which]) != hipSuccess) rc = MICV_EHIP;
            std::lock_guard<std::mutex> lk(mu);
            if (rc != MICV_OK && !failed) {
                failed = true;
                snprintf(down_err, sizeof(down_err), "micv_lk_flow_seq_host: download of pair %d failed: %s", p, micv_last_error());
            }
            done[0] = done[1] = p + 1;
            cv.notify_all();
        }
    };
    // (ONE thread for both fields: two -- a stream and a thread per field -- measured slower, 0.48-0.52 against 0.45 ms
    // per pair: copies to pageable memory do not overlap each other either)
    std::thread tu;
    try {
        tu = std::thread(download, 0);
    } catch (const std::exception &e) {  // (no thread to be had: nothing has been enqueued for it yet)
        set_error("micv_lk_flow_seq_host: cannot start the download thread: %s", e.what());
        return MICV_EHIP;
    }
    struct Joiner {  // (declared after Scope: runs first -- the thread is gone before its stream is)
        std::thread &a; std::mutex &mu; std::condition_variable &cv; bool &stop;
        ~Joiner() {
            { std::lock_guard<std::mutex> lk(mu); stop = true; }
            cv.notify_all();
            if (a.joinable()) a.join();
        }
    } joiner{tu, mu, cv, stop};

    for (int t = 0; t < nframes; t++) {
        // frame t takes the grey block frame t - 3 had: pairs t - 4 and t - 3 read that one
        if (t >= RING) MICV_HIP(hipStreamWaitEvent(st.up, ev_pair[t - RING], 0));
        if (convert) {
            MICV_TRY(copy(raw, srb, frames[t], stride, srb, hipMemcpyHostToDevice, st.up));
            MICV_TRY(micv_to_gray_f32_dev(ctx, raw, rows, cols, srb, channels, depth, grey[t % RING], rb, st.up));
        } else {
            MICV_TRY(copy(grey[t % RING], rb, frames[t], stride, rb, hipMemcpyHostToDevice, st.up));
        }
        MICV_HIP(hipEventRecord(ev_up[t], st.up));
        if (t == 0) continue;
        const int p = t - 1;
        if (p >= RING) {  // the flow blocks pair p - 3 used must have reached the caller
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return (done[0] >= p - RING + 1 && done[1] >= p - RING + 1) || failed; });
            if (failed) break;
        }
        MICV_HIP(hipStreamWaitEvent(st.run, ev_up[t], 0));  // (frame t - 1: earlier on the same streams)
        MICV_TRY(micv_lk_flow_pyr_dev(ctx, grey[p % RING], grey[t % RING], rows, cols, rb, win, levels, du[p % RING],
                                      dv[p % RING], rb, st.run));
        MICV_HIP(hipEventRecord(ev_pair[p], st.run));
        {
            std::lock_guard<std::mutex> lk(mu);
            enqueued = p + 1;
        }
        cv.notify_all();
    }
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return (done[0] >= enqueued && done[1] >= enqueued) || failed; });
        if (failed) {
            set_error("%s", down_err);
            return MICV_EHIP;
        }
        if (enqueued < npairs) return MICV_EHIP;  // (unreachable: every early way out returns above)
    }
    return MICV_OK;
}

int micv_to_gray_f32_host(micv_ctx *ctx, const void *src, int rows, int cols, size_t sstride, int channels,
                          int depth, float *dst, size_t dstride) {
    HostCall h(ctx, "micv_to_gray_f32_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0, "micv_to_gray_f32_host: bad argument");
    MICV_REQUIRE((channels == 1 || channels == 3 || channels == 4) &&
                     (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F),
                 "micv_to_gray_f32_host: source must be 1/3/4-channel 8U or 32F");
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)cols * channels * es;
    MICV_REQUIRE(sstride >= srb && stride_ok(dstride, cols, 4), "micv_to_gray_f32_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    void *cs = h.up<void>(src, sstride, srb, rows);
    float *dd = h.alloc<float>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_to_gray_f32_dev(ctx, cs, rows, cols, srb, channels, depth, dd, rb, h.s));
    h.down(dst, dstride, dd, rb, rows);
    return h.finish();
}

int micv_lk_flow_host(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                      size_t stride, int win, float *u, float *v, size_t ostride) {
    HostCall h(ctx, "micv_lk_flow_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(prev && next && u && v && rows > 0 && cols > 0, "micv_lk_flow_host: bad argument");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && stride_ok(ostride, cols, 4),
                 "micv_lk_flow_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    float *dp = h.up<float>(prev, stride, rb, rows), *dn = h.up<float>(next, stride, rb, rows);
    float *du = h.alloc<float>(n), *dv = h.alloc<float>(n);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_lk_flow_dev(ctx, dp, dn, rows, cols, rb, win, du, dv, rb, h.s));
    h.down(u, ostride, du, rb, rows);
    h.down(v, ostride, dv, rb, rows);
    return h.finish();
}

int micv_lk_warp_host(micv_ctx *ctx, const float *src, size_t sstride, const float *du,
                      const float *dv, size_t fstride, int rows, int cols, float *dst,
                      size_t dstride) {
    HostCall h(ctx, "micv_lk_warp_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && du && dv && dst && rows > 0 && cols > 0, "micv_lk_warp_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(fstride, cols, 4) &&
                     stride_ok(dstride, cols, 4),
                 "micv_lk_warp_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    float *ds = h.up<float>(src, sstride, rb, rows), *dU = h.up<float>(du, fstride, rb, rows);
    float *dV = h.up<float>(dv, fstride, rb, rows), *dd = h.alloc<float>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_lk_warp_dev(ctx, ds, rb, dU, dV, rb, rows, cols, dd, rb, h.s));
    h.down(dst, dstride, dd, rb, rows);
    return h.finish();
}

int micv_pyr_down_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                       float *dst, size_t dstride) {
    HostCall h(ctx, "micv_pyr_down_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0, "micv_pyr_down_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(dstride, cols / 2, 4),
                 "micv_pyr_down_host: bad stride");
    const int dr = rows / 2, dc = cols / 2;
    float *ds = h.up<float>(src, sstride, (size_t)cols * 4, rows), *dd = h.alloc<float>((size_t)dr * dc * 4);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "pyrDownsampleKernel", micv_pyr_down_dev(ctx, ds, rows, cols, (size_t)cols * 4, dd, (size_t)dc * 4, h.s));
    if (dr > 0 && dc > 0) h.down(dst, dstride, dd, (size_t)dc * 4, dr);
    return h.finish();
}

int micv_pyr_up_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                     float *dst, size_t dstride) {
    HostCall h(ctx, "micv_pyr_up_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0, "micv_pyr_up_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(dstride, 2 * cols, 4),
                 "micv_pyr_up_host: bad stride");
    float *ds = h.up<float>(src, sstride, (size_t)cols * 4, rows), *dd = h.alloc<float>((size_t)rows * cols * 16);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "pyrUpsampleKernel", micv_pyr_up_dev(ctx, ds, rows, cols, (size_t)cols * 4, dd, (size_t)cols * 8, h.s));
    h.down(dst, dstride, dd, (size_t)cols * 8, 2 * rows);
    return h.finish();
}

int micv_gaussian_pyramid_host(micv_ctx *ctx, const float *src, int rows, int cols,
                               size_t sstride, int levels, float *const *dst_levels) {
    HostCall h(ctx, "micv_gaussian_pyramid_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst_levels && rows > 0 && cols > 0, "micv_gaussian_pyramid_host: bad argument");
    MICV_REQUIRE(levels >= 1 && levels <= 16 && (rows >> (levels - 1)) > 0 &&
                     (cols >> (levels - 1)) > 0,
                 "micv_gaussian_pyramid_host: %d levels do not fit a %dx%d image", levels, rows,
                 cols);
    MICV_REQUIRE(stride_ok(sstride, cols, 4), "micv_gaussian_pyramid_host: bad stride");
    size_t total = 0, off[16];
    for (int l = 0; l < levels; l++) {
        off[l] = total;
        total += (((size_t)(rows >> l) * (cols >> l)) + 63) & ~size_t(63);
    }
    float *ds = h.up<float>(src, sstride, (size_t)cols * 4, rows), *dd = h.alloc<float>(total * 4);
    if (!h.ok()) return h.finish();
    float *lv[16];
    for (int l = 0; l < levels; l++) lv[l] = dd + off[l];
    MICV_TRY(micv_gaussian_pyramid_dev(ctx, ds, rows, cols, (size_t)cols * 4, levels, lv, h.s));
    for (int l = 0; l < levels; l++) {
        MICV_REQUIRE(dst_levels[l] != nullptr, "micv_gaussian_pyramid_host: dst_levels[%d] is null", l);
        h.down(dst_levels[l], lv[l], (size_t)(rows >> l) * (cols >> l) * 4);
    }
    return h.finish();
}

int micv_sobel_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                    int ksize, float scale, float *gx, float *gy, size_t gstride) {
    HostCall h(ctx, "micv_sobel_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && gx && gy && rows > 0 && cols > 0, "micv_sobel_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(gstride, cols, 4),
                 "micv_sobel_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    float *ds = h.up<float>(src, sstride, rb, rows), *dx = h.alloc<float>(n), *dy = h.alloc<float>(n);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_sobel_dev(ctx, ds, rows, cols, rb, ksize, scale, dx, dy, rb, h.s));
    h.down(gx, gstride, dx, rb, rows);
    h.down(gy, gstride, dy, rb, rows);
    return h.finish();
}

}  // extern "C"

// ---- ps4 / ps2 / ps1 host flavours -----------------------------------------------------------
extern "C" {

int micv_harris_response_ex_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                                 size_t gstride, int win, double sigma, float alpha, int flags, float *resp,
                                 size_t rstride) {
    HostCall h(ctx, "micv_harris_response_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(gx && gy && resp && rows > 0 && cols > 0, "micv_harris_response_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4) && stride_ok(rstride, cols, 4),
                 "micv_harris_response_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    float *dx = h.up<float>(gx, gstride, rb, rows), *dy = h.up<float>(gy, gstride, rb, rows), *dr = h.alloc<float>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "cornerResponseKernel",
               micv_harris_response_ex_dev(ctx, dx, dy, rows, cols, rb, win, sigma, alpha, flags, dr, rb, h.s));
    h.down(resp, rstride, dr, rb, rows);
    return h.finish();
}

int micv_harris_response_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                              size_t gstride, int win, double sigma, float alpha, float *resp,
                              size_t rstride) {
    return micv_harris_response_ex_host(ctx, gx, gy, rows, cols, gstride, win, sigma, alpha, 0, resp, rstride);
}

int micv_harris_refine_host(micv_ctx *ctx, const float *resp, int rows, int cols, size_t rstride,
                            double threshold, int min_distance, float *corners, size_t cstride,
                            int32_t *locs_yx, int64_t cap, int64_t *count) {
    HostCall h(ctx, "micv_harris_refine_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(resp && corners && count && rows > 0 && cols > 0 && cap >= 0,
                 "micv_harris_refine_host: bad argument");
    MICV_REQUIRE(stride_ok(rstride, cols, 4) && stride_ok(cstride, cols, 4),
                 "micv_harris_refine_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    float *dr = h.up<float>(resp, rstride, rb, rows), *dc = h.alloc<float>(rb * rows);
    int32_t *dl = h.alloc<int32_t>((size_t)cap * 8);
    int64_t *dn = h.alloc<int64_t>(8);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "refineCornersKernel",
               micv_harris_refine_dev(ctx, dr, rows, cols, rb, threshold, min_distance, dc, rb, dl, cap, dn, h.s));
    h.down(corners, cstride, dc, rb, rows);
    h.down(count, dn, 8);
    MICV_TRY(h.finish());  // the count is here now
    const int64_t take = *count < cap ? *count : cap;
    if (take > 0) h.down(locs_yx, dl, (size_t)take * 8);
    return h.finish();
}

int micv_harris_corners_host(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                             double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                             size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                             int64_t cap, int64_t *count) {
    HostCall h(ctx, "micv_harris_corners_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && count && rows > 0 && cols > 0 && cap >= 0 && (locs_yx || cap == 0), "micv_harris_corners_host: bad argument");
    MICV_REQUIRE((gx == nullptr) == (gy == nullptr), "micv_harris_corners_host: give both gradient outputs or neither");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && (!gx || stride_ok(gstride, cols, 4)) && (!resp || stride_ok(rstride, cols, 4)) &&
                     (!corners || stride_ok(cstride, cols, 4)),
                 "micv_harris_corners_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    // one upload, every requested field downloaded: what three _host calls move three times
    float *di = h.up<float>(img, stride, rb, rows);
    float *dgx = gx ? h.alloc<float>(n) : nullptr, *dgy = gy ? h.alloc<float>(n) : nullptr;
    float *dr = resp ? h.alloc<float>(n) : nullptr, *dc = corners ? h.alloc<float>(n) : nullptr;
    int32_t *dl = h.alloc<int32_t>((size_t)cap * 8);
    int64_t *dn = h.alloc<int64_t>(8);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "harrisCornersChain",
               micv_harris_corners_dev(ctx, di, rows, cols, rb, sobel_ksize, win, sigma, alpha, flags, threshold, min_distance, dgx, dgy, rb,
                                       dr, rb, dc, rb, dl, cap, dn, h.s));
    if (gx) {
        h.down(gx, gstride, dgx, rb, rows);
        h.down(gy, gstride, dgy, rb, rows);
    }
    if (resp) h.down(resp, rstride, dr, rb, rows);
    if (corners) h.down(corners, cstride, dc, rb, rows);
    h.down(count, dn, 8);
    MICV_TRY(h.finish());  // the count is here now
    const int64_t take = *count < cap ? *count : cap;
    if (take > 0) h.down(locs_yx, dl, (size_t)take * 8);
    return h.finish();
}

int micv_sift_angles_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                          size_t gstride, float *angles, size_t astride) {
    HostCall h(ctx, "micv_sift_angles_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(gx && gy && angles && rows > 0 && cols > 0, "micv_sift_angles_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4) && stride_ok(astride, cols, 4),
                 "micv_sift_angles_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    float *dx = h.up<float>(gx, gstride, rb, rows), *dy = h.up<float>(gy, gstride, rb, rows), *da = h.alloc<float>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_sift_angles_dev(ctx, dx, dy, rows, cols, rb, da, rb, h.s));
    h.down(angles, astride, da, rb, rows);
    return h.finish();
}

int micv_sift_keypoints_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                             size_t gstride, const int32_t *locs_yx, int64_t n, float size,
                             float *kp_xysa) {
    HostCall h(ctx, "micv_sift_keypoints_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(gx && gy && rows > 0 && cols > 0 && n >= 0 && (n == 0 || (locs_yx && kp_xysa)),
                 "micv_sift_keypoints_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4), "micv_sift_keypoints_host: bad stride");
    for (int64_t i = 0; i < n; i++)
        MICV_REQUIRE((unsigned)locs_yx[2 * i] < (unsigned)rows && (unsigned)locs_yx[2 * i + 1] < (unsigned)cols,
                     "micv_sift_keypoints_host: corner %lld outside the image", (long long)i);
    if (n == 0) return MICV_OK;
    const size_t rb = (size_t)cols * 4;
    float *dx = h.up<float>(gx, gstride, rb, rows), *dy = h.up<float>(gy, gstride, rb, rows);
    int32_t *dl = h.up<int32_t>(locs_yx, (size_t)n * 8);
    float *dk = h.alloc<float>((size_t)n * 16);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_sift_keypoints_dev(ctx, dx, dy, rows, cols, rb, dl, n, size, dk, h.s));
    h.down(kp_xysa, dk, (size_t)n * 16);
    return h.finish();
}

int micv_sift_descriptors_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                               size_t gstride, const float *kp_xysa, int64_t n, float *desc,
                               size_t dstride) {
    HostCall h(ctx, "micv_sift_descriptors_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(gx && gy && rows > 0 && cols > 0 && n >= 0 && (n == 0 || (kp_xysa && desc)),
                 "micv_sift_descriptors_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4) && dstride % 4 == 0 && dstride >= 512,
                 "micv_sift_descriptors_host: bad stride");
    if (n == 0) return MICV_OK;
    const size_t rb = (size_t)cols * 4;
    float *dx = h.up<float>(gx, gstride, rb, rows), *dy = h.up<float>(gy, gstride, rb, rows);
    float *dk = h.up<float>(kp_xysa, (size_t)n * 16), *dd = h.alloc<float>((size_t)n * 512);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_sift_descriptors_dev(ctx, dx, dy, rows, cols, rb, dk, n, dd, 512, h.s));
    h.down(desc, dstride, dd, 512, (int)n);
    return h.finish();
}

static int stereo_host(bool ncc, micv_ctx *ctx, const float *left, const float *right, int rows,
                       int cols, size_t stride, int rad, int min_d, int max_d, int flags,
                       int8_t *disp, size_t dstride) {
    HostCall h(ctx, "micv_disparity_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(left && right && disp && rows > 0 && cols > 0, "micv_disparity_host: bad argument");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && dstride >= (size_t)cols, "micv_disparity_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    float *dl = h.up<float>(left, stride, rb, rows), *dr = h.up<float>(right, stride, rb, rows);
    int8_t *dd = h.alloc<int8_t>((size_t)rows * cols);
    if (!h.ok()) return h.finish();
    if (ncc)
        MICV_TIMED(h, "disparityNCorrKernel",
                   micv_disparity_ncorr_dev(ctx, dl, dr, rows, cols, rb, rad, min_d, max_d, flags, dd, cols, h.s));
    else
        MICV_TIMED(h, "disparitySSDKernel",
                   micv_disparity_ssd_dev(ctx, dl, dr, rows, cols, rb, rad, min_d, max_d, flags, dd, cols, h.s));
    h.down(disp, dstride, dd, (size_t)cols, rows);
    return h.finish();
}

int micv_disparity_ssd_host(micv_ctx *ctx, const float *left, const float *right, int rows,
                            int cols, size_t stride, int window_rad, int min_disparity,
                            int max_disparity, int flags, int8_t *disp, size_t dstride) {
    return stereo_host(false, ctx, left, right, rows, cols, stride, window_rad, min_disparity,
                       max_disparity, flags, disp, dstride);
}
int micv_disparity_ncorr_host(micv_ctx *ctx, const float *left, const float *right, int rows,
                              int cols, size_t stride, int window_rad, int min_disparity,
                              int max_disparity, int flags, int8_t *disp, size_t dstride) {
    return stereo_host(true, ctx, left, right, rows, cols, stride, window_rad, min_disparity,
                       max_disparity, flags, disp, dstride);
}

// 1 B per pixel and image up, where the f32 entries send 4
static int stereo_u8_host(bool ncc, const char *fn, micv_ctx *ctx, const uint8_t *left, size_t lstride, const uint8_t *right,
                          size_t rstride, int rows, int cols, int rad, int min_d, int max_d, int flags, int8_t *disp, size_t dstride) {
    HostCall h(ctx, fn);
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(left && right && disp && rows > 0 && cols > 0, "%s: null argument or bad size", fn);
    MICV_REQUIRE(lstride >= (size_t)cols && rstride >= (size_t)cols && dstride >= (size_t)cols, "%s: bad stride", fn);
    const size_t rb = (size_t)cols;
    uint8_t *dl = h.up<uint8_t>(left, lstride, rb, rows), *dr = h.up<uint8_t>(right, rstride, rb, rows);
    int8_t *dd = h.alloc<int8_t>(rb * rows);
    if (!h.ok()) return h.finish();
    if (ncc)
        MICV_TIMED(h, "disparityNCorrKernel",
                   micv_disparity_ncorr_u8_dev(ctx, dl, rb, dr, rb, rows, cols, rad, min_d, max_d, flags, dd, rb, h.s));
    else
        MICV_TIMED(h, "disparitySSDKernel",
                   micv_disparity_ssd_u8_dev(ctx, dl, rb, dr, rb, rows, cols, rad, min_d, max_d, flags, dd, rb, h.s));
    h.down(disp, dstride, dd, rb, rows);
    return h.finish();
}
int micv_disparity_ssd_u8_host(micv_ctx *ctx, const uint8_t *left, size_t lstride, const uint8_t *right, size_t rstride,
                               int rows, int cols, int window_rad, int min_disparity, int max_disparity, int flags,
                               int8_t *disp, size_t dstride) {
    return stereo_u8_host(false, "micv_disparity_ssd_u8_host", ctx, left, lstride, right, rstride, rows, cols, window_rad,
                          min_disparity, max_disparity, flags, disp, dstride);
}
int micv_disparity_ncorr_u8_host(micv_ctx *ctx, const uint8_t *left, size_t lstride, const uint8_t *right, size_t rstride,
                                 int rows, int cols, int window_rad, int min_disparity, int max_disparity, int flags,
                                 int8_t *disp, size_t dstride) {
    return stereo_u8_host(true, "micv_disparity_ncorr_u8_host", ctx, left, lstride, right, rstride, rows, cols, window_rad,
                          min_disparity, max_disparity, flags, disp, dstride);
}

int micv_hough_lines_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                          unsigned rho_bin, unsigned theta_bin, int32_t *acc) {
    HostCall h(ctx, "micv_hough_lines_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(mask && acc && mstride >= (size_t)cols, "micv_hough_lines_host: bad argument");
    int rb, tb;
    MICV_TRY(micv_hough_lines_dims(rows, cols, rho_bin, theta_bin, &rb, &tb));
    uint8_t *dm = h.up<uint8_t>(mask, mstride, (size_t)cols, rows);
    int32_t *da = h.alloc<int32_t>((size_t)rb * tb * 4);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "houghLinesAccumulateKernel", micv_hough_lines_dev(ctx, dm, rows, cols, cols, rho_bin, theta_bin, da, h.s));
    h.down(acc, da, (size_t)rb * tb * 4);
    return h.finish();
}

int micv_hough_circles_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols,
                            size_t mstride, unsigned radius, int32_t *acc) {
    HostCall h(ctx, "micv_hough_circles_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(mask && acc && rows > 0 && cols > 0 && mstride >= (size_t)cols,
                 "micv_hough_circles_host: bad argument");
    uint8_t *dm = h.up<uint8_t>(mask, mstride, (size_t)cols, rows);
    int32_t *da = h.alloc<int32_t>((size_t)rows * cols * 4);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "houghCirclesAccumulateKernel", micv_hough_circles_dev(ctx, dm, rows, cols, cols, radius, da, h.s));
    h.down(acc, da, (size_t)rows * cols * 4);
    return h.finish();
}

int micv_hough_peaks_host(micv_ctx *ctx, const int32_t *acc, int rows, int cols,
                          unsigned num_peaks, int threshold, uint32_t *peaks_rc, int64_t *count) {
    HostCall h(ctx, "micv_hough_peaks_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(acc && count && rows > 0 && cols > 0 && (peaks_rc || num_peaks == 0),
                 "micv_hough_peaks_host: bad argument");
    MICV_REQUIRE((int64_t)rows * cols < ((int64_t)1 << 31) && num_peaks <= 4096,  // before the upload
                 "micv_hough_peaks_host: %dx%d accumulator / %u peaks not supported (< 2^31 cells, <= 4096 peaks)",
                 rows, cols, num_peaks);
    int32_t *da = h.up<int32_t>(acc, (size_t)rows * cols * 4);
    uint32_t *dp = h.alloc<uint32_t>((size_t)num_peaks * 8 + 8);
    int64_t *dn = h.alloc<int64_t>(8);
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "findLocalMaximaKernel", micv_hough_peaks_dev(ctx, da, rows, cols, num_peaks, threshold, dp, dn, h.s));
    h.down(count, dn, 8);
    MICV_TRY(h.finish());  // the count is here now
    if (*count > 0) h.down(peaks_rc, dp, (size_t)*count * 8);
    return h.finish();
}

// ---- host-pointer flavours of the "next" rows --------------------------

int micv_generate_edge_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride,
                            int gauss_size, double gauss_sigma, double low_thresh,
                            double high_thresh, uint8_t *edges, size_t estride) {
    HostCall h(ctx, "micv_generate_edge_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && edges && rows > 0 && cols > 0 && stride >= (size_t)cols && estride >= (size_t)cols,
                 "micv_generate_edge_host: bad argument");
    uint8_t *ds = h.up<uint8_t>(src, stride, (size_t)cols, rows), *de = h.alloc<uint8_t>((size_t)rows * cols);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_generate_edge_dev(ctx, ds, rows, cols, cols, gauss_size, gauss_sigma, low_thresh, high_thresh, de, cols, h.s));
    h.down(edges, estride, de, (size_t)cols, rows);
    return h.finish();
}

int micv_bf_knn2_host(micv_ctx *ctx, const float *query, int nq, size_t qstride, const float *train,
                      int nt, size_t tstride, int dim, int32_t *idx2, float *dist2) {
    HostCall h(ctx, "micv_bf_knn2_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(query && train && idx2 && dist2 && nq > 0 && nt >= 2 && dim > 0 &&
                     stride_ok(qstride, dim, 4) && stride_ok(tstride, dim, 4),
                 "micv_bf_knn2_host: bad argument");
    const size_t rb = (size_t)dim * 4;
    float *dq = h.up<float>(query, qstride, rb, nq), *dt = h.up<float>(train, tstride, rb, nt);
    int32_t *di = h.alloc<int32_t>((size_t)nq * 8);
    float *dd = h.alloc<float>((size_t)nq * 8);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_bf_knn2_dev(ctx, dq, nq, rb, dt, nt, rb, dim, di, dd, h.s));
    h.down(idx2, di, (size_t)nq * 8);
    h.down(dist2, dd, (size_t)nq * 8);
    return h.finish();
}

int micv_bf_ratio_filter_host(micv_ctx *ctx, const int32_t *idx2, const float *dist2, int nq,
                              double ratio, int32_t *matches_qt, float *distances, int64_t cap,
                              int64_t *count) {
    HostCall h(ctx, "micv_bf_ratio_filter_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(idx2 && dist2 && count && nq > 0 && cap >= 0 && (cap == 0 || (matches_qt && distances)),
                 "micv_bf_ratio_filter_host: bad argument");
    int32_t *di = h.up<int32_t>(idx2, (size_t)nq * 8);
    float *dd = h.up<float>(dist2, (size_t)nq * 8);
    int32_t *dm = h.alloc<int32_t>((size_t)cap * 8 + 8);
    float *dl = h.alloc<float>((size_t)cap * 4 + 8);
    int64_t *dn = h.alloc<int64_t>(8);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_bf_ratio_filter_dev(ctx, di, dd, nq, ratio, dm, dl, cap, dn, h.s));
    h.down(count, dn, 8);
    MICV_TRY(h.finish());  // the count is here now
    const int64_t n = *count < cap ? *count : cap;
    if (n > 0) {
        h.down(matches_qt, dm, (size_t)n * 8);
        h.down(distances, dl, (size_t)n * 4);
    }
    return h.finish();
}

int micv_ransac_solve_host(micv_ctx *ctx, const float *src_xy, const float *dst_xy, int64_t n,
                           const int32_t *samples, int iters, int type, int thresh, double min_ratio,
                           float *transforms, uint8_t *inlier_mask, int32_t *stats) {
    HostCall h(ctx, "micv_ransac_solve_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src_xy && dst_xy && samples && transforms && inlier_mask && stats,
                 "micv_ransac_solve_host: null argument");
    // the argument rules of the device entry point, checked before anything is uploaded
    MICV_REQUIRE(type >= MICV_RANSAC_TRANSLATION && type <= MICV_RANSAC_AFFINE && iters >= 1 && n >= type &&
                     n <= (int64_t)1 << 30 && thresh >= 0 && min_ratio == min_ratio,
                 "micv_ransac_solve_host: bad type %d, iters %d, n = %lld, threshold %d or min_ratio", type, iters,
                 (long long)n, thresh);
    const size_t ns = (size_t)iters * type;
    for (size_t i = 0; i < ns; i++)
        MICV_REQUIRE(samples[i] >= 0 && samples[i] < n, "micv_ransac_solve_host: sample %lld = %d outside [0, %lld)",
                     (long long)i, samples[i], (long long)n);
    float *dsrc = h.up<float>(src_xy, (size_t)n * 8), *ddst = h.up<float>(dst_xy, (size_t)n * 8);
    int32_t *dsam = h.up<int32_t>(samples, ns * 4);
    float *dt = h.alloc<float>(48);
    uint8_t *dm = h.alloc<uint8_t>((size_t)n);
    int32_t *dst = h.alloc<int32_t>(12);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_ransac_solve_dev(ctx, dsrc, ddst, n, dsam, iters, type, thresh, min_ratio, dt, dm, dst, h.s));
    h.down(transforms, dt, 48);
    h.down(inlier_mask, dm, (size_t)n);
    h.down(stats, dst, 12);
    return h.finish();
}

int micv_mhi_frame_difference_host(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows,
                                   int cols, size_t stride, double thresh, int blur_w, int blur_h,
                                   double blur_sigma, uint8_t *diff, size_t dstride) {
    HostCall h(ctx, "micv_mhi_frame_difference_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(f1 && f2 && diff && rows > 0 && cols > 0 && stride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_frame_difference_host: bad argument");
    const size_t rb = (size_t)cols;
    uint8_t *d1 = h.up<uint8_t>(f1, stride, rb, rows), *d2 = h.up<uint8_t>(f2, stride, rb, rows), *dd = h.alloc<uint8_t>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mhi_frame_difference_dev(ctx, d1, d2, rows, cols, cols, thresh, blur_w, blur_h, blur_sigma, dd, cols, h.s));
    h.down(diff, dstride, dd, rb, rows);
    return h.finish();
}

int micv_mhi_energy_host(micv_ctx *ctx, const uint8_t *mhi, int rows, int cols, size_t sstride,
                         uint8_t *mei, size_t dstride) {
    HostCall h(ctx, "micv_mhi_energy_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(mhi && mei && rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_energy_host: bad argument");
    const size_t rb = (size_t)cols;
    uint8_t *ds = h.up<uint8_t>(mhi, sstride, rb, rows), *dd = h.alloc<uint8_t>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mhi_energy_dev(ctx, ds, rows, cols, cols, dd, cols, h.s));
    h.down(mei, dstride, dd, rb, rows);
    return h.finish();
}

int micv_mhi_threshold_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride,
                            double thresh, uint8_t *dst, size_t dstride) {
    HostCall h(ctx, "micv_mhi_threshold_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_threshold_host: bad argument");
    const size_t rb = (size_t)cols;
    uint8_t *ds = h.up<uint8_t>(src, sstride, rb, rows), *dd = h.alloc<uint8_t>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mhi_threshold_dev(ctx, ds, rows, cols, cols, thresh, dd, cols, h.s));
    h.down(dst, dstride, dd, rb, rows);
    return h.finish();
}

int micv_mhi_update_host(micv_ctx *ctx, uint8_t *history, size_t hstride, const uint8_t *mask,
                         size_t mstride, int rows, int cols, int tau) {
    HostCall h(ctx, "micv_mhi_update_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(history && mask && rows > 0 && cols > 0 && hstride >= (size_t)cols && mstride >= (size_t)cols,
                 "micv_mhi_update_host: bad argument");
    const size_t rb = (size_t)cols;
    uint8_t *dh = h.up<uint8_t>(history, hstride, rb, rows), *dm = h.up<uint8_t>(mask, mstride, rb, rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mhi_update_dev(ctx, dh, cols, dm, cols, rows, cols, tau, h.s));
    h.down(history, hstride, dh, rb, rows);
    return h.finish();
}


int micv_mhi_history_seq_host(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride,
                              int rows, int cols, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                              const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride) {
    HostCall h(ctx, "micv_mhi_history_seq_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(frames && save && out && nframes >= 2 && nsave >= 1 && rows > 0 && cols > 0 &&
                     stride >= (size_t)cols && frame_pitch >= stride * (size_t)rows && out_stride >= (size_t)cols &&
                     (nsave == 1 || out_pitch >= out_stride * (size_t)rows),
                 "micv_mhi_history_seq_host: bad argument");
    const size_t n = (size_t)rows * cols;
    uint8_t *df = h.alloc<uint8_t>(n * nframes), *dout = h.alloc<uint8_t>(n * nsave);
    for (int f = 0; f < nframes; f++) h.up_to(df + n * f, frames + (size_t)f * frame_pitch, stride, (size_t)cols, rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mhi_history_seq_dev(ctx, df, nframes, n, cols, rows, cols, thresh, blur_w, blur_h, blur_sigma, tau, save, nsave,
                                      dout, n, cols, h.s));
    for (int i = 0; i < nsave; i++) h.down(out + (size_t)i * out_pitch, out_stride, dout + n * i, (size_t)cols, rows);
    return h.finish();
}

int micv_mhi_frame_difference_c_host(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows, int cols, int channels,
                                     size_t stride, double thresh, int blur_w, int blur_h, double blur_sigma, uint8_t *diff,
                                     size_t dstride) {
    HostCall h(ctx, "micv_mhi_frame_difference_c_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_mhi_frame_difference_c_host: channels %d (1, 3 or 4)", channels);
    MICV_REQUIRE(f1 && f2 && diff && rows > 0 && cols > 0 && dstride >= (size_t)cols, "micv_mhi_frame_difference_c_host: bad argument");
    MICV_REQUIRE(stride >= (size_t)cols * channels, "micv_mhi_frame_difference_c_host: stride %zu < cols * channels = %zu", stride,
                 (size_t)cols * channels);
    const size_t rb = (size_t)cols * channels;
    uint8_t *d1 = h.up<uint8_t>(f1, stride, rb, rows), *d2 = h.up<uint8_t>(f2, stride, rb, rows), *dd = h.alloc<uint8_t>((size_t)cols * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mhi_frame_difference_c_dev(ctx, d1, d2, rows, cols, channels, rb, thresh, blur_w, blur_h, blur_sigma, dd, cols, h.s));
    h.down(diff, dstride, dd, (size_t)cols, rows);
    return h.finish();
}

int micv_mhi_history_seq_c_host(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride, int rows,
                                int cols, int channels, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                                const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride,
                                const int *save_diff, int nsave_diff, uint8_t *diff_out, size_t diff_pitch, size_t diff_stride) {
    HostCall h(ctx, "micv_mhi_history_seq_c_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_mhi_history_seq_c_host: channels %d (1, 3 or 4)", channels);
    MICV_REQUIRE(frames && nframes >= 2 && rows > 0 && cols > 0 && nsave >= 0 && nsave_diff >= 0 && nsave + nsave_diff >= 1 &&
                     (nsave == 0 || (save && out)) && (nsave_diff == 0 || (save_diff && diff_out)),
                 "micv_mhi_history_seq_c_host: bad argument");
    MICV_REQUIRE(stride >= (size_t)cols * channels && frame_pitch >= stride * (size_t)rows,
                 "micv_mhi_history_seq_c_host: stride %zu < cols * channels, or frame_pitch below a frame", stride);
    MICV_REQUIRE((nsave == 0 || (out_stride >= (size_t)cols && (nsave == 1 || out_pitch >= out_stride * (size_t)rows))) &&
                     (nsave_diff == 0 || (diff_stride >= (size_t)cols && (nsave_diff == 1 || diff_pitch >= diff_stride * (size_t)rows))),
                 "micv_mhi_history_seq_c_host: bad output stride / pitch");
    const size_t rb = (size_t)cols * channels, nf = rb * rows, n = (size_t)rows * cols;
    uint8_t *df = h.alloc<uint8_t>(nf * nframes), *dout = h.alloc<uint8_t>(n * (nsave ? nsave : 1)),
            *ddiff = h.alloc<uint8_t>(n * (nsave_diff ? nsave_diff : 1));
    for (int f = 0; f < nframes; f++) h.up_to(df + nf * f, frames + (size_t)f * frame_pitch, stride, rb, rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_mhi_history_seq_c_dev(ctx, df, nframes, nf, rb, rows, cols, channels, thresh, blur_w, blur_h, blur_sigma, tau, save,
                                        nsave, dout, n, cols, save_diff, nsave_diff, ddiff, n, cols, h.s));
    for (int i = 0; i < nsave; i++) h.down(out + (size_t)i * out_pitch, out_stride, dout + n * i, (size_t)cols, rows);
    for (int i = 0; i < nsave_diff; i++) h.down(diff_out + (size_t)i * diff_pitch, diff_stride, ddiff + n * i, (size_t)cols, rows);
    return h.finish();
}

int micv_central_moments_host(micv_ctx *ctx, const void *imgs, int batch, size_t img_pitch, size_t stride, int rows,
                              int cols, int type, const int *orders, int n, uint32_t flags, float *mu, float *eta,
                              float *raw) {
    HostCall h(ctx, "micv_central_moments_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(imgs && orders && mu && eta && batch > 0 && rows > 0 && cols > 0 && n >= 1 &&
                     n <= MICV_MOMENTS_MAX_ORDERS && (type == MICV_MOMENTS_U8 || type == MICV_MOMENTS_F32),
                 "micv_central_moments_host: bad argument");
    const size_t elem = type == MICV_MOMENTS_F32 ? 4 : 1, row_bytes = (size_t)cols * elem;
    MICV_REQUIRE(stride >= row_bytes && (batch == 1 || img_pitch >= stride * (size_t)rows),
                 "micv_central_moments_host: bad stride / pitch");
    const size_t img = row_bytes * rows;
    uint8_t *di = h.alloc<uint8_t>(img * batch);
    float *dmu = h.alloc<float>(sizeof(float) * (size_t)batch * (2 * n + 3));
    for (int b = 0; b < batch; b++)
        h.up_to(di + img * b, static_cast<const uint8_t *>(imgs) + (size_t)b * img_pitch, stride, row_bytes, rows);
    if (!h.ok()) return h.finish();
    float *deta = dmu + (size_t)batch * n, *draw = deta + (size_t)batch * n;
    MICV_TRY(micv_central_moments_dev(ctx, di, batch, img, row_bytes, rows, cols, type, orders, n, flags, dmu, deta, draw, h.s));
    h.down(mu, dmu, sizeof(float) * batch * n);
    h.down(eta, deta, sizeof(float) * batch * n);
    if (raw) h.down(raw, draw, sizeof(float) * batch * 3);
    return h.finish();
}

int micv_knn_predict_host(micv_ctx *ctx, const float *train, int ntrain, size_t train_stride, const int *train_labels,
                          const float *test, int ntest, size_t test_stride, int dims, int k, uint32_t flags, int *pred) {
    HostCall h(ctx, "micv_knn_predict_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(train && train_labels && test && pred && ntrain >= 1 && ntest >= 1 && dims >= 1 &&
                     dims <= MICV_KNN_MAX_DIMS && train_stride >= sizeof(float) * dims &&
                     test_stride >= sizeof(float) * dims,
                 "micv_knn_predict_host: bad argument");
    const size_t rb = sizeof(float) * dims;
    float *dt = h.up<float>(train, train_stride, rb, ntrain);
    int *dl = h.up<int>(train_labels, sizeof(int) * ntrain);
    float *dq = h.up<float>(test, test_stride, rb, ntest);
    int *dp = h.alloc<int>(sizeof(int) * ntest);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_knn_predict_dev(ctx, dt, ntrain, rb, dl, dq, ntest, rb, dims, k, flags, dp, h.s));
    h.down(pred, dp, sizeof(int) * ntest);
    return h.finish();
}

int micv_knn_confusion_host(micv_ctx *ctx, const float *features, int n, size_t stride, int dims, const int *labels,
                            const int *groups, int num_labels, int num_groups, int k, uint32_t flags, float *confusion,
                            int *pred, int *left_out) {
    HostCall h(ctx, "micv_knn_confusion_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(features && labels && confusion && n >= 1 && dims >= 1 && dims <= MICV_KNN_MAX_DIMS &&
                     stride >= sizeof(float) * dims && num_labels >= 1 && num_labels <= MICV_KNN_MAX_LABELS &&
                     (!groups || (num_groups >= 1 && num_groups <= MICV_KNN_MAX_GROUPS)),
                 "micv_knn_confusion_host: bad argument");
    const size_t rb = sizeof(float) * dims;
    const int nmat = groups ? num_groups + 1 : 1;
    const size_t mat_bytes = sizeof(float) * (size_t)nmat * num_labels * num_labels;
    float *df = h.up<float>(features, stride, rb, n);
    int *dl = h.up<int>(labels, sizeof(int) * n), *dg = groups ? h.up<int>(groups, sizeof(int) * n) : nullptr;
    int *dp = h.alloc<int>(sizeof(int) * n);
    float *dm = h.alloc<float>(mat_bytes + sizeof(int));
    if (!h.ok()) return h.finish();
    int *dleft = reinterpret_cast<int *>(reinterpret_cast<char *>(dm) + mat_bytes);
    MICV_TRY(micv_knn_confusion_dev(ctx, df, n, rb, dims, dl, dg, num_labels, num_groups, k, flags, dm, dp, dleft, h.s));
    h.down(confusion, dm, mat_bytes);
    if (pred) h.down(pred, dp, sizeof(int) * n);
    if (left_out) h.down(left_out, dleft, sizeof(int));
    return h.finish();
}

// ps3: geometry.  The index lists are checked here, before anything is uploaded.
static int geom_indices_ok(const char *fn, const int32_t *indices, int stride, int T, const int32_t *kcount, int k,
                           int j, int n) {
    if (!indices) return MICV_OK;
    for (int t = 0; t < T; t++) {
        const int kc = kcount ? kcount[t] : k;
        MICV_REQUIRE(kc >= 0 && kc <= k, "%s: kcount[%d] = %d outside [0, %d]", fn, t, kc, k);
        for (int i = 0; i < kc + j; i++) {
            const int32_t v = indices[(size_t)t * stride + i];
            MICV_REQUIRE(v >= 0 && v < n, "%s: index [%d][%d] = %d outside [0, %d)", fn, t, i, v, n);
        }
    }
    return MICV_OK;
}

int micv_calib_ls_trials_host(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices,
                              int stride, int k, int j, int T, const int32_t *kcount, const int *group_sizes, int G,
                              uint32_t flags, float *M, double *residual, int32_t *best_idx, double *best_res,
                              float *best_M) {
    HostCall h(ctx, "micv_calib_ls_trials_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(pts2d && pts3d && M && residual, "micv_calib_ls_trials_host: null argument");
    MICV_REQUIRE(n >= 1 && n <= 1 << 24 && k >= 0 && j >= 0 && j <= 64 && (int64_t)k + j <= n && T >= 1 &&
                     (indices ? stride >= k + j : (T == 1 && !kcount)) && G >= 0 && G <= 64 && (G == 0) == !group_sizes,
                 "micv_calib_ls_trials_host: bad n %d, k %d, j %d, T %d, stride %d or G %d", n, k, j, T, stride, G);
    if (group_sizes) {
        int64_t sum = 0;
        for (int i = 0; i < G; i++) sum += group_sizes[i] < 0 ? -((int64_t)1 << 40) : group_sizes[i];
        MICV_REQUIRE(sum == T && best_idx, "micv_calib_ls_trials_host: group sizes do not sum to T = %d", T);
    }
    MICV_REQUIRE((best_idx != nullptr) == (best_res != nullptr) && (best_idx != nullptr) == (best_M != nullptr) &&
                     !(flags & ~MICV_GEOM_F64),
                 "micv_calib_ls_trials_host: best_idx, best_res and best_M go together; flags %u", flags);
    MICV_TRY(geom_indices_ok("micv_calib_ls_trials_host", indices, stride, T, kcount, k, j, n));
    const size_t ni = indices ? (size_t)T * stride : 1, nr = (size_t)G + 1;
    float *d2 = h.up<float>(pts2d, (size_t)n * 8), *d3 = h.up<float>(pts3d, (size_t)n * 12);
    int32_t *di = h.up<int32_t>(indices, ni * 4), *dk = h.up<int32_t>(kcount, (size_t)T * 4);  // (no copy of a null list)
    float *dM = h.alloc<float>((size_t)T * 48);
    double *dr = h.alloc<double>((size_t)T * 8);
    int32_t *dbi = h.alloc<int32_t>(nr * 4);
    double *dbr = h.alloc<double>(nr * 8);
    float *dbm = h.alloc<float>(nr * 48);
    int32_t *dst = h.alloc<int32_t>(4);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_calib_ls_trials_dev(ctx, d2, d3, n, indices ? di : nullptr, stride, k, j, T, kcount ? dk : nullptr, group_sizes, G,
                                      flags, dM, dr, best_idx ? dbi : nullptr, best_idx ? dbr : nullptr, best_idx ? dbm : nullptr,
                                      dst, h.s));
    h.down(M, dM, (size_t)T * 48);
    h.down(residual, dr, (size_t)T * 8);
    if (best_idx) {
        h.down(best_idx, dbi, nr * 4);
        h.down(best_res, dbr, nr * 8);
        h.down(best_M, dbm, nr * 48);
    }
    return h.finish();
}

// The shape shared by the SVD and the fundamental solve: two point arrays, an index list, `per` floats out per system.
extern "C++" template <typename Fn>
static int geom_solve_host(HostCall &h, const char *fn, const float *pa, size_t abytes, const float *pb, size_t bbytes, int n,
                           const int32_t *indices, int stride, int k, int T, int per, float *out, Fn call) {
    MICV_TRY(geom_indices_ok(fn, indices, stride, T, nullptr, k, 0, n));
    const size_t ni = indices ? (size_t)T * stride : 1;
    float *da = h.up<float>(pa, abytes), *db = h.up<float>(pb, bbytes);
    int32_t *di = h.up<int32_t>(indices, ni * 4);  // (no copy of a null list)
    float *dout = h.alloc<float>((size_t)T * per * 4);
    int32_t *dst = h.alloc<int32_t>(4);
    if (!h.ok()) return h.finish();
    MICV_TRY(call(da, db, indices ? di : nullptr, dout, dst));
    h.down(out, dout, (size_t)T * per * 4);
    return h.finish();
}

int micv_calib_svd_host(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices, int stride,
                        int k, int T, uint32_t flags, float *M) {
    HostCall h(ctx, "micv_calib_svd_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(pts2d && pts3d && M, "micv_calib_svd_host: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && n >= 1 && n <= 1 << 24 && k >= 1 && k <= 1024 && k <= n && T >= 1 &&
                     (indices ? stride >= k : T == 1),
                 "micv_calib_svd_host: bad flags %u, n %d, k %d, T %d or stride %d", flags, n, k, T, stride);
    return geom_solve_host(h, "micv_calib_svd_host", pts2d, (size_t)n * 8, pts3d, (size_t)n * 12, n, indices, stride, k, T, 12, M,
                           [&](float *a, float *b, int32_t *i, float *o, int32_t *st) {
                               return micv_calib_svd_dev(ctx, a, b, n, i, stride, k, T, flags, o, st, h.s);
                           });
}

int micv_fundamental_ls_host(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, const int32_t *indices,
                             int stride, int k, int T, uint32_t flags, float *F) {
    HostCall h(ctx, "micv_fundamental_ls_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(ptsA && ptsB && F, "micv_fundamental_ls_host: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && n >= 1 && n <= 1 << 24 && k >= 0 && k <= n && T >= 1 &&
                     (indices ? stride >= k : T == 1),
                 "micv_fundamental_ls_host: bad flags %u, n %d, k %d, T %d or stride %d", flags, n, k, T, stride);
    return geom_solve_host(h, "micv_fundamental_ls_host", ptsA, (size_t)n * 8, ptsB, (size_t)n * 8, n, indices, stride, k, T, 9, F,
                           [&](float *a, float *b, int32_t *i, float *o, int32_t *st) {
                               return micv_fundamental_ls_dev(ctx, a, b, n, i, stride, k, T, flags, o, st, h.s);
                           });
}

int micv_fundamental_rank_reduce_host(micv_ctx *ctx, const float *F, int T, uint32_t flags, float *out) {
    HostCall h(ctx, "micv_fundamental_rank_reduce_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(F && out && T >= 1 && !(flags & ~MICV_GEOM_F64), "micv_fundamental_rank_reduce_host: bad argument");
    float *di = h.up<float>(F, (size_t)T * 36), *dout = h.alloc<float>((size_t)T * 36);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_fundamental_rank_reduce_dev(ctx, di, T, flags, dout, h.s));
    h.down(out, dout, (size_t)T * 36);
    return h.finish();
}

int micv_fundamental_normalized_host(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, uint32_t flags,
                                     float *Ta, float *Tb, float *Fhat, float *F) {
    HostCall h(ctx, "micv_fundamental_normalized_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(ptsA && ptsB && Ta && Tb && Fhat && F && n >= 1 && n <= 1 << 24 && !(flags & ~MICV_GEOM_F64),
                 "micv_fundamental_normalized_host: bad argument");
    float *da = h.up<float>(ptsA, (size_t)n * 8), *db = h.up<float>(ptsB, (size_t)n * 8), *o = h.alloc<float>(4 * 36);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_fundamental_normalized_dev(ctx, da, db, n, flags, o, o + 9, o + 18, o + 27, h.s));
    h.down(Ta, o, 36);
    h.down(Tb, o + 9, 36);
    h.down(Fhat, o + 18, 36);
    h.down(F, o + 27, 36);
    return h.finish();
}

int micv_epipolar_endpoints_host(micv_ctx *ctx, const float *F, const float *pts, int n, int side, int rows, int cols,
                                 uint32_t flags, float *out) {
    HostCall h(ctx, "micv_epipolar_endpoints_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(F && pts && out && n >= 1 && n <= 1 << 28 && (side == 0 || side == 1) && rows >= 1 && cols >= 1 &&
                     !(flags & ~MICV_GEOM_F64),
                 "micv_epipolar_endpoints_host: bad argument");
    float *dF = h.up<float>(F, 36), *dp = h.up<float>(pts, (size_t)n * 8), *dout = h.alloc<float>((size_t)n * 24);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_epipolar_endpoints_dev(ctx, dF, dp, n, side, rows, cols, flags, dout, h.s));
    h.down(out, dout, (size_t)n * 24);
    return h.finish();
}

int micv_camera_center_host(micv_ctx *ctx, const float *M, int T, uint32_t flags, float *center) {
    HostCall h(ctx, "micv_camera_center_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(M && center && T >= 1 && !(flags & ~MICV_GEOM_F64), "micv_camera_center_host: bad argument");
    float *dM = h.up<float>(M, (size_t)T * 48), *dout = h.alloc<float>((size_t)T * 12);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_camera_center_dev(ctx, dM, T, flags, dout, h.s));
    h.down(center, dout, (size_t)T * 12);
    return h.finish();
}

// ps4 registration (warp.hip).  Sizes and strides are checked here as far as the copies need them (an image
// of more than 32767 rows or columns is refused before anything is allocated); the `_dev` call checks the rest.
static bool warp_image_ok(int depth, int rows, int cols, size_t stride) {
    return (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F) && rows > 0 && cols > 0 && rows <= 32767 &&
           cols <= 32767 && stride_ok(stride, cols, depth == MICV_DEPTH_8U ? 1 : 4);
}

int micv_invert_affine_host(micv_ctx *ctx, const float *m, int count, float *inv) {
    HostCall h(ctx, "micv_invert_affine_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(m && inv && count >= 0, "micv_invert_affine_host: bad argument");
    if (count == 0) return MICV_OK;
    float *dm = h.up<float>(m, (size_t)count * 24), *di = h.alloc<float>((size_t)count * 24);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_invert_affine_dev(ctx, dm, count, di, h.s));
    h.down(inv, di, (size_t)count * 24);
    return h.finish();
}

int micv_warp_affine_host(micv_ctx *ctx, const void *src, int depth, int srows, int scols, size_t sstride, const float *m,
                          int flags, void *dst, int drows, int dcols, size_t dstride) {
    HostCall h(ctx, "micv_warp_affine_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && m && dst, "micv_warp_affine_host: null argument");
    MICV_REQUIRE(warp_image_ok(depth, srows, scols, sstride) && warp_image_ok(depth, drows, dcols, dstride),
                 "micv_warp_affine_host: bad depth %d, size %dx%d -> %dx%d (1..32767) or stride", depth, srows, scols, drows,
                 dcols);
    MICV_REQUIRE(src != dst, "micv_warp_affine_host: src and dst must not alias");
    const size_t e = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)scols * e, drb = (size_t)dcols * e;
    void *ds = h.up<void>(src, sstride, srb, srows), *dd = h.alloc<void>(drb * drows);
    float *dm = h.up<float>(m, 24);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_warp_affine_dev(ctx, ds, depth, srows, scols, srb, dm, flags, dd, drows, dcols, drb, h.s));
    h.down(dst, dstride, dd, drb, drows);
    return h.finish();
}

int micv_add_weighted_host(micv_ctx *ctx, const void *a, size_t astride, double alpha, const void *b, size_t bstride,
                           double beta, double gamma, int depth, int rows, int cols, void *dst, size_t dstride) {
    HostCall h(ctx, "micv_add_weighted_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(a && b && dst, "micv_add_weighted_host: null argument");
    MICV_REQUIRE(warp_image_ok(depth, rows, cols, astride) && warp_image_ok(depth, rows, cols, bstride) &&
                     warp_image_ok(depth, rows, cols, dstride),
                 "micv_add_weighted_host: bad depth %d, size %dx%d (1..32767) or stride", depth, rows, cols);
    const size_t rb = (size_t)cols * (depth == MICV_DEPTH_8U ? 1 : 4);
    void *da = h.up<void>(a, astride, rb, rows), *db = h.up<void>(b, bstride, rb, rows), *dd = h.alloc<void>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_add_weighted_dev(ctx, da, rb, alpha, db, rb, beta, gamma, depth, rows, cols, dd, rb, h.s));
    h.down(dst, dstride, dd, rb, rows);
    return h.finish();
}

int micv_register_blend_host(micv_ctx *ctx, const void *a, size_t astride, const void *b, size_t bstride, int depth, int rows,
                             int cols, const float *m_a_to_b, void *warped, size_t wstride, void *blended, size_t ostride) {
    HostCall h(ctx, "micv_register_blend_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(a && b && m_a_to_b && blended, "micv_register_blend_host: null argument");
    MICV_REQUIRE(warp_image_ok(depth, rows, cols, astride) && warp_image_ok(depth, rows, cols, bstride) &&
                     warp_image_ok(depth, rows, cols, ostride) && (!warped || warp_image_ok(depth, rows, cols, wstride)),
                 "micv_register_blend_host: bad depth %d, size %dx%d (1..32767) or stride", depth, rows, cols);
    const size_t rb = (size_t)cols * (depth == MICV_DEPTH_8U ? 1 : 4), n = rb * rows;
    void *da = h.up<void>(a, astride, rb, rows), *db = h.up<void>(b, bstride, rb, rows);
    void *dw = warped ? h.alloc<void>(n) : nullptr, *dd = h.alloc<void>(n);
    float *dm = h.up<float>(m_a_to_b, 24);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_register_blend_dev(ctx, da, rb, db, rb, depth, rows, cols, dm, dw, rb, dd, rb, h.s));
    if (warped) h.down(warped, wstride, dw, rb, rows);
    h.down(blended, ostride, dd, rb, rows);
    return h.finish();
}

// display (display.hip).  Device images are packed (row = cols elements) at 256-byte-aligned pitches.
static bool display_src_ok(int depth, int rows, int cols, size_t stride) {
    return (depth == MICV_DEPTH_32F || depth == MICV_DEPTH_8U || depth == MICV_DEPTH_8S) && rows > 0 && cols > 0 &&
           (int64_t)rows * cols < ((int64_t)1 << 31) && stride_ok(stride, cols, depth == MICV_DEPTH_32F ? 4 : 1);
}
static size_t pitch256(size_t bytes) { return (bytes + 255) & ~size_t(255); }

int micv_normalize_minmax_batch_host(micv_ctx *ctx, const void *src, size_t src_pitch, int depth, int batch, int rows, int cols,
                                     size_t sstride, uint8_t *dst_u8, size_t u8_pitch, size_t u8_stride,
                                     uint8_t *dst_inverted, size_t inverted_pitch, size_t inverted_stride, uint8_t *dst_jet,
                                     size_t jet_pitch, size_t jet_stride, float *minmax_out) {
    HostCall h(ctx, "micv_normalize_minmax_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && (dst_u8 || dst_inverted || dst_jet), "micv_normalize_minmax_host: no source or no output wanted");
    MICV_REQUIRE(batch >= 0 && display_src_ok(depth, rows, cols, sstride),
                 "micv_normalize_minmax_host: bad batch %d, depth %d, size %dx%d (rows * cols < 2^31) or stride", batch, depth, rows, cols);
    MICV_REQUIRE((!dst_u8 || u8_stride >= (size_t)cols) && (!dst_inverted || inverted_stride >= (size_t)cols) &&
                     (!dst_jet || jet_stride >= 3 * (size_t)cols),
                 "micv_normalize_minmax_host: an output's stride is smaller than its rows");
    const size_t last = (size_t)(rows - 1);
    MICV_REQUIRE(batch <= 1 || (src_pitch >= last * sstride + (size_t)cols * (depth == MICV_DEPTH_32F ? 4 : 1) &&
                                (!dst_u8 || u8_pitch >= last * u8_stride + (size_t)cols) &&
                                (!dst_inverted || inverted_pitch >= last * inverted_stride + (size_t)cols) &&
                                (!dst_jet || jet_pitch >= last * jet_stride + 3 * (size_t)cols)),
                 "micv_normalize_minmax_host: a pitch is smaller than an image");
    if (batch == 0) return MICV_OK;
    const size_t e = depth == MICV_DEPTH_32F ? 4 : 1, srb = (size_t)cols * e, sp = pitch256(srb * rows);
    const size_t gp = pitch256((size_t)cols * rows), jp = pitch256(3 * (size_t)cols * rows), nb = (size_t)batch;
    char *ds = h.alloc<char>(sp * nb);
    uint8_t *du = dst_u8 ? h.alloc<uint8_t>(gp * nb) : nullptr, *di = dst_inverted ? h.alloc<uint8_t>(gp * nb) : nullptr;
    uint8_t *dj = dst_jet ? h.alloc<uint8_t>(jp * nb) : nullptr;
    float *dm = h.alloc<float>(8 * nb);
    for (size_t i = 0; i < nb; i++) h.up_to(ds + i * sp, static_cast<const char *>(src) + i * src_pitch, sstride, srb, rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_normalize_minmax_batch_dev(ctx, ds, sp, depth, batch, rows, cols, srb, du, gp, (size_t)cols, di, gp, (size_t)cols, dj, jp,
                                             3 * (size_t)cols, dm, h.s));
    for (size_t i = 0; i < nb; i++) {
        if (dst_u8) h.down(dst_u8 + i * u8_pitch, u8_stride, du + i * gp, (size_t)cols, rows);
        if (dst_inverted) h.down(dst_inverted + i * inverted_pitch, inverted_stride, di + i * gp, (size_t)cols, rows);
        if (dst_jet) h.down(dst_jet + i * jet_pitch, jet_stride, dj + i * jp, 3 * (size_t)cols, rows);
    }
    if (minmax_out) h.down(minmax_out, dm, 8 * nb);
    return h.finish();
}

int micv_normalize_minmax_host(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride,
                               uint8_t *dst_u8, size_t u8_stride, uint8_t *dst_inverted, size_t inverted_stride,
                               uint8_t *dst_jet, size_t jet_stride, float *minmax_out) {
    return micv_normalize_minmax_batch_host(ctx, src, 0, depth, 1, rows, cols, sstride, dst_u8, 0, u8_stride, dst_inverted, 0,
                                            inverted_stride, dst_jet, 0, jet_stride, minmax_out);
}

int micv_apply_colormap_jet_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, uint8_t *dst_jet,
                                 size_t jet_stride) {
    HostCall h(ctx, "micv_apply_colormap_jet_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst_jet && display_src_ok(MICV_DEPTH_8U, rows, cols, sstride) && jet_stride >= 3 * (size_t)cols,
                 "micv_apply_colormap_jet_host: bad argument, size %dx%d (rows * cols < 2^31) or stride", rows, cols);
    const size_t n = (size_t)rows * cols;
    uint8_t *ds = h.up<uint8_t>(src, sstride, (size_t)cols, rows), *dj = h.alloc<uint8_t>(3 * n);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_apply_colormap_jet_dev(ctx, ds, rows, cols, (size_t)cols, dj, 3 * (size_t)cols, h.s));
    h.down(dst_jet, jet_stride, dj, 3 * (size_t)cols, rows);
    return h.finish();
}

int micv_gain_noise_f32_host(micv_ctx *ctx, const float *src, size_t sstride, float gain, const float *noise, size_t nstride,
                             int rows, int cols, float *dst, size_t dstride) {
    HostCall h(ctx, "micv_gain_noise_f32_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0 && stride_ok(sstride, cols, 4) && stride_ok(dstride, cols, 4) &&
                     (!noise || stride_ok(nstride, cols, 4)),
                 "micv_gain_noise_f32_host: bad argument, size %dx%d or stride", rows, cols);
    const size_t rb = (size_t)cols * 4;
    float *ds = h.up<float>(src, sstride, rb, rows), *dn = noise ? h.up<float>(noise, nstride, rb, rows) : nullptr;
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_gain_noise_f32_dev(ctx, ds, rb, gain, dn, rb, rows, cols, ds, rb, h.s));
    h.down(dst, dstride, ds, rb, rows);
    return h.finish();
}

// One body for the pair with and without its display images (img_left == nullptr: the maps alone).
static int pair_host(const char *fn, micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                     float gain, const float *noise_left, const float *noise_right, size_t nstride, int rad, int range,
                     int metric, int flags, int8_t *disp_left, int8_t *disp_right, size_t dstride, bool display,
                     uint8_t *img_left, uint8_t *img_left_inv, uint8_t *img_right, size_t istride) {
    HostCall h(ctx, "micv_disparity_pair_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(left && right && disp_left && disp_right && (!display || (img_left && img_right)), "%s: null argument", fn);
    MICV_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols < ((int64_t)1 << 31) && stride_ok(stride, cols, 4) &&
                     dstride >= (size_t)cols && (!display || istride >= (size_t)cols),
                 "%s: bad size %dx%d (rows * cols < 2^31) or stride", fn, rows, cols);
    MICV_REQUIRE(!noise_left == !noise_right && (!noise_left || stride_ok(nstride, cols, 4)),
                 "%s: one noise image without the other, or a bad noise stride", fn);
    const size_t rb = (size_t)cols * 4, n = rb * rows, g = pitch256((size_t)cols * rows);
    const bool change = noise_left || gain != 1.f;
    float *dl = h.up<float>(left, stride, rb, rows), *dr = h.up<float>(right, stride, rb, rows);
    float *dnl = noise_left ? h.up<float>(noise_left, nstride, rb, rows) : nullptr;
    float *dnr = noise_left ? h.up<float>(noise_right, nstride, rb, rows) : nullptr;
    float *dw = change ? h.alloc<float>(2 * n) : nullptr;
    int8_t *d0 = h.alloc<int8_t>(2 * g), *d1 = d0 + g;
    uint8_t *i0 = h.alloc<uint8_t>(display ? 3 * g : 16), *i1 = i0 + g, *i2 = i1 + g;
    if (!h.ok()) return h.finish();
    if (display)
        MICV_TRY(micv_disparity_pair_display_dev(ctx, dl, dr, rows, cols, rb, gain, dnl, dnr, rb, rad, range, metric, flags, d0, d1,
                                                 (size_t)cols, i0, img_left_inv ? i1 : nullptr, i2, (size_t)cols, dw, h.s));
    else
        MICV_TRY(micv_disparity_pair_dev(ctx, dl, dr, rows, cols, rb, rad, range, metric, flags, d0, d1, (size_t)cols, h.s));
    h.down(disp_left, dstride, d0, (size_t)cols, rows);
    h.down(disp_right, dstride, d1, (size_t)cols, rows);
    if (display) {
        h.down(img_left, istride, i0, (size_t)cols, rows);
        if (img_left_inv) h.down(img_left_inv, istride, i1, (size_t)cols, rows);
        h.down(img_right, istride, i2, (size_t)cols, rows);
    }
    return h.finish();
}

int micv_disparity_pair_host(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                             int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                             int8_t *disp_right, size_t dstride) {
    return pair_host("micv_disparity_pair_host", ctx, left, right, rows, cols, stride, 1.f, nullptr, nullptr, 0, window_rad,
                     disparity_range, metric, flags, disp_left, disp_right, dstride, false, nullptr, nullptr, nullptr, 0);
}

int micv_disparity_pair_display_host(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                                     float gain, const float *noise_left, const float *noise_right, size_t nstride,
                                     int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                                     int8_t *disp_right, size_t dstride, uint8_t *image_left, uint8_t *image_left_inverted,
                                     uint8_t *image_right, size_t istride) {
    return pair_host("micv_disparity_pair_display_host", ctx, left, right, rows, cols, stride, gain, noise_left, noise_right, nstride,
                     window_rad, disparity_range, metric, flags, disp_left, disp_right, dstride, true, image_left,
                     image_left_inverted, image_right, istride);
}

// ---- ps1 driver (hough.hip's radius-range search, ps1.hip) ------------------------------------

int micv_hough_circles_range_peaks_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                                        unsigned min_radius, unsigned max_radius, unsigned num_peaks, int threshold,
                                        uint32_t *peaks_rc, int64_t *counts, int32_t *acc) {
    HostCall h(ctx, "micv_hough_circles_range_peaks_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(mask && rows > 0 && cols > 0 && rows <= 32767 && cols <= 32767 && mstride >= (size_t)cols && num_peaks <= 4096,
                 "micv_hough_circles_range_peaks_host: bad argument");
    if (min_radius > max_radius) return MICV_OK;
    MICV_REQUIRE(counts && (peaks_rc || num_peaks == 0), "micv_hough_circles_range_peaks_host: null output");
    const size_t n_radii = (size_t)max_radius - min_radius + 1, cells = (size_t)rows * cols;
    const size_t pbytes = n_radii * num_peaks * 8, abytes = acc ? n_radii * cells * 4 : 0;
    uint8_t *dm = h.up<uint8_t>(mask, mstride, (size_t)cols, rows);
    uint32_t *dp = h.alloc<uint32_t>(pbytes + 8);
    int64_t *dn = h.alloc<int64_t>(n_radii * 8);
    int32_t *da = h.alloc<int32_t>(abytes + 8);
    if (!h.ok()) return h.finish();
    if (pbytes) h.check(hipMemsetAsync(dp, 0, pbytes, h.s), "hipMemsetAsync");  // rows past a count are unspecified; the host copy gets zeros
    if (!h.ok()) return h.finish();
    MICV_TIMED(h, "houghCirclesAccumulateKernel",
               micv_hough_circles_range_peaks_dev(ctx, dm, rows, cols, cols, min_radius, max_radius, num_peaks, threshold, dp, dn,
                                                  acc ? da : nullptr, h.s));
    h.down(counts, dn, n_radii * 8);
    if (pbytes) h.down(peaks_rc, dp, pbytes);
    if (abytes) h.down(acc, da, abytes);
    return h.finish();
}

// one image in, one image out: upload, `call` on the device blocks (dense pitches), download
extern "C++" template <typename Fn>
static int image_host(micv_ctx *ctx, const char *fn, const void *src, size_t sstride, size_t src_row_bytes, void *dst, size_t dstride,
                      size_t dst_row_bytes, int rows, int cols, Fn call) {
    HostCall h(ctx, fn);
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0 && sstride >= src_row_bytes && dstride >= dst_row_bytes, "%s: bad argument", fn);
    void *ds = h.up<void>(src, sstride, src_row_bytes, rows), *dd = h.alloc<void>((size_t)rows * dst_row_bytes);
    if (!h.ok()) return h.finish();
    MICV_TRY(call(ds, dd, h.s));
    h.down(dst, dstride, dd, dst_row_bytes, rows);
    return h.finish();
}

int micv_gaussian_blur_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int gauss_size,
                               double gauss_sigma, uint8_t *dst, size_t dstride) {
    return image_host(ctx, "micv_gaussian_blur_u8_host", src, sstride, (size_t)cols, dst, dstride, (size_t)cols, rows, cols,
                      [&](void *ds, void *dd, hipStream_t s) {
                          return micv_gaussian_blur_u8_dev(ctx, static_cast<uint8_t *>(ds), rows, cols, cols, gauss_size, gauss_sigma,
                                                           static_cast<uint8_t *>(dd), cols, s);
                      });
}

int micv_gaussian_blur_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int gauss_size,
                                double gauss_sigma, float *dst, size_t dstride) {
    return image_host(ctx, "micv_gaussian_blur_f32_host", src, sstride, (size_t)cols * 4, dst, dstride, (size_t)cols * 4, rows, cols,
                      [&](void *ds, void *dd, hipStream_t s) {
                          return micv_gaussian_blur_f32_dev(ctx, static_cast<float *>(ds), rows, cols, (size_t)cols * 4, gauss_size,
                                                            gauss_sigma, static_cast<float *>(dd), (size_t)cols * 4, s);
                      });
}

int micv_generate_edge_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t stride, int gauss_size,
                                double gauss_sigma, double low_thresh, double high_thresh, uint8_t *edges,
                                size_t estride) {
    return image_host(ctx, "micv_generate_edge_f32_host", src, stride, (size_t)cols * 4, edges, estride, (size_t)cols, rows, cols,
                      [&](void *ds, void *dd, hipStream_t s) {
                          return micv_generate_edge_f32_dev(ctx, static_cast<float *>(ds), rows, cols, (size_t)cols * 4, gauss_size,
                                                            gauss_sigma, low_thresh, high_thresh, static_cast<uint8_t *>(dd), cols, s);
                      });
}

int micv_hysteresis_u8_host(micv_ctx *ctx, const uint8_t *cand, size_t cstride, const uint8_t *strong, size_t sstride, int rows, int cols,
                            uint8_t *edges, size_t estride) {
    HostCall h(ctx, "micv_hysteresis_u8_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(cand && strong && edges && rows > 0 && cols > 0 && cstride >= (size_t)cols && sstride >= (size_t)cols && estride >= (size_t)cols,
                 "micv_hysteresis_u8_host: bad argument");
    uint8_t *dc = h.up<uint8_t>(cand, cstride, (size_t)cols, rows), *dst = h.up<uint8_t>(strong, sstride, (size_t)cols, rows);
    uint8_t *de = h.alloc<uint8_t>((size_t)rows * cols);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_hysteresis_u8_async(ctx, dc, cols, dst, cols, rows, cols, de, cols, h.s));
    h.down(edges, estride, de, (size_t)cols, rows);
    return h.finish();
}

// The images of a batch arrive as they lie in host memory (ROIs with pitches of their own) and are packed into ONE
// device block on the way up; one batch call; the edges come down from one block, each to its own rows.
int micv_generate_edge_batch_host(micv_ctx *ctx, const uint8_t *const *srcs, const size_t *strides, int batch, int rows, int cols,
                                  int gauss_size, double gauss_sigma, double low_thresh, double high_thresh, uint8_t *const *edges,
                                  const size_t *estrides) {
    HostCall h(ctx, "micv_generate_edge_batch_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(srcs && strides && edges && estrides && batch >= 1 && rows > 0 && cols > 0, "micv_generate_edge_batch_host: bad argument");
    for (int i = 0; i < batch; i++)
        MICV_REQUIRE(srcs[i] && edges[i] && strides[i] >= (size_t)cols && estrides[i] >= (size_t)cols,
                     "micv_generate_edge_batch_host: image %d: null pointer or a pitch below the width", i);
    const size_t n = (size_t)rows * cols;
    uint8_t *ds = h.alloc<uint8_t>(n * batch), *de = h.alloc<uint8_t>(n * batch);
    for (int i = 0; i < batch; i++) h.up_to(ds + i * n, srcs[i], strides[i], (size_t)cols, rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_generate_edge_batch_async(ctx, ds, batch, n, rows, cols, cols, gauss_size, gauss_sigma, low_thresh, high_thresh, de, n, cols,
                                            0, h.s));
    for (int i = 0; i < batch; i++) h.down(edges[i], estrides[i], de + i * n, (size_t)cols, rows);
    return h.finish();
}

int micv_erode_ellipse_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int ksize, float *dst,
                                size_t dstride) {
    return image_host(ctx, "micv_erode_ellipse_f32_host", src, sstride, (size_t)cols * 4, dst, dstride, (size_t)cols * 4, rows, cols,
                      [&](void *ds, void *dd, hipStream_t s) {
                          return micv_erode_ellipse_f32_dev(ctx, static_cast<float *>(ds), rows, cols, (size_t)cols * 4, ksize,
                                                            static_cast<float *>(dd), (size_t)cols * 4, s);
                      });
}

int micv_erode_ellipse_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int ksize,
                               uint8_t *dst, size_t dstride) {
    return image_host(ctx, "micv_erode_ellipse_u8_host", src, sstride, (size_t)cols, dst, dstride, (size_t)cols, rows, cols,
                      [&](void *ds, void *dd, hipStream_t s) {
                          return micv_erode_ellipse_u8_dev(ctx, static_cast<uint8_t *>(ds), rows, cols, cols, ksize,
                                                           static_cast<uint8_t *>(dd), cols, s);
                      });
}

int micv_gray_to_rgb8_host(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride, uint8_t *dst,
                           size_t dstride) {
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_gray_to_rgb8_host: depth %d not supported (8U, 32F)", depth);
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4;
    return image_host(ctx, "micv_gray_to_rgb8_host", src, sstride, (size_t)cols * es, dst, dstride, (size_t)cols * 3, rows, cols,
                      [&](void *ds, void *dd, hipStream_t s) {
                          return micv_gray_to_rgb8_dev(ctx, ds, depth, rows, cols, (size_t)cols * es, static_cast<uint8_t *>(dd),
                                                       (size_t)cols * 3, s);
                      });
}

int micv_parallel_lines_host(micv_ctx *ctx, const uint32_t *peaks_rc, int64_t count, unsigned delta_rho,
                             unsigned delta_theta, uint32_t *out_rc, int64_t *out_count) {
    HostCall h(ctx, "micv_parallel_lines_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(out_count && count >= 0 && count <= 4096 && ((peaks_rc && out_rc) || count == 0),
                 "micv_parallel_lines_host: bad argument (<= 4096 peaks)");
    MICV_REQUIRE(delta_rho > 0 && delta_theta > 0, "micv_parallel_lines_host: delta_rho and delta_theta must be positive");
    uint32_t *dp = h.alloc<uint32_t>((size_t)count * 8 + 8), *dout = h.alloc<uint32_t>((size_t)count * 8 + 8);
    int64_t *dn = h.alloc<int64_t>(16);
    if (count) h.up_to(dp, peaks_rc, (size_t)count * 8, (size_t)count * 8, 1);
    h.up_to(dn, &count, 8, 8, 1);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_parallel_lines_dev(ctx, dp, dn, (unsigned)count, delta_rho, delta_theta, dout, dn + 1, h.s));
    h.down(out_count, dn + 1, 8);
    MICV_TRY(h.finish());  // the count is here now
    if (*out_count > 0) h.down(out_rc, dout, (size_t)*out_count * 8);
    return h.finish();
}

int micv_draw_lines_parametric_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride,
                                    const uint32_t *peaks_rc, int64_t count, unsigned rho_bin, unsigned theta_bin,
                                    const uint8_t *color) {
    HostCall h(ctx, "micv_draw_lines_parametric_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && color && rows > 0 && cols > 0 && stride >= (size_t)cols * 3 && count >= 0 && count <= 4096 &&
                     (peaks_rc || count == 0),
                 "micv_draw_lines_parametric_host: bad argument (<= 4096 peaks)");
    const size_t rb = (size_t)cols * 3;
    uint8_t *di = h.up<uint8_t>(img, stride, rb, rows);
    uint32_t *dp = h.alloc<uint32_t>((size_t)count * 8 + 8);
    if (count) h.up_to(dp, peaks_rc, (size_t)count * 8, (size_t)count * 8, 1);
    int64_t *dn = h.up<int64_t>(&count, 8);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_lines_parametric_dev(ctx, di, rows, cols, rb, dp, dn, (unsigned)count, rho_bin, theta_bin, color, h.s));
    h.down(img, stride, di, rb, rows);
    return h.finish();
}

int micv_draw_circles_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride, const uint32_t *peaks_rc,
                           const int64_t *counts, unsigned n_radii, unsigned num_peaks, unsigned min_radius,
                           const uint8_t *color) {
    HostCall h(ctx, "micv_draw_circles_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && color && rows > 0 && cols > 0 && stride >= (size_t)cols * 3 && num_peaks <= 4096 &&
                     (unsigned long long)n_radii * num_peaks < (1ull << 31),
                 "micv_draw_circles_host: bad argument");
    const size_t total = (size_t)n_radii * num_peaks;
    if (total == 0) return MICV_OK;
    MICV_REQUIRE(peaks_rc && counts, "micv_draw_circles_host: null argument");
    const size_t rb = (size_t)cols * 3;
    uint8_t *di = h.up<uint8_t>(img, stride, rb, rows);
    uint32_t *dp = h.up<uint32_t>(peaks_rc, total * 8);
    int64_t *dn = h.up<int64_t>(counts, (size_t)n_radii * 8);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_circles_dev(ctx, di, rows, cols, rb, dp, dn, n_radii, num_peaks, min_radius, color, h.s));
    h.down(img, stride, di, rb, rows);
    return h.finish();
}

// ---- ps5 driver (ps5.hip) ----------------------------------------------------------------------

int micv_draw_velocity_vectors_host(micv_ctx *ctx, uint8_t *img, size_t img_pitch, size_t stride, const float *u, const float *v,
                                    size_t field_pitch, size_t fstride, int batch, int rows, int cols, const uint8_t *color) {
    HostCall h(ctx, "micv_draw_velocity_vectors_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && u && v && color && rows > 0 && cols > 0 && batch >= 0 && stride >= (size_t)cols * 3 && stride_ok(fstride, cols, 4),
                 "micv_draw_velocity_vectors_host: bad argument, size %dx%d or stride", rows, cols);
    MICV_REQUIRE(batch <= 1 || (img_pitch >= (size_t)(rows - 1) * stride + (size_t)cols * 3 &&
                                field_pitch >= (size_t)(rows - 1) * fstride + (size_t)cols * 4),
                 "micv_draw_velocity_vectors_host: a pitch is smaller than an image or a field");
    if (batch == 0) return MICV_OK;
    const size_t irb = (size_t)cols * 3, frb = (size_t)cols * 4, ip = pitch256(irb * rows), fp = pitch256(frb * rows), nb = (size_t)batch;
    char *di = h.alloc<char>(ip * nb), *du = h.alloc<char>(fp * nb), *dv = h.alloc<char>(fp * nb);
    for (size_t i = 0; i < nb; i++) {
        h.up_to(di + i * ip, img + i * img_pitch, stride, irb, rows);
        h.up_to(du + i * fp, reinterpret_cast<const char *>(u) + i * field_pitch, fstride, frb, rows);
        h.up_to(dv + i * fp, reinterpret_cast<const char *>(v) + i * field_pitch, fstride, frb, rows);
    }
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_velocity_vectors_dev(ctx, reinterpret_cast<uint8_t *>(di), ip, irb, reinterpret_cast<float *>(du),
                                            reinterpret_cast<float *>(dv), fp, frb, batch, rows, cols, color, h.s));
    for (size_t i = 0; i < nb; i++) h.down(img + i * img_pitch, stride, di + i * ip, irb, rows);
    return h.finish();
}

int micv_gray_or_bgr_to_bgr8_host(micv_ctx *ctx, const void *src, int depth, int channels, int rows, int cols, size_t sstride,
                                  uint8_t *dst, size_t dstride) {
    MICV_REQUIRE(depth == MICV_DEPTH_8U && (channels == 1 || channels == 3),
                 "micv_gray_or_bgr_to_bgr8_host: depth %d / %d channels not supported (8U, 1 or 3 channels)", depth, channels);
    return image_host(ctx, "micv_gray_or_bgr_to_bgr8_host", src, sstride, (size_t)cols * channels, dst, dstride, (size_t)cols * 3, rows,
                      cols, [&](void *ds, void *dd, hipStream_t s) {
                          return micv_gray_or_bgr_to_bgr8_dev(ctx, ds, depth, channels, rows, cols, (size_t)cols * channels,
                                                              static_cast<uint8_t *>(dd), (size_t)cols * 3, s);
                      });
}

int micv_pyramid_montage_host(micv_ctx *ctx, const void *const *levels, const int *level_rows, const int *level_cols,
                              const size_t *level_strides, int depth, uint8_t *dst, size_t dstride) {
    HostCall h(ctx, "micv_pyramid_montage_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(levels && level_rows && level_cols && level_strides && dst, "micv_pyramid_montage_host: null argument");
    MICV_REQUIRE(depth == MICV_DEPTH_32F || depth == MICV_DEPTH_8U, "micv_pyramid_montage_host: depth %d not supported (32F, 8U)", depth);
    const size_t e = depth == MICV_DEPTH_32F ? 4 : 1;
    size_t off[5] = {0, 0, 0, 0, 0}, rb[4];
    for (int l = 0; l < 4; l++) {
        MICV_REQUIRE(levels[l] && level_rows[l] > 0 && level_cols[l] > 0 && level_rows[l] <= 16383 && level_cols[l] <= 16383 &&
                         stride_ok(level_strides[l], level_cols[l], e),
                     "micv_pyramid_montage_host: level %d: null, bad size or stride", l);
        rb[l] = (size_t)level_cols[l] * e;
        off[l + 1] = off[l] + pitch256(rb[l] * level_rows[l]);
    }
    const int R = level_rows[0], C = level_cols[0];
    MICV_REQUIRE(dstride >= (size_t)2 * C, "micv_pyramid_montage_host: stride %zu does not hold %d columns", dstride, 2 * C);
    char *dl = h.alloc<char>(off[4]);
    uint8_t *dd = h.alloc<uint8_t>((size_t)4 * R * C);
    const void *dev_levels[4];
    for (int l = 0; l < 4; l++) {
        h.up_to(dl + off[l], levels[l], level_strides[l], rb[l], level_rows[l]);
        dev_levels[l] = dl + off[l];
    }
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_pyramid_montage_dev(ctx, dev_levels, level_rows, level_cols, rb, depth, dd, (size_t)2 * C, h.s));
    h.down(dst, dstride, dd, (size_t)2 * C, 2 * R);
    return h.finish();
}

int micv_lk_warp_diff_host(micv_ctx *ctx, const float *prev, size_t pstride, const float *next, size_t nstride, const float *du,
                           const float *dv, size_t fstride, int rows, int cols, float *diff, size_t dstride) {
    HostCall h(ctx, "micv_lk_warp_diff_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(prev && next && du && dv && diff && rows > 0 && cols > 0, "micv_lk_warp_diff_host: bad argument");
    MICV_REQUIRE(stride_ok(pstride, cols, 4) && stride_ok(nstride, cols, 4) && stride_ok(fstride, cols, 4) && stride_ok(dstride, cols, 4),
                 "micv_lk_warp_diff_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    float *dp = h.up<float>(prev, pstride, rb, rows), *dn = h.up<float>(next, nstride, rb, rows);
    float *dU = h.up<float>(du, fstride, rb, rows), *dV = h.up<float>(dv, fstride, rb, rows), *dd = h.alloc<float>(rb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_lk_warp_diff_dev(ctx, dp, rb, dn, rb, dU, dV, rb, rows, cols, dd, rb, h.s));
    h.down(diff, dstride, dd, rb, rows);
    return h.finish();
}

int micv_ps5_warp_diff_seq_host(micv_ctx *ctx, const void *const *frames, int nframes, int rows, int cols, size_t stride,
                                int channels, int depth, int levels, int level, int win, uint8_t *diff_u8, float *diff_f32,
                                float *u, float *v) {
    HostCall h(ctx, "micv_ps5_warp_diff_seq_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(frames && diff_u8 && rows > 0 && cols > 0, "micv_ps5_warp_diff_seq_host: bad argument");
    MICV_REQUIRE(nframes >= 2 && nframes <= 1025, "micv_ps5_warp_diff_seq_host: %d frames (2..1025: at least one pair)", nframes);
    MICV_REQUIRE((channels == 1 || channels == 3 || channels == 4) && (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F),
                 "micv_ps5_warp_diff_seq_host: frames must be 1/3/4-channel 8U or 32F");
    MICV_REQUIRE(levels >= 1 && levels <= 16 && level >= 0 && level < levels && (rows >> level) > 0 && (cols >> level) > 0,
                 "micv_ps5_warp_diff_seq_host: level %d of %d does not fit a %dx%d image", level, levels, rows, cols);
    MICV_REQUIRE((u == nullptr) == (v == nullptr), "micv_ps5_warp_diff_seq_host: give both flow outputs or none");
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)cols * channels * es;
    MICV_REQUIRE(stride >= srb, "micv_ps5_warp_diff_seq_host: bad stride");
    for (int t = 0; t < nframes; t++) MICV_REQUIRE(frames[t] != nullptr, "micv_ps5_warp_diff_seq_host: frame %d is null", t);
    const size_t nf = (size_t)nframes, np = nf - 1, rb = (size_t)cols * 4, n0 = (size_t)rows * cols;
    // the pyramid block holds levels 1.. only (level 0 is `grey` itself), and nothing when the chain takes level 0
    size_t lvl_off[17] = {0};
    if (level > 0)
        for (int l = 1; l < levels; l++) lvl_off[l + 1] = lvl_off[l] + pitch256((size_t)(rows >> l) * (cols >> l) * 4 * nf);
    const int lr = rows >> level, lc = cols >> level;
    const size_t ln = (size_t)lr * lc;
    void *raw = h.alloc<void>(srb * rows);
    float *grey = h.alloc<float>(n0 * 4 * nf);
    char *pyr = h.alloc<char>(lvl_off[levels] ? lvl_off[levels] : 16);
    uint8_t *d8 = h.alloc<uint8_t>(ln * np);
    float *df = diff_f32 ? h.alloc<float>(ln * 4 * np) : nullptr;
    float *dU = u ? h.alloc<float>(ln * 4 * np) : nullptr, *dV = u ? h.alloc<float>(ln * 4 * np) : nullptr;
    if (!h.ok()) return h.finish();
    for (size_t t = 0; t < nf; t++) {  // (one raw block: the copy of frame t + 1 queues behind the conversion of frame t)
        h.up_to(raw, frames[t], stride, srb, rows);
        if (!h.ok()) return h.finish();
        MICV_TRY(micv_to_gray_f32_dev(ctx, raw, rows, cols, srb, channels, depth, grey + t * n0, rb, h.s));
    }
    const float *lvl_frames = grey;
    if (level > 0) {
        float *dst_levels[16];
        for (int l = 0; l < levels; l++) dst_levels[l] = l == 0 ? nullptr : reinterpret_cast<float *>(pyr + lvl_off[l]);
        MICV_TRY(micv_gaussian_pyramid_batch_dev(ctx, grey, nframes, n0 * 4, rows, cols, rb, levels, dst_levels, nullptr, nullptr, h.s));
        lvl_frames = dst_levels[level];
    }
    MICV_TRY(micv_ps5_warp_diff_seq_dev(ctx, lvl_frames, ln * 4, nframes, lr, lc, (size_t)lc * 4, win, d8, ln, (size_t)lc, df, dU, dV, h.s));
    h.down(diff_u8, d8, ln * np);
    if (diff_f32) h.down(diff_f32, df, ln * 4 * np);
    if (u) {
        h.down(u, dU, ln * 4 * np);
        h.down(v, dV, ln * 4 * np);
    }
    return h.finish();
}

int micv_dense_lk_display_host(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols, size_t stride, int channels,
                               int depth, int mode, int win, int levels, const uint8_t *color, float *u, float *v, size_t ostride,
                               uint8_t *arrows, size_t astride, uint8_t *jet_u, uint8_t *jet_v, size_t jstride) {
    HostCall h(ctx, "micv_dense_lk_display_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(prev && next && color && u && v && arrows && rows > 0 && cols > 0, "micv_dense_lk_display_host: bad argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U && (channels == 1 || channels == 3),
                 "micv_dense_lk_display_host: depth %d / %d channels not supported (8-bit frames of 1 or 3 channels)", depth, channels);
    MICV_REQUIRE((jet_u == nullptr) == (jet_v == nullptr), "micv_dense_lk_display_host: give both colour maps or none");
    const size_t srb = (size_t)cols * channels, rb = (size_t)cols * 4, n = rb * rows, irb = (size_t)cols * 3, in = pitch256(irb * rows);
    MICV_REQUIRE(stride >= srb && stride_ok(ostride, cols, 4) && astride >= irb && (!jet_u || jstride >= irb),
                 "micv_dense_lk_display_host: bad stride");
    const size_t fn = pitch256(n);
    void *dp = h.up<void>(prev, stride, srb, rows), *dn = h.up<void>(next, stride, srb, rows);
    char *duv = h.alloc<char>(2 * fn);
    uint8_t *da = h.alloc<uint8_t>(in), *ju = jet_u ? h.alloc<uint8_t>(2 * in) : nullptr, *jv = jet_u ? ju + in : nullptr;
    if (!h.ok()) return h.finish();
    float *du = reinterpret_cast<float *>(duv), *dv = reinterpret_cast<float *>(duv + fn);
    MICV_TRY(micv_dense_lk_display_dev(ctx, dp, dn, rows, cols, srb, channels, depth, mode, win, levels, color, du, dv, rb, da, irb, ju, jv,
                                       irb, h.s));
    h.down(u, ostride, du, rb, rows);
    h.down(v, ostride, dv, rb, rows);
    h.down(arrows, astride, da, irb, rows);
    if (jet_u) {
        h.down(jet_u, jstride, ju, irb, rows);
        h.down(jet_v, jstride, jv, irb, rows);
    }
    return h.finish();
}

int micv_dense_lk_display_seq_host(micv_ctx *ctx, const void *const *frames, int nframes, int rows, int cols, size_t stride, int channels,
                                   int depth, int win, int levels, const uint8_t *color, float *const *u, float *const *v, size_t ostride,
                                   uint8_t *const *arrows, size_t astride, uint8_t *const *jet_u, uint8_t *const *jet_v, size_t jstride) {
    HostCall h(ctx, "micv_dense_lk_display_seq_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(frames && color && u && v && arrows && nframes >= 2 && nframes <= 32768 && rows > 0 && cols > 0,
                 "micv_dense_lk_display_seq_host: bad argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U && (channels == 1 || channels == 3),
                 "micv_dense_lk_display_seq_host: depth %d / %d channels not supported (8-bit frames of 1 or 3 channels)", depth, channels);
    MICV_REQUIRE((jet_u == nullptr) == (jet_v == nullptr), "micv_dense_lk_display_seq_host: give both colour maps or none");
    const size_t srb = (size_t)cols * channels, rb = (size_t)cols * 4, irb = (size_t)cols * 3;
    MICV_REQUIRE(stride >= srb && stride_ok(ostride, cols, 4) && astride >= irb && (!jet_u || jstride >= irb),
                 "micv_dense_lk_display_seq_host: bad stride");
    const int pairs = nframes - 1;
    for (int t = 0; t < nframes; t++) MICV_REQUIRE(frames[t] != nullptr, "micv_dense_lk_display_seq_host: frame %d is null", t);
    for (int p = 0; p < pairs; p++)
        MICV_REQUIRE(u[p] && v[p] && arrows[p] && (!jet_u || (jet_u[p] && jet_v[p])), "micv_dense_lk_display_seq_host: an output of pair %d is null", p);
    // one block of frames up, one block of outputs down: [u | v | arrows | jet_u | jet_v], each pairs images of one pitch
    const size_t fp = pitch256(srb * rows), op = pitch256(rb * rows), ip = pitch256(irb * rows);
    char *df = h.alloc<char>(fp * nframes);
    char *out = h.alloc<char>((2 * op + (jet_u ? 3 : 1) * ip) * pairs);
    if (!h.ok()) return h.finish();
    for (int t = 0; t < nframes; t++) h.up_to(df + t * fp, frames[t], stride, srb, rows);
    if (!h.ok()) return h.finish();
    float *du = reinterpret_cast<float *>(out), *dv = reinterpret_cast<float *>(out + op * pairs);
    uint8_t *da = reinterpret_cast<uint8_t *>(out + 2 * op * pairs);
    uint8_t *ju = jet_u ? da + ip * pairs : nullptr, *jv = jet_u ? ju + ip * pairs : nullptr;
    MICV_TRY(micv_dense_lk_display_seq_async(ctx, df, fp, nframes, rows, cols, srb, channels, depth, win, levels, color, du, dv, op, rb, da, ip, irb,
                                             ju, jv, ip, irb, h.s));
    for (int p = 0; p < pairs; p++) {
        h.down(u[p], ostride, reinterpret_cast<char *>(du) + p * op, rb, rows);
        h.down(v[p], ostride, reinterpret_cast<char *>(dv) + p * op, rb, rows);
        h.down(arrows[p], astride, da + p * ip, irb, rows);
        if (jet_u) {
            h.down(jet_u[p], jstride, ju + p * ip, irb, rows);
            h.down(jet_v[p], jstride, jv + p * ip, irb, rows);
        }
    }
    return h.finish();
}

// ---- ps4 driver (ps4.hip) ----------------------------------------------------------------------

int micv_draw_dots_host(micv_ctx *ctx, const void *gray, int depth, int rows, int cols, size_t gstride, const float *corners,
                        size_t cstride, uint8_t *dst, size_t dstride) {
    HostCall h(ctx, "micv_draw_dots_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(gray && corners && dst && rows > 0 && cols > 0, "micv_draw_dots_host: bad argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_draw_dots_host: depth %d not supported (8U, 32F)", depth);
    const size_t e = depth == MICV_DEPTH_32F ? 4 : 1, grb = (size_t)cols * e, crb = (size_t)cols * 4, drb = (size_t)cols * 3;
    MICV_REQUIRE(stride_ok(gstride, cols, e) && stride_ok(cstride, cols, 4) && dstride >= drb, "micv_draw_dots_host: bad stride");
    void *dg = h.up<void>(gray, gstride, grb, rows);
    float *dc = h.up<float>(corners, cstride, crb, rows);
    uint8_t *dd = h.alloc<uint8_t>(drb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_dots_dev(ctx, dg, depth, rows, cols, grb, dc, crb, dd, drb, h.s));
    h.down(dst, dstride, dd, drb, rows);
    return h.finish();
}

int micv_hconcat_host(micv_ctx *ctx, const uint8_t *a, size_t astride, int acols, const uint8_t *b, size_t bstride, int bcols,
                      int rows, int bpp, uint8_t *dst, size_t dstride) {
    HostCall h(ctx, "micv_hconcat_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(a && b && dst && rows > 0 && acols > 0 && bcols > 0 && (bpp == 1 || bpp == 3), "micv_hconcat_host: bad argument");
    const size_t arb = (size_t)acols * bpp, brb = (size_t)bcols * bpp;
    MICV_REQUIRE(astride >= arb && bstride >= brb && dstride >= arb + brb, "micv_hconcat_host: a stride is smaller than its row");
    uint8_t *da = h.up<uint8_t>(a, astride, arb, rows), *db = h.up<uint8_t>(b, bstride, brb, rows);
    uint8_t *dd = h.alloc<uint8_t>((arb + brb) * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_hconcat_dev(ctx, da, arb, acols, db, brb, bcols, rows, bpp, dd, arb + brb, h.s));
    h.down(dst, dstride, dd, arb + brb, rows);
    return h.finish();
}

int micv_draw_keypoints_host(micv_ctx *ctx, const uint8_t *src, int channels, int rows, int cols, size_t sstride, uint8_t *canvas,
                             int canvas_cols, size_t cstride, int x0, const float *kp_xysa, int64_t n, uint64_t *rng_state) {
    HostCall h(ctx, "micv_draw_keypoints_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(canvas && rng_state && rows > 0 && cols > 0 && n >= 0 && (n == 0 || kp_xysa), "micv_draw_keypoints_host: bad argument");
    MICV_REQUIRE(!src || channels == 1 || channels == 3, "micv_draw_keypoints_host: %d channels not supported (1 or 3)", channels);
    MICV_REQUIRE(x0 >= 0 && (int64_t)x0 + cols <= canvas_cols && cstride >= (size_t)canvas_cols * 3 &&
                     (!src || sstride >= (size_t)cols * channels),
                 "micv_draw_keypoints_host: the window does not lie in the canvas, or bad stride");
    // the window alone travels: it is a canvas of its own on the device
    const size_t srb = src ? (size_t)cols * channels : 16, prb = (size_t)cols * 3;
    uint8_t *window = canvas + 3 * (size_t)x0;
    uint8_t *ds = src ? h.up<uint8_t>(src, sstride, srb, rows) : nullptr;
    uint8_t *dp = src ? h.alloc<uint8_t>(prb * rows) : h.up<uint8_t>(window, cstride, prb, rows);
    float *dk = h.up<float>(kp_xysa, (size_t)n * 16);
    const int64_t words[2] = {n, (int64_t)*rng_state};
    int64_t *dw = h.up<int64_t>(words, 16);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_keypoints_dev(ctx, ds, channels, rows, cols, srb, dp, cols, prb, 0, dk, dw, n,
                                     reinterpret_cast<uint64_t *>(dw + 1), h.s));
    h.down(window, cstride, dp, prb, rows);
    h.down(rng_state, dw + 1, 8);
    return h.finish();
}

int micv_draw_match_lines_host(micv_ctx *ctx, uint8_t *canvas, int rows, int cols, size_t stride, const float *kp_a, int64_t na,
                               const float *kp_b, int64_t nb, const int32_t *matches_qt, int64_t n, const uint8_t *mask,
                               int x_offset, uint64_t seed) {
    HostCall h(ctx, "micv_draw_match_lines_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(canvas && rows > 0 && cols > 0 && stride >= (size_t)cols * 3 && na >= 0 && nb >= 0 && n >= 0,
                 "micv_draw_match_lines_host: bad argument");
    if (n == 0 || na == 0 || nb == 0) return MICV_OK;
    MICV_REQUIRE(kp_a && kp_b && matches_qt, "micv_draw_match_lines_host: null argument");
    const size_t rb = (size_t)cols * 3;
    uint8_t *dc = h.up<uint8_t>(canvas, stride, rb, rows);
    float *da = h.up<float>(kp_a, (size_t)na * 16), *db = h.up<float>(kp_b, (size_t)nb * 16);
    int32_t *dm = h.up<int32_t>(matches_qt, (size_t)n * 8);
    uint8_t *dk = mask ? h.up<uint8_t>(mask, (size_t)n) : nullptr;
    int64_t *dw = h.up<int64_t>(&n, 8);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_match_lines_dev(ctx, dc, rows, cols, rb, da, na, db, nb, dm, dw, n, dk, x_offset, seed, h.s));
    h.down(canvas, stride, dc, rb, rows);
    return h.finish();
}

int micv_ps4_harris_display_host(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                                 double sigma, float alpha, int flags, double threshold, int min_distance, float *fields,
                                 int32_t *locs_yx, int64_t cap, int64_t *count, uint8_t *grad_panel, size_t gstride,
                                 uint8_t *resp_u8, size_t rstride, uint8_t *dots, size_t dstride) {
    HostCall h(ctx, "micv_ps4_harris_display_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && fields && count && grad_panel && resp_u8 && dots && rows > 0 && cols > 0 && cap >= 0 && (cap == 0 || locs_yx),
                 "micv_ps4_harris_display_host: bad argument");
    const size_t n = (size_t)rows * cols, rb = (size_t)cols * 4;
    MICV_REQUIRE(stride_ok(stride, cols, 4) && gstride >= (size_t)2 * cols && rstride >= (size_t)cols && dstride >= (size_t)cols * 3,
                 "micv_ps4_harris_display_host: bad stride");
    float *di = h.up<float>(img, stride, rb, rows), *df = h.alloc<float>(n * 16);
    int32_t *dl = h.alloc<int32_t>(cap ? (size_t)cap * 8 : 16);
    int64_t *dn = h.alloc<int64_t>(8);
    uint8_t *dg = h.alloc<uint8_t>(2 * n), *dr = h.alloc<uint8_t>(n), *dd = h.alloc<uint8_t>(3 * n);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_ps4_harris_display_dev(ctx, di, rows, cols, rb, sobel_ksize, win, sigma, alpha, flags, threshold, min_distance, df, dl, cap,
                                         dn, dg, (size_t)2 * cols, dr, (size_t)cols, dd, (size_t)3 * cols, h.s));
    h.down(fields, df, n * 16);
    h.down(count, dn, 8);
    h.down(grad_panel, gstride, dg, (size_t)2 * cols, rows);
    h.down(resp_u8, rstride, dr, (size_t)cols, rows);
    h.down(dots, dstride, dd, (size_t)3 * cols, rows);
    MICV_TRY(h.finish());  // the count is here now
    const int64_t got = *count < cap ? *count : cap;
    if (got > 0) h.down(locs_yx, dl, (size_t)got * 8);
    return h.finish();
}

int micv_ps4_match_panels_host(micv_ctx *ctx, const uint8_t *img_a, size_t astride, int cols_a, const uint8_t *img_b, size_t bstride,
                               int cols_b, int rows, const float *kp_a, int64_t n_a, const float *kp_b, int64_t n_b,
                               const int32_t *matches_qt, int64_t n_matches, const uint8_t *mask, int flags, uint64_t seed,
                               uint64_t *rng_state, uint8_t *keypoint_panel, uint8_t *match_panel, size_t pstride) {
    HostCall h(ctx, "micv_ps4_match_panels_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img_a && img_b && match_panel && rng_state && rows > 0 && cols_a > 0 && cols_b > 0 && n_a >= 0 && n_b >= 0 &&
                     n_matches >= 0 && (n_a == 0 || kp_a) && (n_b == 0 || kp_b) && (n_matches == 0 || matches_qt),
                 "micv_ps4_match_panels_host: bad argument");
    const size_t prb = ((size_t)cols_a + cols_b) * 3;
    MICV_REQUIRE(astride >= (size_t)cols_a && bstride >= (size_t)cols_b && pstride >= prb, "micv_ps4_match_panels_host: bad stride");
    uint8_t *da = h.up<uint8_t>(img_a, astride, (size_t)cols_a, rows), *db = h.up<uint8_t>(img_b, bstride, (size_t)cols_b, rows);
    float *dka = h.up<float>(kp_a, (size_t)n_a * 16), *dkb = h.up<float>(kp_b, (size_t)n_b * 16);
    int32_t *dm = h.up<int32_t>(matches_qt, (size_t)n_matches * 8);
    uint8_t *dk = mask ? h.up<uint8_t>(mask, (size_t)n_matches) : nullptr;
    const int64_t words[4] = {n_a, n_b, n_matches, (int64_t)*rng_state};
    int64_t *w = h.up<int64_t>(words, 32);
    uint8_t *dp1 = keypoint_panel ? h.alloc<uint8_t>(prb * rows) : nullptr, *dp2 = h.alloc<uint8_t>(prb * rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_ps4_match_panels_dev(ctx, da, (size_t)cols_a, cols_a, db, (size_t)cols_b, cols_b, rows, dka, w, n_a, dkb, w + 1, n_b, dm,
                                       w + 2, n_matches, dk, flags, seed, reinterpret_cast<uint64_t *>(w + 3), dp1, dp2, prb, h.s));
    if (keypoint_panel) h.down(keypoint_panel, pstride, dp1, prb, rows);
    h.down(match_panel, pstride, dp2, prb, rows);
    h.down(rng_state, w + 3, 8);
    return h.finish();
}

// ---- ps6 driver (ps6.hip) ----------------------------------------------------------------------
// The image goes up with its pixels only; the padding of the caller's rows is never read or written.

int micv_draw_particles_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                             const double *color) {
    HostCall h(ctx, "micv_draw_particles_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && color && rows > 0 && cols > 0 && n >= 0 && (n == 0 || xy), "micv_draw_particles_host: bad argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_draw_particles_host: %d channels not supported (1, 3, 4)", channels);
    const size_t rb = (size_t)cols * channels;
    MICV_REQUIRE(stride >= rb, "micv_draw_particles_host: stride %zu < %zu", stride, rb);
    if (n == 0) return MICV_OK;
    uint8_t *di = h.up<uint8_t>(img, stride, rb, rows);
    float *dp = h.up<float>(xy, (size_t)n * 8);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_particles_dev(ctx, di, rows, cols, channels, rb, dp, n, color, h.s));
    h.down(img, stride, di, rb, rows);
    return h.finish();
}

int micv_draw_rectangle_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, int x, int y, int w, int hgt,
                             const double *color) {
    HostCall h(ctx, "micv_draw_rectangle_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && color && rows > 0 && cols > 0, "micv_draw_rectangle_host: bad argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_draw_rectangle_host: %d channels not supported (1, 3, 4)", channels);
    const size_t rb = (size_t)cols * channels;
    MICV_REQUIRE(stride >= rb, "micv_draw_rectangle_host: stride %zu < %zu", stride, rb);
    uint8_t *di = h.up<uint8_t>(img, stride, rb, rows);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_draw_rectangle_dev(ctx, di, rows, cols, channels, rb, x, y, w, hgt, color, h.s));
    h.down(img, stride, di, rb, rows);
    return h.finish();
}

int micv_ps6_overlay_list_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                               const double *dot_color, const float *centre, float bbox_w, float bbox_h, const double *box_color) {
    HostCall h(ctx, "micv_ps6_overlay_list_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && dot_color && centre && box_color && rows > 0 && cols > 0 && n >= 0 && (n == 0 || xy),
                 "micv_ps6_overlay_list_host: bad argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_ps6_overlay_list_host: %d channels not supported (1, 3, 4)",
                 channels);
    const size_t rb = (size_t)cols * channels;
    MICV_REQUIRE(stride >= rb, "micv_ps6_overlay_list_host: stride %zu < %zu", stride, rb);
    uint8_t *di = h.up<uint8_t>(img, stride, rb, rows);
    float *dp = h.up<float>(xy, (size_t)n * 8), *dc = h.up<float>(centre, 8);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_ps6_overlay_list_dev(ctx, di, rows, cols, channels, rb, dp, n, dot_color, dc, bbox_w, bbox_h, box_color, h.s));
    h.down(img, stride, di, rb, rows);
    return h.finish();
}

}  // extern "C"
