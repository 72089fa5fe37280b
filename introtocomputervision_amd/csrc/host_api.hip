// host_api.hip -- `_host` flavours: host pointers in, host pointers out, synchronous.
// This is the behaviour of the reference's cv::Mat functions (upload -> kernel -> sync ->
// download inside every call, e.g. Harris.cu:118-158, Pyramids.cu:45-72); it is PCIe-bound
// by construction.  Device buffers are allocated per call like the reference's GpuMats.
#include <atomic>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "common.hpp"

namespace micv {

// RAII device allocation; `ok()` reports failure through set_error.
// Device block of a host-pointer call, taken from the context's cache (no hipMalloc / hipFree on a
// repeated call of the same shape).  `io_ctx` is set by HOST_PROLOGUE.
static thread_local micv_ctx *io_ctx = nullptr;
struct DevBuf {
    void *p = nullptr;
    micv_ctx *owner;
    explicit DevBuf(size_t bytes) : owner(io_ctx) { p = owner ? owner->io_acquire(bytes) : nullptr; }
    ~DevBuf() {
        if (p) owner->io_release(p);
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

#define MICV_ALLOC_OK(buf)                                        \
    do {                                                          \
        if (!(buf).p) {                                           \
            ::micv::set_error("device allocation failed");        \
            return MICV_ENOMEM;                                   \
        }                                                         \
    } while (0)

// A continuous cv::Mat (step == row bytes: what cv::Mat::create gives) goes as ONE linear copy; only a
// pitched view (an ROI) needs the 2-D form.  Pageable host memory is fine: the runtime pins the pages
// for the transfer and reaches the same 53 GB/s as hipHostMalloc'd memory on this platform
// (tools/probes/pcie_probe.py), so there is no staging ring to copy through.
static int up2d(void *dst, const void *src, size_t sstride, size_t row_bytes, int rows,
                hipStream_t s) {
    if (sstride == row_bytes || rows == 1)
        MICV_HIP(hipMemcpyAsync(dst, src, row_bytes * (size_t)rows, hipMemcpyHostToDevice, s));
    else
        MICV_HIP(hipMemcpy2DAsync(dst, row_bytes, src, sstride, row_bytes, rows, hipMemcpyHostToDevice, s));
    return MICV_OK;
}
static int down2d(void *dst, size_t dstride, const void *src, size_t row_bytes, int rows,
                  hipStream_t s) {
    if (dstride == row_bytes || rows == 1)
        MICV_HIP(hipMemcpyAsync(dst, src, row_bytes * (size_t)rows, hipMemcpyDeviceToHost, s));
    else
        MICV_HIP(hipMemcpy2DAsync(dst, dstride, src, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, s));
    return MICV_OK;
}

}  // namespace micv

using namespace micv;

// Every `_host` function enqueues asynchronous copies; whichever way it returns (an error in a
// later step included) the stream is drained first, so no D2H copy into the caller's buffer is
// still in flight and no cached device block is handed out again while something uses it.
//
// Kernel-timing log lines: the reference brackets its kernels with a GpuTimer and
// logs "<kernel> execution took {} ms" (Harris.cu:144-155, DisparitySSD.cu:192-203, Hough.cu:277-289,
// Pyramids.cu:61-69).  With a sink registered (micv_set_kernel_log) the `_host` entry point of each of
// those functions records an event pair around its device call and, after the final synchronisation,
// hands (the reference's kernel name, milliseconds) to the sink; without one nothing is recorded.
static std::atomic<micv_kernel_log_fn> g_log_fn{nullptr};
static std::atomic<void *> g_log_user{nullptr};

struct HostSync {
    hipStream_t s;
    const char *name = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void begin(const char *kernel) {
        if (!g_log_fn.load(std::memory_order_relaxed)) return;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
        name = kernel;
        (void)hipEventRecord(e0, s);
    }
    void end() {
        if (name) (void)hipEventRecord(e1, s);
    }
    ~HostSync() {
        (void)hipStreamSynchronize(s);
        if (name) {
            float ms = 0.f;
            const micv_kernel_log_fn fn = g_log_fn.load(std::memory_order_relaxed);
            if (fn && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) fn(name, ms, g_log_user.load(std::memory_order_relaxed));
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// The device call of a `_host` function, bracketed for the kernel log (a no-op without a sink).
#define MICV_TIMED(kernel, call)       \
    do {                               \
        host_sync_.begin(kernel);      \
        const int rc_timed_ = (call);  \
        host_sync_.end();              \
        if (rc_timed_ != MICV_OK) return rc_timed_; \
    } while (0)

#define HOST_PROLOGUE(fn)                                    \
    MICV_REQUIRE(ctx != nullptr, fn ": ctx is null");        \
    MICV_HIP(hipSetDevice(ctx->device));                     \
    ::micv::io_ctx = ctx;                                    \
    hipStream_t s = nullptr;                                 \
    HostSync host_sync_{s}

extern "C" {

int micv_set_kernel_log(micv_kernel_log_fn fn, void *user) {
    g_log_user.store(user, std::memory_order_relaxed);
    g_log_fn.store(fn, std::memory_order_release);
    return MICV_OK;
}

int micv_lk_flow_pyr_host(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                          size_t stride, int win, int levels, float *u, float *v, size_t ostride) {
    HOST_PROLOGUE("micv_lk_flow_pyr_host");
    MICV_REQUIRE(prev && next && u && v && rows > 0 && cols > 0, "micv_lk_flow_pyr_host: bad argument");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && stride_ok(ostride, cols, 4),
                 "micv_lk_flow_pyr_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf dp(n), dn(n), du(n), dv(n);
    MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn); MICV_ALLOC_OK(du); MICV_ALLOC_OK(dv);
    MICV_TRY(up2d(dp.p, prev, stride, rb, rows, s));
    MICV_TRY(up2d(dn.p, next, stride, rb, rows, s));
    MICV_TRY(micv_lk_flow_pyr_dev(ctx, dp.as<float>(), dn.as<float>(), rows, cols, rb, win, levels,
                                  du.as<float>(), dv.as<float>(), rb, s));
    MICV_TRY(down2d(u, ostride, du.p, rb, rows, s));
    MICV_TRY(down2d(v, ostride, dv.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

/* lk::calcOpticalFlowPyr on frames as the ps5 driver hands them over (denseLKWrapper passes the
 * COLOUR frames, Solution.cpp:63; makeGaussianPyramid converts, Pyramids.cpp:9-15): one upload of
 * the interleaved frames, grey conversion on the device, then the pyramid chain. */
int micv_lk_flow_pyr_frames_host(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols,
                                 size_t stride, int channels, int depth, int win, int levels, float *u,
                                 float *v, size_t ostride) {
    HOST_PROLOGUE("micv_lk_flow_pyr_frames_host");
    MICV_REQUIRE(prev && next && u && v && rows > 0 && cols > 0, "micv_lk_flow_pyr_frames_host: bad argument");
    MICV_REQUIRE((channels == 1 || channels == 3 || channels == 4) &&
                     (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F),
                 "micv_lk_flow_pyr_frames_host: frames must be 1/3/4-channel 8U or 32F");
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)cols * channels * es;
    MICV_REQUIRE(stride >= srb && stride_ok(ostride, cols, 4), "micv_lk_flow_pyr_frames_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf cp(srb * rows), cn(srb * rows), dp(n), dn(n), du(n), dv(n);
    MICV_ALLOC_OK(cp); MICV_ALLOC_OK(cn); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn); MICV_ALLOC_OK(du); MICV_ALLOC_OK(dv);
    MICV_TRY(up2d(cp.p, prev, stride, srb, rows, s));
    MICV_TRY(up2d(cn.p, next, stride, srb, rows, s));
    MICV_TRY(micv_to_gray_f32_dev(ctx, cp.p, rows, cols, srb, channels, depth, dp.as<float>(), rb, s));
    MICV_TRY(micv_to_gray_f32_dev(ctx, cn.p, rows, cols, srb, channels, depth, dn.as<float>(), rb, s));
    MICV_TRY(micv_lk_flow_pyr_dev(ctx, dp.as<float>(), dn.as<float>(), rows, cols, rb, win, levels,
                                  du.as<float>(), dv.as<float>(), rb, s));
    MICV_TRY(down2d(u, ostride, du.p, rb, rows, s));
    MICV_TRY(down2d(v, ostride, dv.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
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
 * 0.27 ms per image: 0.65 ms).  Same bits as the per-pair calls. */
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
    MICV_HIP(hipSetDevice(ctx->device));
    ::micv::io_ctx = ctx;
    const bool convert = !(channels == 1 && depth == MICV_DEPTH_32F);
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    constexpr int RING = 3;
    DevBuf raw(convert ? srb * rows : 256), g0(n), g1(n), g2(n), u0(n), u1(n), u2(n), v0(n), v1(n), v2(n);
    MICV_ALLOC_OK(raw); MICV_ALLOC_OK(g0); MICV_ALLOC_OK(g1); MICV_ALLOC_OK(g2);
    MICV_ALLOC_OK(u0); MICV_ALLOC_OK(u1); MICV_ALLOC_OK(u2); MICV_ALLOC_OK(v0); MICV_ALLOC_OK(v1); MICV_ALLOC_OK(v2);
    float *grey[RING] = {g0.as<float>(), g1.as<float>(), g2.as<float>()};
    float *du[RING] = {u0.as<float>(), u1.as<float>(), u2.as<float>()}, *dv[RING] = {v0.as<float>(), v1.as<float>(), v2.as<float>()};
    const int npairs = nframes - 1;

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
            if (rc == MICV_OK) rc = down2d(u[p], ostride, du[p % RING], rb, rows, st.down[which]);
            if (rc == MICV_OK) rc = down2d(v[p], ostride, dv[p % RING], rb, rows, st.down[which]);
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
            MICV_TRY(up2d(raw.p, frames[t], stride, srb, rows, st.up));
            MICV_TRY(micv_to_gray_f32_dev(ctx, raw.p, rows, cols, srb, channels, depth, grey[t % RING], rb, st.up));
        } else {
            MICV_TRY(up2d(grey[t % RING], frames[t], stride, rb, rows, st.up));
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
    HOST_PROLOGUE("micv_to_gray_f32_host");
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0, "micv_to_gray_f32_host: bad argument");
    MICV_REQUIRE((channels == 1 || channels == 3 || channels == 4) &&
                     (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F),
                 "micv_to_gray_f32_host: source must be 1/3/4-channel 8U or 32F");
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)cols * channels * es;
    MICV_REQUIRE(sstride >= srb && stride_ok(dstride, cols, 4), "micv_to_gray_f32_host: bad stride");
    const size_t rb = (size_t)cols * 4;
    DevBuf cs(srb * rows), dd(rb * rows);
    MICV_ALLOC_OK(cs); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(cs.p, src, sstride, srb, rows, s));
    MICV_TRY(micv_to_gray_f32_dev(ctx, cs.p, rows, cols, srb, channels, depth, dd.as<float>(), rb, s));
    MICV_TRY(down2d(dst, dstride, dd.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_lk_flow_host(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                      size_t stride, int win, float *u, float *v, size_t ostride) {
    HOST_PROLOGUE("micv_lk_flow_host");
    MICV_REQUIRE(prev && next && u && v && rows > 0 && cols > 0, "micv_lk_flow_host: bad argument");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && stride_ok(ostride, cols, 4),
                 "micv_lk_flow_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf dp(n), dn(n), du(n), dv(n);
    MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn); MICV_ALLOC_OK(du); MICV_ALLOC_OK(dv);
    MICV_TRY(up2d(dp.p, prev, stride, rb, rows, s));
    MICV_TRY(up2d(dn.p, next, stride, rb, rows, s));
    MICV_TRY(micv_lk_flow_dev(ctx, dp.as<float>(), dn.as<float>(), rows, cols, rb, win,
                              du.as<float>(), dv.as<float>(), rb, s));
    MICV_TRY(down2d(u, ostride, du.p, rb, rows, s));
    MICV_TRY(down2d(v, ostride, dv.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_lk_warp_host(micv_ctx *ctx, const float *src, size_t sstride, const float *du,
                      const float *dv, size_t fstride, int rows, int cols, float *dst,
                      size_t dstride) {
    HOST_PROLOGUE("micv_lk_warp_host");
    MICV_REQUIRE(src && du && dv && dst && rows > 0 && cols > 0, "micv_lk_warp_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(fstride, cols, 4) &&
                     stride_ok(dstride, cols, 4),
                 "micv_lk_warp_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf ds(n), dU(n), dV(n), dd(n);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dU); MICV_ALLOC_OK(dV); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(ds.p, src, sstride, rb, rows, s));
    MICV_TRY(up2d(dU.p, du, fstride, rb, rows, s));
    MICV_TRY(up2d(dV.p, dv, fstride, rb, rows, s));
    MICV_TRY(micv_lk_warp_dev(ctx, ds.as<float>(), rb, dU.as<float>(), dV.as<float>(), rb, rows,
                              cols, dd.as<float>(), rb, s));
    MICV_TRY(down2d(dst, dstride, dd.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_pyr_down_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                       float *dst, size_t dstride) {
    HOST_PROLOGUE("micv_pyr_down_host");
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0, "micv_pyr_down_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(dstride, cols / 2, 4),
                 "micv_pyr_down_host: bad stride");
    const int dr = rows / 2, dc = cols / 2;
    DevBuf ds((size_t)rows * cols * 4), dd((size_t)dr * dc * 4);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(ds.p, src, sstride, (size_t)cols * 4, rows, s));
    MICV_TIMED("pyrDownsampleKernel", micv_pyr_down_dev(ctx, ds.as<float>(), rows, cols, (size_t)cols * 4, dd.as<float>(),
                               (size_t)dc * 4, s));
    if (dr > 0 && dc > 0) MICV_TRY(down2d(dst, dstride, dd.p, (size_t)dc * 4, dr, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_pyr_up_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                     float *dst, size_t dstride) {
    HOST_PROLOGUE("micv_pyr_up_host");
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0, "micv_pyr_up_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(dstride, 2 * cols, 4),
                 "micv_pyr_up_host: bad stride");
    DevBuf ds((size_t)rows * cols * 4), dd((size_t)rows * cols * 16);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(ds.p, src, sstride, (size_t)cols * 4, rows, s));
    MICV_TIMED("pyrUpsampleKernel", micv_pyr_up_dev(ctx, ds.as<float>(), rows, cols, (size_t)cols * 4, dd.as<float>(),
                             (size_t)cols * 8, s));
    MICV_TRY(down2d(dst, dstride, dd.p, (size_t)cols * 8, 2 * rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_gaussian_pyramid_host(micv_ctx *ctx, const float *src, int rows, int cols,
                               size_t sstride, int levels, float *const *dst_levels) {
    HOST_PROLOGUE("micv_gaussian_pyramid_host");
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
    DevBuf ds((size_t)rows * cols * 4), dd(total * 4);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(ds.p, src, sstride, (size_t)cols * 4, rows, s));
    float *lv[16];
    for (int l = 0; l < levels; l++) lv[l] = dd.as<float>() + off[l];
    MICV_TRY(micv_gaussian_pyramid_dev(ctx, ds.as<float>(), rows, cols, (size_t)cols * 4, levels, lv, s));
    for (int l = 0; l < levels; l++) {
        MICV_REQUIRE(dst_levels[l] != nullptr, "micv_gaussian_pyramid_host: dst_levels[%d] is null", l);
        MICV_HIP(hipMemcpyAsync(dst_levels[l], lv[l], (size_t)(rows >> l) * (cols >> l) * 4,
                                hipMemcpyDeviceToHost, s));
    }
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_sobel_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                    int ksize, float scale, float *gx, float *gy, size_t gstride) {
    HOST_PROLOGUE("micv_sobel_host");
    MICV_REQUIRE(src && gx && gy && rows > 0 && cols > 0, "micv_sobel_host: bad argument");
    MICV_REQUIRE(stride_ok(sstride, cols, 4) && stride_ok(gstride, cols, 4),
                 "micv_sobel_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf ds(n), dx(n), dy(n);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dx); MICV_ALLOC_OK(dy);
    MICV_TRY(up2d(ds.p, src, sstride, rb, rows, s));
    MICV_TRY(micv_sobel_dev(ctx, ds.as<float>(), rows, cols, rb, ksize, scale, dx.as<float>(),
                            dy.as<float>(), rb, s));
    MICV_TRY(down2d(gx, gstride, dx.p, rb, rows, s));
    MICV_TRY(down2d(gy, gstride, dy.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

}  // extern "C"

// ---- ps4 / ps2 / ps1 host flavours -----------------------------------------------------------
extern "C" {

int micv_harris_response_ex_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                                 size_t gstride, int win, double sigma, float alpha, int flags, float *resp,
                                 size_t rstride) {
    HOST_PROLOGUE("micv_harris_response_host");
    MICV_REQUIRE(gx && gy && resp && rows > 0 && cols > 0, "micv_harris_response_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4) && stride_ok(rstride, cols, 4),
                 "micv_harris_response_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf dx(n), dy(n), dr(n);
    MICV_ALLOC_OK(dx); MICV_ALLOC_OK(dy); MICV_ALLOC_OK(dr);
    MICV_TRY(up2d(dx.p, gx, gstride, rb, rows, s));
    MICV_TRY(up2d(dy.p, gy, gstride, rb, rows, s));
    MICV_TIMED("cornerResponseKernel", micv_harris_response_ex_dev(ctx, dx.as<float>(), dy.as<float>(), rows, cols, rb, win,
                                      sigma, alpha, flags, dr.as<float>(), rb, s));
    MICV_TRY(down2d(resp, rstride, dr.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_harris_response_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                              size_t gstride, int win, double sigma, float alpha, float *resp,
                              size_t rstride) {
    return micv_harris_response_ex_host(ctx, gx, gy, rows, cols, gstride, win, sigma, alpha, 0, resp, rstride);
}

int micv_harris_refine_host(micv_ctx *ctx, const float *resp, int rows, int cols, size_t rstride,
                            double threshold, int min_distance, float *corners, size_t cstride,
                            int32_t *locs_yx, int64_t cap, int64_t *count) {
    HOST_PROLOGUE("micv_harris_refine_host");
    MICV_REQUIRE(resp && corners && count && rows > 0 && cols > 0 && cap >= 0,
                 "micv_harris_refine_host: bad argument");
    MICV_REQUIRE(stride_ok(rstride, cols, 4) && stride_ok(cstride, cols, 4),
                 "micv_harris_refine_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf dr(n), dc(n), dl((size_t)cap * 8), dn(8);
    MICV_ALLOC_OK(dr); MICV_ALLOC_OK(dc); MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dn);
    MICV_TRY(up2d(dr.p, resp, rstride, rb, rows, s));
    MICV_TIMED("refineCornersKernel", micv_harris_refine_dev(ctx, dr.as<float>(), rows, cols, rb, threshold, min_distance,
                                    dc.as<float>(), rb, dl.as<int32_t>(), cap, dn.as<int64_t>(), s));
    MICV_TRY(down2d(corners, cstride, dc.p, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(count, dn.p, 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    const int64_t take = *count < cap ? *count : cap;
    if (take > 0) MICV_HIP(hipMemcpy(locs_yx, dl.p, (size_t)take * 8, hipMemcpyDeviceToHost));
    return MICV_OK;
}

int micv_harris_corners_host(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                             double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                             size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                             int64_t cap, int64_t *count) {
    HOST_PROLOGUE("micv_harris_corners_host");
    MICV_REQUIRE(img && count && rows > 0 && cols > 0 && cap >= 0 && (locs_yx || cap == 0), "micv_harris_corners_host: bad argument");
    MICV_REQUIRE((gx == nullptr) == (gy == nullptr), "micv_harris_corners_host: give both gradient outputs or neither");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && (!gx || stride_ok(gstride, cols, 4)) && (!resp || stride_ok(rstride, cols, 4)) &&
                     (!corners || stride_ok(cstride, cols, 4)),
                 "micv_harris_corners_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    // one upload, every requested field downloaded: what three _host calls move three times
    DevBuf di(n), dgx(gx ? n : 0), dgy(gy ? n : 0), dr(resp ? n : 0), dc(corners ? n : 0), dl((size_t)cap * 8), dn(8);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dn);
    if (gx) { MICV_ALLOC_OK(dgx); MICV_ALLOC_OK(dgy); }
    if (resp) MICV_ALLOC_OK(dr);
    if (corners) MICV_ALLOC_OK(dc);
    MICV_TRY(up2d(di.p, img, stride, rb, rows, s));
    MICV_TIMED("harrisCornersChain",
               micv_harris_corners_dev(ctx, di.as<float>(), rows, cols, rb, sobel_ksize, win, sigma, alpha, flags, threshold, min_distance,
                                       gx ? dgx.as<float>() : nullptr, gy ? dgy.as<float>() : nullptr, rb, resp ? dr.as<float>() : nullptr, rb,
                                       corners ? dc.as<float>() : nullptr, rb, dl.as<int32_t>(), cap, dn.as<int64_t>(), s));
    if (gx) {
        MICV_TRY(down2d(gx, gstride, dgx.p, rb, rows, s));
        MICV_TRY(down2d(gy, gstride, dgy.p, rb, rows, s));
    }
    if (resp) MICV_TRY(down2d(resp, rstride, dr.p, rb, rows, s));
    if (corners) MICV_TRY(down2d(corners, cstride, dc.p, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(count, dn.p, 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    const int64_t take = *count < cap ? *count : cap;
    if (take > 0) MICV_HIP(hipMemcpy(locs_yx, dl.p, (size_t)take * 8, hipMemcpyDeviceToHost));
    return MICV_OK;
}

int micv_sift_angles_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                          size_t gstride, float *angles, size_t astride) {
    HOST_PROLOGUE("micv_sift_angles_host");
    MICV_REQUIRE(gx && gy && angles && rows > 0 && cols > 0, "micv_sift_angles_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4) && stride_ok(astride, cols, 4),
                 "micv_sift_angles_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf dx(n), dy(n), da(n);
    MICV_ALLOC_OK(dx); MICV_ALLOC_OK(dy); MICV_ALLOC_OK(da);
    MICV_TRY(up2d(dx.p, gx, gstride, rb, rows, s));
    MICV_TRY(up2d(dy.p, gy, gstride, rb, rows, s));
    MICV_TRY(micv_sift_angles_dev(ctx, dx.as<float>(), dy.as<float>(), rows, cols, rb,
                                  da.as<float>(), rb, s));
    MICV_TRY(down2d(angles, astride, da.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_sift_keypoints_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                             size_t gstride, const int32_t *locs_yx, int64_t n, float size,
                             float *kp_xysa) {
    HOST_PROLOGUE("micv_sift_keypoints_host");
    MICV_REQUIRE(gx && gy && rows > 0 && cols > 0 && n >= 0 && (n == 0 || (locs_yx && kp_xysa)),
                 "micv_sift_keypoints_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4), "micv_sift_keypoints_host: bad stride");
    for (int64_t i = 0; i < n; i++)
        MICV_REQUIRE((unsigned)locs_yx[2 * i] < (unsigned)rows && (unsigned)locs_yx[2 * i + 1] < (unsigned)cols,
                     "micv_sift_keypoints_host: corner %lld outside the image", (long long)i);
    if (n == 0) return MICV_OK;
    const size_t rb = (size_t)cols * 4, bytes = rb * rows;
    DevBuf dx(bytes), dy(bytes), dl((size_t)n * 8), dk((size_t)n * 16);
    MICV_ALLOC_OK(dx); MICV_ALLOC_OK(dy); MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dk);
    MICV_TRY(up2d(dx.p, gx, gstride, rb, rows, s));
    MICV_TRY(up2d(dy.p, gy, gstride, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(dl.p, locs_yx, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_sift_keypoints_dev(ctx, dx.as<float>(), dy.as<float>(), rows, cols, rb,
                                     dl.as<int32_t>(), n, size, dk.as<float>(), s));
    MICV_HIP(hipMemcpyAsync(kp_xysa, dk.p, (size_t)n * 16, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_sift_descriptors_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                               size_t gstride, const float *kp_xysa, int64_t n, float *desc,
                               size_t dstride) {
    HOST_PROLOGUE("micv_sift_descriptors_host");
    MICV_REQUIRE(gx && gy && rows > 0 && cols > 0 && n >= 0 && (n == 0 || (kp_xysa && desc)),
                 "micv_sift_descriptors_host: bad argument");
    MICV_REQUIRE(stride_ok(gstride, cols, 4) && dstride % 4 == 0 && dstride >= 512,
                 "micv_sift_descriptors_host: bad stride");
    if (n == 0) return MICV_OK;
    const size_t rb = (size_t)cols * 4, bytes = rb * rows;
    DevBuf dx(bytes), dy(bytes), dk((size_t)n * 16), dd((size_t)n * 512);
    MICV_ALLOC_OK(dx); MICV_ALLOC_OK(dy); MICV_ALLOC_OK(dk); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(dx.p, gx, gstride, rb, rows, s));
    MICV_TRY(up2d(dy.p, gy, gstride, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(dk.p, kp_xysa, (size_t)n * 16, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_sift_descriptors_dev(ctx, dx.as<float>(), dy.as<float>(), rows, cols, rb, dk.as<float>(), n,
                                       dd.as<float>(), 512, s));
    MICV_TRY(down2d(desc, dstride, dd.p, 512, (int)n, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

static int stereo_host(bool ncc, micv_ctx *ctx, const float *left, const float *right, int rows,
                       int cols, size_t stride, int rad, int min_d, int max_d, int flags,
                       int8_t *disp, size_t dstride) {
    HOST_PROLOGUE("micv_disparity_host");
    MICV_REQUIRE(left && right && disp && rows > 0 && cols > 0, "micv_disparity_host: bad argument");
    MICV_REQUIRE(stride_ok(stride, cols, 4) && dstride >= (size_t)cols, "micv_disparity_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf dl(n), dr(n), dd((size_t)rows * cols);
    MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dr); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(dl.p, left, stride, rb, rows, s));
    MICV_TRY(up2d(dr.p, right, stride, rb, rows, s));
    if (ncc)
        MICV_TIMED("disparityNCorrKernel", micv_disparity_ncorr_dev(ctx, dl.as<float>(), dr.as<float>(), rows, cols, rb, rad,
                                          min_d, max_d, flags, dd.as<int8_t>(), cols, s));
    else
        MICV_TIMED("disparitySSDKernel", micv_disparity_ssd_dev(ctx, dl.as<float>(), dr.as<float>(), rows, cols, rb, rad,
                                        min_d, max_d, flags, dd.as<int8_t>(), cols, s));
    MICV_TRY(down2d(disp, dstride, dd.p, (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
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

int micv_hough_lines_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                          unsigned rho_bin, unsigned theta_bin, int32_t *acc) {
    HOST_PROLOGUE("micv_hough_lines_host");
    MICV_REQUIRE(mask && acc && mstride >= (size_t)cols, "micv_hough_lines_host: bad argument");
    int rb, tb;
    MICV_TRY(micv_hough_lines_dims(rows, cols, rho_bin, theta_bin, &rb, &tb));
    DevBuf dm((size_t)rows * cols), da((size_t)rb * tb * 4);
    MICV_ALLOC_OK(dm); MICV_ALLOC_OK(da);
    MICV_TRY(up2d(dm.p, mask, mstride, (size_t)cols, rows, s));
    MICV_TIMED("houghLinesAccumulateKernel", micv_hough_lines_dev(ctx, dm.as<uint8_t>(), rows, cols, cols, rho_bin, theta_bin,
                                  da.as<int32_t>(), s));
    MICV_HIP(hipMemcpyAsync(acc, da.p, (size_t)rb * tb * 4, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_hough_circles_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols,
                            size_t mstride, unsigned radius, int32_t *acc) {
    HOST_PROLOGUE("micv_hough_circles_host");
    MICV_REQUIRE(mask && acc && rows > 0 && cols > 0 && mstride >= (size_t)cols,
                 "micv_hough_circles_host: bad argument");
    DevBuf dm((size_t)rows * cols), da((size_t)rows * cols * 4);
    MICV_ALLOC_OK(dm); MICV_ALLOC_OK(da);
    MICV_TRY(up2d(dm.p, mask, mstride, (size_t)cols, rows, s));
    MICV_TIMED("houghCirclesAccumulateKernel", micv_hough_circles_dev(ctx, dm.as<uint8_t>(), rows, cols, cols, radius,
                                    da.as<int32_t>(), s));
    MICV_HIP(hipMemcpyAsync(acc, da.p, (size_t)rows * cols * 4, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_hough_peaks_host(micv_ctx *ctx, const int32_t *acc, int rows, int cols,
                          unsigned num_peaks, int threshold, uint32_t *peaks_rc, int64_t *count) {
    HOST_PROLOGUE("micv_hough_peaks_host");
    MICV_REQUIRE(acc && count && rows > 0 && cols > 0 && (peaks_rc || num_peaks == 0),
                 "micv_hough_peaks_host: bad argument");
    MICV_REQUIRE((int64_t)rows * cols < ((int64_t)1 << 31) && num_peaks <= 4096,  // before the upload
                 "micv_hough_peaks_host: %dx%d accumulator / %u peaks not supported (< 2^31 cells, <= 4096 peaks)",
                 rows, cols, num_peaks);
    DevBuf da((size_t)rows * cols * 4), dp((size_t)num_peaks * 8 + 8), dn(8);
    MICV_ALLOC_OK(da); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn);
    MICV_HIP(hipMemcpyAsync(da.p, acc, (size_t)rows * cols * 4, hipMemcpyHostToDevice, s));
    MICV_TIMED("findLocalMaximaKernel", micv_hough_peaks_dev(ctx, da.as<int32_t>(), rows, cols, num_peaks, threshold,
                                  dp.as<uint32_t>(), dn.as<int64_t>(), s));
    MICV_HIP(hipMemcpyAsync(count, dn.p, 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    if (*count > 0) MICV_HIP(hipMemcpy(peaks_rc, dp.p, (size_t)*count * 8, hipMemcpyDeviceToHost));
    return MICV_OK;
}

// ---- host-pointer flavours of the "next" rows --------------------------

int micv_generate_edge_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride,
                            int gauss_size, double gauss_sigma, double low_thresh,
                            double high_thresh, uint8_t *edges, size_t estride) {
    HOST_PROLOGUE("micv_generate_edge_host");
    MICV_REQUIRE(src && edges && rows > 0 && cols > 0 && stride >= (size_t)cols && estride >= (size_t)cols,
                 "micv_generate_edge_host: bad argument");
    DevBuf ds((size_t)rows * cols), de((size_t)rows * cols);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(de);
    MICV_TRY(up2d(ds.p, src, stride, (size_t)cols, rows, s));
    MICV_TRY(micv_generate_edge_dev(ctx, ds.as<uint8_t>(), rows, cols, cols, gauss_size, gauss_sigma,
                                    low_thresh, high_thresh, de.as<uint8_t>(), cols, s));
    MICV_TRY(down2d(edges, estride, de.p, (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_bf_knn2_host(micv_ctx *ctx, const float *query, int nq, size_t qstride, const float *train,
                      int nt, size_t tstride, int dim, int32_t *idx2, float *dist2) {
    HOST_PROLOGUE("micv_bf_knn2_host");
    MICV_REQUIRE(query && train && idx2 && dist2 && nq > 0 && nt >= 2 && dim > 0 &&
                     stride_ok(qstride, dim, 4) && stride_ok(tstride, dim, 4),
                 "micv_bf_knn2_host: bad argument");
    const size_t rb = (size_t)dim * 4;
    DevBuf dq(rb * nq), dt(rb * nt), di((size_t)nq * 8), dd((size_t)nq * 8);
    MICV_ALLOC_OK(dq); MICV_ALLOC_OK(dt); MICV_ALLOC_OK(di); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(dq.p, query, qstride, rb, nq, s));
    MICV_TRY(up2d(dt.p, train, tstride, rb, nt, s));
    MICV_TRY(micv_bf_knn2_dev(ctx, dq.as<float>(), nq, rb, dt.as<float>(), nt, rb, dim, di.as<int32_t>(),
                              dd.as<float>(), s));
    MICV_HIP(hipMemcpyAsync(idx2, di.p, (size_t)nq * 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(dist2, dd.p, (size_t)nq * 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_bf_ratio_filter_host(micv_ctx *ctx, const int32_t *idx2, const float *dist2, int nq,
                              double ratio, int32_t *matches_qt, float *distances, int64_t cap,
                              int64_t *count) {
    HOST_PROLOGUE("micv_bf_ratio_filter_host");
    MICV_REQUIRE(idx2 && dist2 && count && nq > 0 && cap >= 0 && (cap == 0 || (matches_qt && distances)),
                 "micv_bf_ratio_filter_host: bad argument");
    DevBuf di((size_t)nq * 8), dd((size_t)nq * 8), dm((size_t)cap * 8 + 8), dl((size_t)cap * 4 + 8), dn(8);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dd); MICV_ALLOC_OK(dm); MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dn);
    MICV_HIP(hipMemcpyAsync(di.p, idx2, (size_t)nq * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dd.p, dist2, (size_t)nq * 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_bf_ratio_filter_dev(ctx, di.as<int32_t>(), dd.as<float>(), nq, ratio, dm.as<int32_t>(),
                                      dl.as<float>(), cap, dn.as<int64_t>(), s));
    MICV_HIP(hipMemcpyAsync(count, dn.p, 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    const int64_t n = *count < cap ? *count : cap;
    if (n > 0) {
        MICV_HIP(hipMemcpy(matches_qt, dm.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        MICV_HIP(hipMemcpy(distances, dl.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return MICV_OK;
}

int micv_ransac_solve_host(micv_ctx *ctx, const float *src_xy, const float *dst_xy, int64_t n,
                           const int32_t *samples, int iters, int type, int thresh, double min_ratio,
                           float *transforms, uint8_t *inlier_mask, int32_t *stats) {
    HOST_PROLOGUE("micv_ransac_solve_host");
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
    DevBuf dsrc((size_t)n * 8), ddst((size_t)n * 8), dsam(ns * 4), dt(48), dm((size_t)n), dst(12);
    MICV_ALLOC_OK(dsrc); MICV_ALLOC_OK(ddst); MICV_ALLOC_OK(dsam); MICV_ALLOC_OK(dt); MICV_ALLOC_OK(dm);
    MICV_ALLOC_OK(dst);
    MICV_HIP(hipMemcpyAsync(dsrc.p, src_xy, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(ddst.p, dst_xy, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dsam.p, samples, ns * 4, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_ransac_solve_dev(ctx, dsrc.as<float>(), ddst.as<float>(), n, dsam.as<int32_t>(), iters, type,
                                   thresh, min_ratio, dt.as<float>(), dm.as<uint8_t>(), dst.as<int32_t>(), s));
    MICV_HIP(hipMemcpyAsync(transforms, dt.p, 48, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(inlier_mask, dm.p, (size_t)n, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(stats, dst.p, 12, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_mhi_frame_difference_host(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows,
                                   int cols, size_t stride, double thresh, int blur_w, int blur_h,
                                   double blur_sigma, uint8_t *diff, size_t dstride) {
    HOST_PROLOGUE("micv_mhi_frame_difference_host");
    MICV_REQUIRE(f1 && f2 && diff && rows > 0 && cols > 0 && stride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_frame_difference_host: bad argument");
    const size_t n = (size_t)rows * cols;
    DevBuf d1(n), d2(n), dd(n);
    MICV_ALLOC_OK(d1); MICV_ALLOC_OK(d2); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(d1.p, f1, stride, (size_t)cols, rows, s));
    MICV_TRY(up2d(d2.p, f2, stride, (size_t)cols, rows, s));
    MICV_TRY(micv_mhi_frame_difference_dev(ctx, d1.as<uint8_t>(), d2.as<uint8_t>(), rows, cols, cols, thresh,
                                           blur_w, blur_h, blur_sigma, dd.as<uint8_t>(), cols, s));
    MICV_TRY(down2d(diff, dstride, dd.p, (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_mhi_energy_host(micv_ctx *ctx, const uint8_t *mhi, int rows, int cols, size_t sstride,
                         uint8_t *mei, size_t dstride) {
    HOST_PROLOGUE("micv_mhi_energy_host");
    MICV_REQUIRE(mhi && mei && rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_energy_host: bad argument");
    const size_t n = (size_t)rows * cols;
    DevBuf ds(n), dd(n);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(ds.p, mhi, sstride, (size_t)cols, rows, s));
    MICV_TRY(micv_mhi_energy_dev(ctx, ds.as<uint8_t>(), rows, cols, cols, dd.as<uint8_t>(), cols, s));
    MICV_TRY(down2d(mei, dstride, dd.p, (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_mhi_threshold_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride,
                            double thresh, uint8_t *dst, size_t dstride) {
    HOST_PROLOGUE("micv_mhi_threshold_host");
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_threshold_host: bad argument");
    const size_t n = (size_t)rows * cols;
    DevBuf ds(n), dd(n);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(ds.p, src, sstride, (size_t)cols, rows, s));
    MICV_TRY(micv_mhi_threshold_dev(ctx, ds.as<uint8_t>(), rows, cols, cols, thresh, dd.as<uint8_t>(), cols, s));
    MICV_TRY(down2d(dst, dstride, dd.p, (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_mhi_update_host(micv_ctx *ctx, uint8_t *history, size_t hstride, const uint8_t *mask,
                         size_t mstride, int rows, int cols, int tau) {
    HOST_PROLOGUE("micv_mhi_update_host");
    MICV_REQUIRE(history && mask && rows > 0 && cols > 0 && hstride >= (size_t)cols && mstride >= (size_t)cols,
                 "micv_mhi_update_host: bad argument");
    const size_t n = (size_t)rows * cols;
    DevBuf dh(n), dm(n);
    MICV_ALLOC_OK(dh); MICV_ALLOC_OK(dm);
    MICV_TRY(up2d(dh.p, history, hstride, (size_t)cols, rows, s));
    MICV_TRY(up2d(dm.p, mask, mstride, (size_t)cols, rows, s));
    MICV_TRY(micv_mhi_update_dev(ctx, dh.as<uint8_t>(), cols, dm.as<uint8_t>(), cols, rows, cols, tau, s));
    MICV_TRY(down2d(history, hstride, dh.p, (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}


int micv_mhi_history_seq_host(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride,
                              int rows, int cols, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                              const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride) {
    HOST_PROLOGUE("micv_mhi_history_seq_host");
    MICV_REQUIRE(frames && save && out && nframes >= 2 && nsave >= 1 && rows > 0 && cols > 0 &&
                     stride >= (size_t)cols && frame_pitch >= stride * (size_t)rows && out_stride >= (size_t)cols &&
                     (nsave == 1 || out_pitch >= out_stride * (size_t)rows),
                 "micv_mhi_history_seq_host: bad argument");
    const size_t n = (size_t)rows * cols;
    DevBuf df(n * nframes), dout(n * nsave);
    MICV_ALLOC_OK(df); MICV_ALLOC_OK(dout);
    for (int f = 0; f < nframes; f++)
        MICV_TRY(up2d(df.as<uint8_t>() + n * f, frames + (size_t)f * frame_pitch, stride, (size_t)cols, rows, s));
    MICV_TRY(micv_mhi_history_seq_dev(ctx, df.as<uint8_t>(), nframes, n, cols, rows, cols, thresh, blur_w, blur_h,
                                      blur_sigma, tau, save, nsave, dout.as<uint8_t>(), n, cols, s));
    for (int i = 0; i < nsave; i++)
        MICV_TRY(down2d(out + (size_t)i * out_pitch, out_stride, dout.as<uint8_t>() + n * i, (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_central_moments_host(micv_ctx *ctx, const void *imgs, int batch, size_t img_pitch, size_t stride, int rows,
                              int cols, int type, const int *orders, int n, uint32_t flags, float *mu, float *eta,
                              float *raw) {
    HOST_PROLOGUE("micv_central_moments_host");
    MICV_REQUIRE(imgs && orders && mu && eta && batch > 0 && rows > 0 && cols > 0 && n >= 1 &&
                     n <= MICV_MOMENTS_MAX_ORDERS && (type == MICV_MOMENTS_U8 || type == MICV_MOMENTS_F32),
                 "micv_central_moments_host: bad argument");
    const size_t elem = type == MICV_MOMENTS_F32 ? 4 : 1, row_bytes = (size_t)cols * elem;
    MICV_REQUIRE(stride >= row_bytes && (batch == 1 || img_pitch >= stride * (size_t)rows),
                 "micv_central_moments_host: bad stride / pitch");
    const size_t img = row_bytes * rows;
    DevBuf di(img * batch), dout(sizeof(float) * (size_t)batch * (2 * n + 3));
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dout);
    for (int b = 0; b < batch; b++)
        MICV_TRY(up2d(di.as<uint8_t>() + img * b, static_cast<const uint8_t *>(imgs) + (size_t)b * img_pitch, stride,
                      row_bytes, rows, s));
    float *dmu = dout.as<float>(), *deta = dmu + (size_t)batch * n, *draw = deta + (size_t)batch * n;
    MICV_TRY(micv_central_moments_dev(ctx, di.p, batch, img, row_bytes, rows, cols, type, orders, n, flags, dmu, deta,
                                      draw, s));
    MICV_HIP(hipMemcpyAsync(mu, dmu, sizeof(float) * batch * n, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(eta, deta, sizeof(float) * batch * n, hipMemcpyDeviceToHost, s));
    if (raw) MICV_HIP(hipMemcpyAsync(raw, draw, sizeof(float) * batch * 3, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_knn_predict_host(micv_ctx *ctx, const float *train, int ntrain, size_t train_stride, const int *train_labels,
                          const float *test, int ntest, size_t test_stride, int dims, int k, uint32_t flags, int *pred) {
    HOST_PROLOGUE("micv_knn_predict_host");
    MICV_REQUIRE(train && train_labels && test && pred && ntrain >= 1 && ntest >= 1 && dims >= 1 &&
                     dims <= MICV_KNN_MAX_DIMS && train_stride >= sizeof(float) * dims &&
                     test_stride >= sizeof(float) * dims,
                 "micv_knn_predict_host: bad argument");
    const size_t rb = sizeof(float) * dims;
    DevBuf dt(rb * ntrain), dl(sizeof(int) * ntrain), dq(rb * ntest), dp(sizeof(int) * ntest);
    MICV_ALLOC_OK(dt); MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dq); MICV_ALLOC_OK(dp);
    MICV_TRY(up2d(dt.p, train, train_stride, rb, ntrain, s));
    MICV_HIP(hipMemcpyAsync(dl.p, train_labels, sizeof(int) * ntrain, hipMemcpyHostToDevice, s));
    MICV_TRY(up2d(dq.p, test, test_stride, rb, ntest, s));
    MICV_TRY(micv_knn_predict_dev(ctx, dt.as<float>(), ntrain, rb, dl.as<int>(), dq.as<float>(), ntest, rb, dims, k,
                                  flags, dp.as<int>(), s));
    MICV_HIP(hipMemcpyAsync(pred, dp.p, sizeof(int) * ntest, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_knn_confusion_host(micv_ctx *ctx, const float *features, int n, size_t stride, int dims, const int *labels,
                            const int *groups, int num_labels, int num_groups, int k, uint32_t flags, float *confusion,
                            int *pred, int *left_out) {
    HOST_PROLOGUE("micv_knn_confusion_host");
    MICV_REQUIRE(features && labels && confusion && n >= 1 && dims >= 1 && dims <= MICV_KNN_MAX_DIMS &&
                     stride >= sizeof(float) * dims && num_labels >= 1 && num_labels <= MICV_KNN_MAX_LABELS &&
                     (!groups || (num_groups >= 1 && num_groups <= MICV_KNN_MAX_GROUPS)),
                 "micv_knn_confusion_host: bad argument");
    const size_t rb = sizeof(float) * dims;
    const int nmat = groups ? num_groups + 1 : 1;
    const size_t mat_bytes = sizeof(float) * (size_t)nmat * num_labels * num_labels;
    DevBuf df(rb * n), dl(sizeof(int) * n), dg(groups ? sizeof(int) * n : 1), dp(sizeof(int) * n),
        dm(mat_bytes + sizeof(int));
    MICV_ALLOC_OK(df); MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dg); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dm);
    MICV_TRY(up2d(df.p, features, stride, rb, n, s));
    MICV_HIP(hipMemcpyAsync(dl.p, labels, sizeof(int) * n, hipMemcpyHostToDevice, s));
    if (groups) MICV_HIP(hipMemcpyAsync(dg.p, groups, sizeof(int) * n, hipMemcpyHostToDevice, s));
    int *dleft = reinterpret_cast<int *>(dm.as<char>() + mat_bytes);
    MICV_TRY(micv_knn_confusion_dev(ctx, df.as<float>(), n, rb, dims, dl.as<int>(), groups ? dg.as<int>() : nullptr,
                                    num_labels, num_groups, k, flags, dm.as<float>(), dp.as<int>(), dleft, s));
    MICV_HIP(hipMemcpyAsync(confusion, dm.p, mat_bytes, hipMemcpyDeviceToHost, s));
    if (pred) MICV_HIP(hipMemcpyAsync(pred, dp.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    if (left_out) MICV_HIP(hipMemcpyAsync(left_out, dleft, sizeof(int), hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
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
    HOST_PROLOGUE("micv_calib_ls_trials_host");
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
    DevBuf d2((size_t)n * 8), d3((size_t)n * 12), di(ni * 4), dk((size_t)T * 4), dM((size_t)T * 48), dr((size_t)T * 8),
        dbi(nr * 4), dbr(nr * 8), dbm(nr * 48), dst(4);
    MICV_ALLOC_OK(d2); MICV_ALLOC_OK(d3); MICV_ALLOC_OK(di); MICV_ALLOC_OK(dk); MICV_ALLOC_OK(dM); MICV_ALLOC_OK(dr);
    MICV_ALLOC_OK(dbi); MICV_ALLOC_OK(dbr); MICV_ALLOC_OK(dbm); MICV_ALLOC_OK(dst);
    MICV_HIP(hipMemcpyAsync(d2.p, pts2d, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(d3.p, pts3d, (size_t)n * 12, hipMemcpyHostToDevice, s));
    if (indices) MICV_HIP(hipMemcpyAsync(di.p, indices, ni * 4, hipMemcpyHostToDevice, s));
    if (kcount) MICV_HIP(hipMemcpyAsync(dk.p, kcount, (size_t)T * 4, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_calib_ls_trials_dev(ctx, d2.as<float>(), d3.as<float>(), n, indices ? di.as<int32_t>() : nullptr,
                                      stride, k, j, T, kcount ? dk.as<int32_t>() : nullptr, group_sizes, G, flags,
                                      dM.as<float>(), dr.as<double>(), best_idx ? dbi.as<int32_t>() : nullptr,
                                      best_idx ? dbr.as<double>() : nullptr, best_idx ? dbm.as<float>() : nullptr,
                                      dst.as<int32_t>(), s));
    MICV_HIP(hipMemcpyAsync(M, dM.p, (size_t)T * 48, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(residual, dr.p, (size_t)T * 8, hipMemcpyDeviceToHost, s));
    if (best_idx) {
        MICV_HIP(hipMemcpyAsync(best_idx, dbi.p, nr * 4, hipMemcpyDeviceToHost, s));
        MICV_HIP(hipMemcpyAsync(best_res, dbr.p, nr * 8, hipMemcpyDeviceToHost, s));
        MICV_HIP(hipMemcpyAsync(best_M, dbm.p, nr * 48, hipMemcpyDeviceToHost, s));
    }
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

// The shape shared by the SVD and the fundamental solve: two point arrays, an index list, `per` floats out per system.
extern "C++" template <typename Fn>
static int geom_solve_host(micv_ctx *ctx, hipStream_t s, const char *fn, const float *pa, size_t abytes, const float *pb,
                           size_t bbytes, int n, const int32_t *indices, int stride, int k, int T, int per, float *out,
                           Fn call) {
    MICV_TRY(geom_indices_ok(fn, indices, stride, T, nullptr, k, 0, n));
    const size_t ni = indices ? (size_t)T * stride : 1;
    DevBuf da(abytes), db(bbytes), di(ni * 4), dout((size_t)T * per * 4), dst(4);
    MICV_ALLOC_OK(da); MICV_ALLOC_OK(db); MICV_ALLOC_OK(di); MICV_ALLOC_OK(dout); MICV_ALLOC_OK(dst);
    MICV_HIP(hipMemcpyAsync(da.p, pa, abytes, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(db.p, pb, bbytes, hipMemcpyHostToDevice, s));
    if (indices) MICV_HIP(hipMemcpyAsync(di.p, indices, ni * 4, hipMemcpyHostToDevice, s));
    MICV_TRY(call(da.as<float>(), db.as<float>(), indices ? di.as<int32_t>() : nullptr, dout.as<float>(),
                  dst.as<int32_t>()));
    MICV_HIP(hipMemcpyAsync(out, dout.p, (size_t)T * per * 4, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_calib_svd_host(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices, int stride,
                        int k, int T, uint32_t flags, float *M) {
    HOST_PROLOGUE("micv_calib_svd_host");
    MICV_REQUIRE(pts2d && pts3d && M, "micv_calib_svd_host: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && n >= 1 && n <= 1 << 24 && k >= 1 && k <= 1024 && k <= n && T >= 1 &&
                     (indices ? stride >= k : T == 1),
                 "micv_calib_svd_host: bad flags %u, n %d, k %d, T %d or stride %d", flags, n, k, T, stride);
    return geom_solve_host(ctx, s, "micv_calib_svd_host", pts2d, (size_t)n * 8, pts3d, (size_t)n * 12, n, indices, stride,
                           k, T, 12, M, [&](float *a, float *b, int32_t *i, float *o, int32_t *st) {
                               return micv_calib_svd_dev(ctx, a, b, n, i, stride, k, T, flags, o, st, s);
                           });
}

int micv_fundamental_ls_host(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, const int32_t *indices,
                             int stride, int k, int T, uint32_t flags, float *F) {
    HOST_PROLOGUE("micv_fundamental_ls_host");
    MICV_REQUIRE(ptsA && ptsB && F, "micv_fundamental_ls_host: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && n >= 1 && n <= 1 << 24 && k >= 0 && k <= n && T >= 1 &&
                     (indices ? stride >= k : T == 1),
                 "micv_fundamental_ls_host: bad flags %u, n %d, k %d, T %d or stride %d", flags, n, k, T, stride);
    return geom_solve_host(ctx, s, "micv_fundamental_ls_host", ptsA, (size_t)n * 8, ptsB, (size_t)n * 8, n, indices,
                           stride, k, T, 9, F, [&](float *a, float *b, int32_t *i, float *o, int32_t *st) {
                               return micv_fundamental_ls_dev(ctx, a, b, n, i, stride, k, T, flags, o, st, s);
                           });
}

int micv_fundamental_rank_reduce_host(micv_ctx *ctx, const float *F, int T, uint32_t flags, float *out) {
    HOST_PROLOGUE("micv_fundamental_rank_reduce_host");
    MICV_REQUIRE(F && out && T >= 1 && !(flags & ~MICV_GEOM_F64), "micv_fundamental_rank_reduce_host: bad argument");
    DevBuf di((size_t)T * 36), dout((size_t)T * 36);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dout);
    MICV_HIP(hipMemcpyAsync(di.p, F, (size_t)T * 36, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_fundamental_rank_reduce_dev(ctx, di.as<float>(), T, flags, dout.as<float>(), s));
    MICV_HIP(hipMemcpyAsync(out, dout.p, (size_t)T * 36, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_fundamental_normalized_host(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, uint32_t flags,
                                     float *Ta, float *Tb, float *Fhat, float *F) {
    HOST_PROLOGUE("micv_fundamental_normalized_host");
    MICV_REQUIRE(ptsA && ptsB && Ta && Tb && Fhat && F && n >= 1 && n <= 1 << 24 && !(flags & ~MICV_GEOM_F64),
                 "micv_fundamental_normalized_host: bad argument");
    DevBuf da((size_t)n * 8), db((size_t)n * 8), dout(4 * 36);
    MICV_ALLOC_OK(da); MICV_ALLOC_OK(db); MICV_ALLOC_OK(dout);
    MICV_HIP(hipMemcpyAsync(da.p, ptsA, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(db.p, ptsB, (size_t)n * 8, hipMemcpyHostToDevice, s));
    float *o = dout.as<float>();
    MICV_TRY(micv_fundamental_normalized_dev(ctx, da.as<float>(), db.as<float>(), n, flags, o, o + 9, o + 18, o + 27, s));
    MICV_HIP(hipMemcpyAsync(Ta, o, 36, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(Tb, o + 9, 36, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(Fhat, o + 18, 36, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(F, o + 27, 36, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_epipolar_endpoints_host(micv_ctx *ctx, const float *F, const float *pts, int n, int side, int rows, int cols,
                                 uint32_t flags, float *out) {
    HOST_PROLOGUE("micv_epipolar_endpoints_host");
    MICV_REQUIRE(F && pts && out && n >= 1 && n <= 1 << 28 && (side == 0 || side == 1) && rows >= 1 && cols >= 1 &&
                     !(flags & ~MICV_GEOM_F64),
                 "micv_epipolar_endpoints_host: bad argument");
    DevBuf dF(36), dp((size_t)n * 8), dout((size_t)n * 24);
    MICV_ALLOC_OK(dF); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dout);
    MICV_HIP(hipMemcpyAsync(dF.p, F, 36, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dp.p, pts, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_epipolar_endpoints_dev(ctx, dF.as<float>(), dp.as<float>(), n, side, rows, cols, flags,
                                         dout.as<float>(), s));
    MICV_HIP(hipMemcpyAsync(out, dout.p, (size_t)n * 24, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_camera_center_host(micv_ctx *ctx, const float *M, int T, uint32_t flags, float *center) {
    HOST_PROLOGUE("micv_camera_center_host");
    MICV_REQUIRE(M && center && T >= 1 && !(flags & ~MICV_GEOM_F64), "micv_camera_center_host: bad argument");
    DevBuf dM((size_t)T * 48), dout((size_t)T * 12);
    MICV_ALLOC_OK(dM); MICV_ALLOC_OK(dout);
    MICV_HIP(hipMemcpyAsync(dM.p, M, (size_t)T * 48, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_camera_center_dev(ctx, dM.as<float>(), T, flags, dout.as<float>(), s));
    MICV_HIP(hipMemcpyAsync(center, dout.p, (size_t)T * 12, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

// ps4 registration (warp.hip).  Sizes and strides are checked here as far as the copies need them (an image
// of more than 32767 rows or columns is refused before anything is allocated); the `_dev` call checks the rest.
static bool warp_image_ok(int depth, int rows, int cols, size_t stride) {
    return (depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F) && rows > 0 && cols > 0 && rows <= 32767 &&
           cols <= 32767 && stride_ok(stride, cols, depth == MICV_DEPTH_8U ? 1 : 4);
}

int micv_invert_affine_host(micv_ctx *ctx, const float *m, int count, float *inv) {
    HOST_PROLOGUE("micv_invert_affine_host");
    MICV_REQUIRE(m && inv && count >= 0, "micv_invert_affine_host: bad argument");
    if (count == 0) return MICV_OK;
    DevBuf dm((size_t)count * 24), di((size_t)count * 24);
    MICV_ALLOC_OK(dm); MICV_ALLOC_OK(di);
    MICV_HIP(hipMemcpyAsync(dm.p, m, (size_t)count * 24, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_invert_affine_dev(ctx, dm.as<float>(), count, di.as<float>(), s));
    MICV_HIP(hipMemcpyAsync(inv, di.p, (size_t)count * 24, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_warp_affine_host(micv_ctx *ctx, const void *src, int depth, int srows, int scols, size_t sstride, const float *m,
                          int flags, void *dst, int drows, int dcols, size_t dstride) {
    HOST_PROLOGUE("micv_warp_affine_host");
    MICV_REQUIRE(src && m && dst, "micv_warp_affine_host: null argument");
    MICV_REQUIRE(warp_image_ok(depth, srows, scols, sstride) && warp_image_ok(depth, drows, dcols, dstride),
                 "micv_warp_affine_host: bad depth %d, size %dx%d -> %dx%d (1..32767) or stride", depth, srows, scols, drows,
                 dcols);
    MICV_REQUIRE(src != dst, "micv_warp_affine_host: src and dst must not alias");
    const size_t e = depth == MICV_DEPTH_8U ? 1 : 4, srb = (size_t)scols * e, drb = (size_t)dcols * e;
    DevBuf ds(srb * srows), dd(drb * drows), dm(24);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dd); MICV_ALLOC_OK(dm);
    MICV_TRY(up2d(ds.p, src, sstride, srb, srows, s));
    MICV_HIP(hipMemcpyAsync(dm.p, m, 24, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_warp_affine_dev(ctx, ds.p, depth, srows, scols, srb, dm.as<float>(), flags, dd.p, drows, dcols, drb, s));
    MICV_TRY(down2d(dst, dstride, dd.p, drb, drows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_add_weighted_host(micv_ctx *ctx, const void *a, size_t astride, double alpha, const void *b, size_t bstride,
                           double beta, double gamma, int depth, int rows, int cols, void *dst, size_t dstride) {
    HOST_PROLOGUE("micv_add_weighted_host");
    MICV_REQUIRE(a && b && dst, "micv_add_weighted_host: null argument");
    MICV_REQUIRE(warp_image_ok(depth, rows, cols, astride) && warp_image_ok(depth, rows, cols, bstride) &&
                     warp_image_ok(depth, rows, cols, dstride),
                 "micv_add_weighted_host: bad depth %d, size %dx%d (1..32767) or stride", depth, rows, cols);
    const size_t rb = (size_t)cols * (depth == MICV_DEPTH_8U ? 1 : 4), n = rb * rows;
    DevBuf da(n), db(n), dd(n);
    MICV_ALLOC_OK(da); MICV_ALLOC_OK(db); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(da.p, a, astride, rb, rows, s));
    MICV_TRY(up2d(db.p, b, bstride, rb, rows, s));
    MICV_TRY(micv_add_weighted_dev(ctx, da.p, rb, alpha, db.p, rb, beta, gamma, depth, rows, cols, dd.p, rb, s));
    MICV_TRY(down2d(dst, dstride, dd.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_register_blend_host(micv_ctx *ctx, const void *a, size_t astride, const void *b, size_t bstride, int depth, int rows,
                             int cols, const float *m_a_to_b, void *warped, size_t wstride, void *blended, size_t ostride) {
    HOST_PROLOGUE("micv_register_blend_host");
    MICV_REQUIRE(a && b && m_a_to_b && blended, "micv_register_blend_host: null argument");
    MICV_REQUIRE(warp_image_ok(depth, rows, cols, astride) && warp_image_ok(depth, rows, cols, bstride) &&
                     warp_image_ok(depth, rows, cols, ostride) && (!warped || warp_image_ok(depth, rows, cols, wstride)),
                 "micv_register_blend_host: bad depth %d, size %dx%d (1..32767) or stride", depth, rows, cols);
    const size_t rb = (size_t)cols * (depth == MICV_DEPTH_8U ? 1 : 4), n = rb * rows;
    DevBuf da(n), db(n), dw(warped ? n : 16), dd(n), dm(24);
    MICV_ALLOC_OK(da); MICV_ALLOC_OK(db); MICV_ALLOC_OK(dw); MICV_ALLOC_OK(dd); MICV_ALLOC_OK(dm);
    MICV_TRY(up2d(da.p, a, astride, rb, rows, s));
    MICV_TRY(up2d(db.p, b, bstride, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(dm.p, m_a_to_b, 24, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_register_blend_dev(ctx, da.p, rb, db.p, rb, depth, rows, cols, dm.as<float>(), warped ? dw.p : nullptr, rb,
                                     dd.p, rb, s));
    if (warped) MICV_TRY(down2d(warped, wstride, dw.p, rb, rows, s));
    MICV_TRY(down2d(blended, ostride, dd.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
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
    HOST_PROLOGUE("micv_normalize_minmax_host");
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
    DevBuf ds(sp * nb), du(dst_u8 ? gp * nb : 16), di(dst_inverted ? gp * nb : 16), dj(dst_jet ? jp * nb : 16), dm(8 * nb);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(du); MICV_ALLOC_OK(di); MICV_ALLOC_OK(dj); MICV_ALLOC_OK(dm);
    for (size_t i = 0; i < nb; i++)
        MICV_TRY(up2d(ds.as<char>() + i * sp, static_cast<const char *>(src) + i * src_pitch, sstride, srb, rows, s));
    MICV_TRY(micv_normalize_minmax_batch_dev(ctx, ds.p, sp, depth, batch, rows, cols, srb, dst_u8 ? du.as<uint8_t>() : nullptr, gp,
                                             (size_t)cols, dst_inverted ? di.as<uint8_t>() : nullptr, gp, (size_t)cols,
                                             dst_jet ? dj.as<uint8_t>() : nullptr, jp, 3 * (size_t)cols, dm.as<float>(), s));
    for (size_t i = 0; i < nb; i++) {
        if (dst_u8) MICV_TRY(down2d(dst_u8 + i * u8_pitch, u8_stride, du.as<char>() + i * gp, (size_t)cols, rows, s));
        if (dst_inverted) MICV_TRY(down2d(dst_inverted + i * inverted_pitch, inverted_stride, di.as<char>() + i * gp, (size_t)cols, rows, s));
        if (dst_jet) MICV_TRY(down2d(dst_jet + i * jet_pitch, jet_stride, dj.as<char>() + i * jp, 3 * (size_t)cols, rows, s));
    }
    if (minmax_out) MICV_HIP(hipMemcpyAsync(minmax_out, dm.p, 8 * nb, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_normalize_minmax_host(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride,
                               uint8_t *dst_u8, size_t u8_stride, uint8_t *dst_inverted, size_t inverted_stride,
                               uint8_t *dst_jet, size_t jet_stride, float *minmax_out) {
    return micv_normalize_minmax_batch_host(ctx, src, 0, depth, 1, rows, cols, sstride, dst_u8, 0, u8_stride, dst_inverted, 0,
                                            inverted_stride, dst_jet, 0, jet_stride, minmax_out);
}

int micv_apply_colormap_jet_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, uint8_t *dst_jet,
                                 size_t jet_stride) {
    HOST_PROLOGUE("micv_apply_colormap_jet_host");
    MICV_REQUIRE(src && dst_jet && display_src_ok(MICV_DEPTH_8U, rows, cols, sstride) && jet_stride >= 3 * (size_t)cols,
                 "micv_apply_colormap_jet_host: bad argument, size %dx%d (rows * cols < 2^31) or stride", rows, cols);
    const size_t n = (size_t)rows * cols;
    DevBuf ds(n), dj(3 * n);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dj);
    MICV_TRY(up2d(ds.p, src, sstride, (size_t)cols, rows, s));
    MICV_TRY(micv_apply_colormap_jet_dev(ctx, ds.as<uint8_t>(), rows, cols, (size_t)cols, dj.as<uint8_t>(), 3 * (size_t)cols, s));
    MICV_TRY(down2d(dst_jet, jet_stride, dj.p, 3 * (size_t)cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_gain_noise_f32_host(micv_ctx *ctx, const float *src, size_t sstride, float gain, const float *noise, size_t nstride,
                             int rows, int cols, float *dst, size_t dstride) {
    HOST_PROLOGUE("micv_gain_noise_f32_host");
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0 && stride_ok(sstride, cols, 4) && stride_ok(dstride, cols, 4) &&
                     (!noise || stride_ok(nstride, cols, 4)),
                 "micv_gain_noise_f32_host: bad argument, size %dx%d or stride", rows, cols);
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf ds(n), dn(noise ? n : 16);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dn);
    MICV_TRY(up2d(ds.p, src, sstride, rb, rows, s));
    if (noise) MICV_TRY(up2d(dn.p, noise, nstride, rb, rows, s));
    MICV_TRY(micv_gain_noise_f32_dev(ctx, ds.as<float>(), rb, gain, noise ? dn.as<float>() : nullptr, rb, rows, cols, ds.as<float>(),
                                     rb, s));
    MICV_TRY(down2d(dst, dstride, ds.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

// One body for the pair with and without its display images (img_left == nullptr: the maps alone).
static int pair_host(const char *fn, micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                     float gain, const float *noise_left, const float *noise_right, size_t nstride, int rad, int range,
                     int metric, int flags, int8_t *disp_left, int8_t *disp_right, size_t dstride, bool display,
                     uint8_t *img_left, uint8_t *img_left_inv, uint8_t *img_right, size_t istride) {
    HOST_PROLOGUE("micv_disparity_pair_host");
    MICV_REQUIRE(left && right && disp_left && disp_right && (!display || (img_left && img_right)), "%s: null argument", fn);
    MICV_REQUIRE(rows > 0 && cols > 0 && (int64_t)rows * cols < ((int64_t)1 << 31) && stride_ok(stride, cols, 4) &&
                     dstride >= (size_t)cols && (!display || istride >= (size_t)cols),
                 "%s: bad size %dx%d (rows * cols < 2^31) or stride", fn, rows, cols);
    MICV_REQUIRE(!noise_left == !noise_right && (!noise_left || stride_ok(nstride, cols, 4)),
                 "%s: one noise image without the other, or a bad noise stride", fn);
    const size_t rb = (size_t)cols * 4, n = rb * rows, g = pitch256((size_t)cols * rows);
    const bool change = noise_left || gain != 1.f;
    DevBuf dl(n), dr(n), dnl(noise_left ? n : 16), dnr(noise_left ? n : 16), dw(change ? 2 * n : 16), dd(2 * g), di(display ? 3 * g : 16);
    MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dr); MICV_ALLOC_OK(dnl); MICV_ALLOC_OK(dnr); MICV_ALLOC_OK(dw); MICV_ALLOC_OK(dd); MICV_ALLOC_OK(di);
    MICV_TRY(up2d(dl.p, left, stride, rb, rows, s));
    MICV_TRY(up2d(dr.p, right, stride, rb, rows, s));
    if (noise_left) {
        MICV_TRY(up2d(dnl.p, noise_left, nstride, rb, rows, s));
        MICV_TRY(up2d(dnr.p, noise_right, nstride, rb, rows, s));
    }
    int8_t *d0 = dd.as<int8_t>(), *d1 = d0 + g;
    uint8_t *i0 = di.as<uint8_t>(), *i1 = i0 + g, *i2 = i1 + g;
    if (display)
        MICV_TRY(micv_disparity_pair_display_dev(ctx, dl.as<float>(), dr.as<float>(), rows, cols, rb, gain,
                                                 noise_left ? dnl.as<float>() : nullptr, noise_left ? dnr.as<float>() : nullptr, rb,
                                                 rad, range, metric, flags, d0, d1, (size_t)cols, i0, img_left_inv ? i1 : nullptr, i2,
                                                 (size_t)cols, change ? dw.as<float>() : nullptr, s));
    else
        MICV_TRY(micv_disparity_pair_dev(ctx, dl.as<float>(), dr.as<float>(), rows, cols, rb, rad, range, metric, flags, d0, d1,
                                         (size_t)cols, s));
    MICV_TRY(down2d(disp_left, dstride, d0, (size_t)cols, rows, s));
    MICV_TRY(down2d(disp_right, dstride, d1, (size_t)cols, rows, s));
    if (display) {
        MICV_TRY(down2d(img_left, istride, i0, (size_t)cols, rows, s));
        if (img_left_inv) MICV_TRY(down2d(img_left_inv, istride, i1, (size_t)cols, rows, s));
        MICV_TRY(down2d(img_right, istride, i2, (size_t)cols, rows, s));
    }
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
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
    HOST_PROLOGUE("micv_hough_circles_range_peaks_host");
    MICV_REQUIRE(mask && rows > 0 && cols > 0 && rows <= 32767 && cols <= 32767 && mstride >= (size_t)cols && num_peaks <= 4096,
                 "micv_hough_circles_range_peaks_host: bad argument");
    if (min_radius > max_radius) return MICV_OK;
    MICV_REQUIRE(counts && (peaks_rc || num_peaks == 0), "micv_hough_circles_range_peaks_host: null output");
    const size_t n_radii = (size_t)max_radius - min_radius + 1, cells = (size_t)rows * cols;
    const size_t pbytes = n_radii * num_peaks * 8, abytes = acc ? n_radii * cells * 4 : 0;
    DevBuf dm(cells), dp(pbytes + 8), dn(n_radii * 8), da(abytes + 8);
    MICV_ALLOC_OK(dm); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn); MICV_ALLOC_OK(da);
    MICV_TRY(up2d(dm.p, mask, mstride, (size_t)cols, rows, s));
    if (pbytes) MICV_HIP(hipMemsetAsync(dp.p, 0, pbytes, s));  // rows past a count are unspecified; the host copy gets zeros
    MICV_TIMED("houghCirclesAccumulateKernel",
               micv_hough_circles_range_peaks_dev(ctx, dm.as<uint8_t>(), rows, cols, cols, min_radius, max_radius, num_peaks,
                                                  threshold, dp.as<uint32_t>(), dn.as<int64_t>(), acc ? da.as<int32_t>() : nullptr, s));
    MICV_HIP(hipMemcpyAsync(counts, dn.p, n_radii * 8, hipMemcpyDeviceToHost, s));
    if (pbytes) MICV_HIP(hipMemcpyAsync(peaks_rc, dp.p, pbytes, hipMemcpyDeviceToHost, s));
    if (abytes) MICV_HIP(hipMemcpyAsync(acc, da.p, abytes, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

// one image in, one image out: upload, `call` on the device blocks (dense pitches), download
#define PS1_IMAGE_HOST(fn, src, sstride, src_row_bytes, dst, dstride, dst_row_bytes, call)                  \
    HOST_PROLOGUE(fn);                                                                                      \
    MICV_REQUIRE(src && dst && rows > 0 && cols > 0 && sstride >= (size_t)(src_row_bytes) &&                \
                     dstride >= (size_t)(dst_row_bytes),                                                    \
                 fn ": bad argument");                                                                      \
    DevBuf ds((size_t)rows * (src_row_bytes)), dd((size_t)rows * (dst_row_bytes));                          \
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dd);                                                                   \
    MICV_TRY(up2d(ds.p, src, sstride, (size_t)(src_row_bytes), rows, s));                                   \
    MICV_TRY(call);                                                                                         \
    MICV_TRY(down2d(dst, dstride, dd.p, (size_t)(dst_row_bytes), rows, s));                                 \
    MICV_HIP(hipStreamSynchronize(s));                                                                      \
    return MICV_OK

int micv_gaussian_blur_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int gauss_size,
                               double gauss_sigma, uint8_t *dst, size_t dstride) {
    PS1_IMAGE_HOST("micv_gaussian_blur_u8_host", src, sstride, cols, dst, dstride, cols,
                   micv_gaussian_blur_u8_dev(ctx, ds.as<uint8_t>(), rows, cols, cols, gauss_size, gauss_sigma, dd.as<uint8_t>(), cols, s));
}

int micv_gaussian_blur_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int gauss_size,
                                double gauss_sigma, float *dst, size_t dstride) {
    PS1_IMAGE_HOST("micv_gaussian_blur_f32_host", src, sstride, (size_t)cols * 4, dst, dstride, (size_t)cols * 4,
                   micv_gaussian_blur_f32_dev(ctx, ds.as<float>(), rows, cols, (size_t)cols * 4, gauss_size, gauss_sigma, dd.as<float>(),
                                              (size_t)cols * 4, s));
}

int micv_generate_edge_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t stride, int gauss_size,
                                double gauss_sigma, double low_thresh, double high_thresh, uint8_t *edges,
                                size_t estride) {
    PS1_IMAGE_HOST("micv_generate_edge_f32_host", src, stride, (size_t)cols * 4, edges, estride, cols,
                   micv_generate_edge_f32_dev(ctx, ds.as<float>(), rows, cols, (size_t)cols * 4, gauss_size, gauss_sigma, low_thresh,
                                              high_thresh, dd.as<uint8_t>(), cols, s));
}

int micv_erode_ellipse_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int ksize, float *dst,
                                size_t dstride) {
    PS1_IMAGE_HOST("micv_erode_ellipse_f32_host", src, sstride, (size_t)cols * 4, dst, dstride, (size_t)cols * 4,
                   micv_erode_ellipse_f32_dev(ctx, ds.as<float>(), rows, cols, (size_t)cols * 4, ksize, dd.as<float>(), (size_t)cols * 4, s));
}

int micv_erode_ellipse_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int ksize,
                               uint8_t *dst, size_t dstride) {
    PS1_IMAGE_HOST("micv_erode_ellipse_u8_host", src, sstride, cols, dst, dstride, cols,
                   micv_erode_ellipse_u8_dev(ctx, ds.as<uint8_t>(), rows, cols, cols, ksize, dd.as<uint8_t>(), cols, s));
}

int micv_gray_to_rgb8_host(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride, uint8_t *dst,
                           size_t dstride) {
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_gray_to_rgb8_host: depth %d not supported (8U, 32F)", depth);
    const size_t es = depth == MICV_DEPTH_8U ? 1 : 4;
    PS1_IMAGE_HOST("micv_gray_to_rgb8_host", src, sstride, (size_t)cols * es, dst, dstride, (size_t)cols * 3,
                   micv_gray_to_rgb8_dev(ctx, ds.p, depth, rows, cols, (size_t)cols * es, dd.as<uint8_t>(), (size_t)cols * 3, s));
}

int micv_parallel_lines_host(micv_ctx *ctx, const uint32_t *peaks_rc, int64_t count, unsigned delta_rho,
                             unsigned delta_theta, uint32_t *out_rc, int64_t *out_count) {
    HOST_PROLOGUE("micv_parallel_lines_host");
    MICV_REQUIRE(out_count && count >= 0 && count <= 4096 && ((peaks_rc && out_rc) || count == 0),
                 "micv_parallel_lines_host: bad argument (<= 4096 peaks)");
    MICV_REQUIRE(delta_rho > 0 && delta_theta > 0, "micv_parallel_lines_host: delta_rho and delta_theta must be positive");
    DevBuf dp((size_t)count * 8 + 8), dout((size_t)count * 8 + 8), dn(16);
    MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dout); MICV_ALLOC_OK(dn);
    if (count) MICV_HIP(hipMemcpyAsync(dp.p, peaks_rc, (size_t)count * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dn.p, &count, 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_parallel_lines_dev(ctx, dp.as<uint32_t>(), dn.as<int64_t>(), (unsigned)count, delta_rho, delta_theta,
                                     dout.as<uint32_t>(), dn.as<int64_t>() + 1, s));
    MICV_HIP(hipMemcpyAsync(out_count, dn.as<int64_t>() + 1, 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    if (*out_count > 0) MICV_HIP(hipMemcpy(out_rc, dout.p, (size_t)*out_count * 8, hipMemcpyDeviceToHost));
    return MICV_OK;
}

int micv_draw_lines_parametric_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride,
                                    const uint32_t *peaks_rc, int64_t count, unsigned rho_bin, unsigned theta_bin,
                                    const uint8_t *color) {
    HOST_PROLOGUE("micv_draw_lines_parametric_host");
    MICV_REQUIRE(img && color && rows > 0 && cols > 0 && stride >= (size_t)cols * 3 && count >= 0 && count <= 4096 &&
                     (peaks_rc || count == 0),
                 "micv_draw_lines_parametric_host: bad argument (<= 4096 peaks)");
    const size_t rb = (size_t)cols * 3;
    DevBuf di((size_t)rows * rb), dp((size_t)count * 8 + 8), dn(8);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn);
    MICV_TRY(up2d(di.p, img, stride, rb, rows, s));
    if (count) MICV_HIP(hipMemcpyAsync(dp.p, peaks_rc, (size_t)count * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dn.p, &count, 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_draw_lines_parametric_dev(ctx, di.as<uint8_t>(), rows, cols, rb, dp.as<uint32_t>(), dn.as<int64_t>(), (unsigned)count,
                                            rho_bin, theta_bin, color, s));
    MICV_TRY(down2d(img, stride, di.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_draw_circles_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride, const uint32_t *peaks_rc,
                           const int64_t *counts, unsigned n_radii, unsigned num_peaks, unsigned min_radius,
                           const uint8_t *color) {
    HOST_PROLOGUE("micv_draw_circles_host");
    MICV_REQUIRE(img && color && rows > 0 && cols > 0 && stride >= (size_t)cols * 3 && num_peaks <= 4096 &&
                     (unsigned long long)n_radii * num_peaks < (1ull << 31),
                 "micv_draw_circles_host: bad argument");
    const size_t total = (size_t)n_radii * num_peaks;
    if (total == 0) return MICV_OK;
    MICV_REQUIRE(peaks_rc && counts, "micv_draw_circles_host: null argument");
    const size_t rb = (size_t)cols * 3;
    DevBuf di((size_t)rows * rb), dp(total * 8), dn((size_t)n_radii * 8);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn);
    MICV_TRY(up2d(di.p, img, stride, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(dp.p, peaks_rc, total * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dn.p, counts, (size_t)n_radii * 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_draw_circles_dev(ctx, di.as<uint8_t>(), rows, cols, rb, dp.as<uint32_t>(), dn.as<int64_t>(), n_radii, num_peaks,
                                   min_radius, color, s));
    MICV_TRY(down2d(img, stride, di.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

// ---- ps5 driver (ps5.hip) ----------------------------------------------------------------------

int micv_draw_velocity_vectors_host(micv_ctx *ctx, uint8_t *img, size_t img_pitch, size_t stride, const float *u, const float *v,
                                    size_t field_pitch, size_t fstride, int batch, int rows, int cols, const uint8_t *color) {
    HOST_PROLOGUE("micv_draw_velocity_vectors_host");
    MICV_REQUIRE(img && u && v && color && rows > 0 && cols > 0 && batch >= 0 && stride >= (size_t)cols * 3 && stride_ok(fstride, cols, 4),
                 "micv_draw_velocity_vectors_host: bad argument, size %dx%d or stride", rows, cols);
    MICV_REQUIRE(batch <= 1 || (img_pitch >= (size_t)(rows - 1) * stride + (size_t)cols * 3 &&
                                field_pitch >= (size_t)(rows - 1) * fstride + (size_t)cols * 4),
                 "micv_draw_velocity_vectors_host: a pitch is smaller than an image or a field");
    if (batch == 0) return MICV_OK;
    const size_t irb = (size_t)cols * 3, frb = (size_t)cols * 4, ip = pitch256(irb * rows), fp = pitch256(frb * rows), nb = (size_t)batch;
    DevBuf di(ip * nb), du(fp * nb), dv(fp * nb);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(du); MICV_ALLOC_OK(dv);
    for (size_t i = 0; i < nb; i++) {
        MICV_TRY(up2d(di.as<char>() + i * ip, img + i * img_pitch, stride, irb, rows, s));
        MICV_TRY(up2d(du.as<char>() + i * fp, reinterpret_cast<const char *>(u) + i * field_pitch, fstride, frb, rows, s));
        MICV_TRY(up2d(dv.as<char>() + i * fp, reinterpret_cast<const char *>(v) + i * field_pitch, fstride, frb, rows, s));
    }
    MICV_TRY(micv_draw_velocity_vectors_dev(ctx, di.as<uint8_t>(), ip, irb, du.as<float>(), dv.as<float>(), fp, frb, batch, rows, cols,
                                            color, s));
    for (size_t i = 0; i < nb; i++) MICV_TRY(down2d(img + i * img_pitch, stride, di.as<char>() + i * ip, irb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_gray_or_bgr_to_bgr8_host(micv_ctx *ctx, const void *src, int depth, int channels, int rows, int cols, size_t sstride,
                                  uint8_t *dst, size_t dstride) {
    MICV_REQUIRE(depth == MICV_DEPTH_8U && (channels == 1 || channels == 3),
                 "micv_gray_or_bgr_to_bgr8_host: depth %d / %d channels not supported (8U, 1 or 3 channels)", depth, channels);
    PS1_IMAGE_HOST("micv_gray_or_bgr_to_bgr8_host", src, sstride, (size_t)cols * channels, dst, dstride, (size_t)cols * 3,
                   micv_gray_or_bgr_to_bgr8_dev(ctx, ds.p, depth, channels, rows, cols, (size_t)cols * channels, dd.as<uint8_t>(),
                                                (size_t)cols * 3, s));
}

int micv_pyramid_montage_host(micv_ctx *ctx, const void *const *levels, const int *level_rows, const int *level_cols,
                              const size_t *level_strides, int depth, uint8_t *dst, size_t dstride) {
    HOST_PROLOGUE("micv_pyramid_montage_host");
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
    DevBuf dl(off[4]), dd((size_t)4 * R * C);
    MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dd);
    const void *dev_levels[4];
    for (int l = 0; l < 4; l++) {
        MICV_TRY(up2d(dl.as<char>() + off[l], levels[l], level_strides[l], rb[l], level_rows[l], s));
        dev_levels[l] = dl.as<char>() + off[l];
    }
    MICV_TRY(micv_pyramid_montage_dev(ctx, dev_levels, level_rows, level_cols, rb, depth, dd.as<uint8_t>(), (size_t)2 * C, s));
    MICV_TRY(down2d(dst, dstride, dd.p, (size_t)2 * C, 2 * R, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_lk_warp_diff_host(micv_ctx *ctx, const float *prev, size_t pstride, const float *next, size_t nstride, const float *du,
                           const float *dv, size_t fstride, int rows, int cols, float *diff, size_t dstride) {
    HOST_PROLOGUE("micv_lk_warp_diff_host");
    MICV_REQUIRE(prev && next && du && dv && diff && rows > 0 && cols > 0, "micv_lk_warp_diff_host: bad argument");
    MICV_REQUIRE(stride_ok(pstride, cols, 4) && stride_ok(nstride, cols, 4) && stride_ok(fstride, cols, 4) && stride_ok(dstride, cols, 4),
                 "micv_lk_warp_diff_host: bad stride");
    const size_t rb = (size_t)cols * 4, n = rb * rows;
    DevBuf dp(n), dn(n), dU(n), dV(n), dd(n);
    MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn); MICV_ALLOC_OK(dU); MICV_ALLOC_OK(dV); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(dp.p, prev, pstride, rb, rows, s));
    MICV_TRY(up2d(dn.p, next, nstride, rb, rows, s));
    MICV_TRY(up2d(dU.p, du, fstride, rb, rows, s));
    MICV_TRY(up2d(dV.p, dv, fstride, rb, rows, s));
    MICV_TRY(micv_lk_warp_diff_dev(ctx, dp.as<float>(), rb, dn.as<float>(), rb, dU.as<float>(), dV.as<float>(), rb, rows, cols,
                                   dd.as<float>(), rb, s));
    MICV_TRY(down2d(diff, dstride, dd.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_ps5_warp_diff_seq_host(micv_ctx *ctx, const void *const *frames, int nframes, int rows, int cols, size_t stride,
                                int channels, int depth, int levels, int level, int win, uint8_t *diff_u8, float *diff_f32,
                                float *u, float *v) {
    HOST_PROLOGUE("micv_ps5_warp_diff_seq_host");
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
    DevBuf raw(srb * rows), grey(n0 * 4 * nf), pyr(lvl_off[levels] ? lvl_off[levels] : 16), d8(ln * np), df(diff_f32 ? ln * 4 * np : 16),
        dU(u ? ln * 4 * np : 16), dV(u ? ln * 4 * np : 16);
    MICV_ALLOC_OK(raw); MICV_ALLOC_OK(grey); MICV_ALLOC_OK(pyr); MICV_ALLOC_OK(d8); MICV_ALLOC_OK(df); MICV_ALLOC_OK(dU); MICV_ALLOC_OK(dV);
    for (size_t t = 0; t < nf; t++) {  // (one raw block: the copy of frame t + 1 queues behind the conversion of frame t)
        MICV_TRY(up2d(raw.p, frames[t], stride, srb, rows, s));
        MICV_TRY(micv_to_gray_f32_dev(ctx, raw.p, rows, cols, srb, channels, depth, grey.as<float>() + t * n0, rb, s));
    }
    const float *lvl_frames = grey.as<float>();
    if (level > 0) {
        float *dst_levels[16];
        for (int l = 0; l < levels; l++) dst_levels[l] = l == 0 ? nullptr : reinterpret_cast<float *>(pyr.as<char>() + lvl_off[l]);
        MICV_TRY(micv_gaussian_pyramid_batch_dev(ctx, grey.as<float>(), nframes, n0 * 4, rows, cols, rb, levels, dst_levels, nullptr,
                                                 nullptr, s));
        lvl_frames = dst_levels[level];
    }
    MICV_TRY(micv_ps5_warp_diff_seq_dev(ctx, lvl_frames, ln * 4, nframes, lr, lc, (size_t)lc * 4, win, d8.as<uint8_t>(), ln, (size_t)lc,
                                        diff_f32 ? df.as<float>() : nullptr, u ? dU.as<float>() : nullptr, u ? dV.as<float>() : nullptr,
                                        s));
    MICV_HIP(hipMemcpyAsync(diff_u8, d8.p, ln * np, hipMemcpyDeviceToHost, s));
    if (diff_f32) MICV_HIP(hipMemcpyAsync(diff_f32, df.p, ln * 4 * np, hipMemcpyDeviceToHost, s));
    if (u) {
        MICV_HIP(hipMemcpyAsync(u, dU.p, ln * 4 * np, hipMemcpyDeviceToHost, s));
        MICV_HIP(hipMemcpyAsync(v, dV.p, ln * 4 * np, hipMemcpyDeviceToHost, s));
    }
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_dense_lk_display_host(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols, size_t stride, int channels,
                               int depth, int mode, int win, int levels, const uint8_t *color, float *u, float *v, size_t ostride,
                               uint8_t *arrows, size_t astride, uint8_t *jet_u, uint8_t *jet_v, size_t jstride) {
    HOST_PROLOGUE("micv_dense_lk_display_host");
    MICV_REQUIRE(prev && next && color && u && v && arrows && rows > 0 && cols > 0, "micv_dense_lk_display_host: bad argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U && (channels == 1 || channels == 3),
                 "micv_dense_lk_display_host: depth %d / %d channels not supported (8-bit frames of 1 or 3 channels)", depth, channels);
    MICV_REQUIRE((jet_u == nullptr) == (jet_v == nullptr), "micv_dense_lk_display_host: give both colour maps or none");
    const size_t srb = (size_t)cols * channels, rb = (size_t)cols * 4, n = rb * rows, irb = (size_t)cols * 3, in = pitch256(irb * rows);
    MICV_REQUIRE(stride >= srb && stride_ok(ostride, cols, 4) && astride >= irb && (!jet_u || jstride >= irb),
                 "micv_dense_lk_display_host: bad stride");
    const size_t fn = pitch256(n);
    DevBuf dp(srb * rows), dn(srb * rows), duv(2 * fn), da(in), dj(jet_u ? 2 * in : 16);
    MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dn); MICV_ALLOC_OK(duv); MICV_ALLOC_OK(da); MICV_ALLOC_OK(dj);
    MICV_TRY(up2d(dp.p, prev, stride, srb, rows, s));
    MICV_TRY(up2d(dn.p, next, stride, srb, rows, s));
    float *du = duv.as<float>(), *dv = reinterpret_cast<float *>(duv.as<char>() + fn);
    uint8_t *ju = jet_u ? dj.as<uint8_t>() : nullptr, *jv = jet_u ? ju + in : nullptr;
    MICV_TRY(micv_dense_lk_display_dev(ctx, dp.p, dn.p, rows, cols, srb, channels, depth, mode, win, levels, color, du, dv, rb,
                                       da.as<uint8_t>(), irb, ju, jv, irb, s));
    MICV_TRY(down2d(u, ostride, du, rb, rows, s));
    MICV_TRY(down2d(v, ostride, dv, rb, rows, s));
    MICV_TRY(down2d(arrows, astride, da.p, irb, rows, s));
    if (jet_u) {
        MICV_TRY(down2d(jet_u, jstride, ju, irb, rows, s));
        MICV_TRY(down2d(jet_v, jstride, jv, irb, rows, s));
    }
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

// ---- ps4 driver (ps4.hip) ----------------------------------------------------------------------

int micv_draw_dots_host(micv_ctx *ctx, const void *gray, int depth, int rows, int cols, size_t gstride, const float *corners,
                        size_t cstride, uint8_t *dst, size_t dstride) {
    HOST_PROLOGUE("micv_draw_dots_host");
    MICV_REQUIRE(gray && corners && dst && rows > 0 && cols > 0, "micv_draw_dots_host: bad argument");
    MICV_REQUIRE(depth == MICV_DEPTH_8U || depth == MICV_DEPTH_32F, "micv_draw_dots_host: depth %d not supported (8U, 32F)", depth);
    const size_t e = depth == MICV_DEPTH_32F ? 4 : 1, grb = (size_t)cols * e, crb = (size_t)cols * 4, drb = (size_t)cols * 3;
    MICV_REQUIRE(stride_ok(gstride, cols, e) && stride_ok(cstride, cols, 4) && dstride >= drb, "micv_draw_dots_host: bad stride");
    DevBuf dg(grb * rows), dc(crb * rows), dd(drb * rows);
    MICV_ALLOC_OK(dg); MICV_ALLOC_OK(dc); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(dg.p, gray, gstride, grb, rows, s));
    MICV_TRY(up2d(dc.p, corners, cstride, crb, rows, s));
    MICV_TRY(micv_draw_dots_dev(ctx, dg.p, depth, rows, cols, grb, dc.as<float>(), crb, dd.as<uint8_t>(), drb, s));
    MICV_TRY(down2d(dst, dstride, dd.p, drb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_hconcat_host(micv_ctx *ctx, const uint8_t *a, size_t astride, int acols, const uint8_t *b, size_t bstride, int bcols,
                      int rows, int bpp, uint8_t *dst, size_t dstride) {
    HOST_PROLOGUE("micv_hconcat_host");
    MICV_REQUIRE(a && b && dst && rows > 0 && acols > 0 && bcols > 0 && (bpp == 1 || bpp == 3), "micv_hconcat_host: bad argument");
    const size_t arb = (size_t)acols * bpp, brb = (size_t)bcols * bpp;
    MICV_REQUIRE(astride >= arb && bstride >= brb && dstride >= arb + brb, "micv_hconcat_host: a stride is smaller than its row");
    DevBuf da(arb * rows), db(brb * rows), dd((arb + brb) * rows);
    MICV_ALLOC_OK(da); MICV_ALLOC_OK(db); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(da.p, a, astride, arb, rows, s));
    MICV_TRY(up2d(db.p, b, bstride, brb, rows, s));
    MICV_TRY(micv_hconcat_dev(ctx, da.as<uint8_t>(), arb, acols, db.as<uint8_t>(), brb, bcols, rows, bpp, dd.as<uint8_t>(), arb + brb, s));
    MICV_TRY(down2d(dst, dstride, dd.p, arb + brb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_draw_keypoints_host(micv_ctx *ctx, const uint8_t *src, int channels, int rows, int cols, size_t sstride, uint8_t *canvas,
                             int canvas_cols, size_t cstride, int x0, const float *kp_xysa, int64_t n, uint64_t *rng_state) {
    HOST_PROLOGUE("micv_draw_keypoints_host");
    MICV_REQUIRE(canvas && rng_state && rows > 0 && cols > 0 && n >= 0 && (n == 0 || kp_xysa), "micv_draw_keypoints_host: bad argument");
    MICV_REQUIRE(!src || channels == 1 || channels == 3, "micv_draw_keypoints_host: %d channels not supported (1 or 3)", channels);
    MICV_REQUIRE(x0 >= 0 && (int64_t)x0 + cols <= canvas_cols && cstride >= (size_t)canvas_cols * 3 &&
                     (!src || sstride >= (size_t)cols * channels),
                 "micv_draw_keypoints_host: the window does not lie in the canvas, or bad stride");
    // the window alone travels: it is a canvas of its own on the device
    const size_t srb = src ? (size_t)cols * channels : 16, prb = (size_t)cols * 3;
    DevBuf ds(srb * rows), dp(prb * rows), dk(n ? (size_t)n * 16 : 16), dw(16);
    MICV_ALLOC_OK(ds); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dk); MICV_ALLOC_OK(dw);
    uint8_t *window = canvas + 3 * (size_t)x0;
    if (src)
        MICV_TRY(up2d(ds.p, src, sstride, srb, rows, s));
    else
        MICV_TRY(up2d(dp.p, window, cstride, prb, rows, s));
    if (n) MICV_HIP(hipMemcpyAsync(dk.p, kp_xysa, (size_t)n * 16, hipMemcpyHostToDevice, s));
    const int64_t words[2] = {n, (int64_t)*rng_state};
    MICV_HIP(hipMemcpyAsync(dw.p, words, 16, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_draw_keypoints_dev(ctx, src ? ds.as<uint8_t>() : nullptr, channels, rows, cols, srb, dp.as<uint8_t>(), cols, prb, 0,
                                     dk.as<float>(), dw.as<int64_t>(), n, reinterpret_cast<uint64_t *>(dw.as<int64_t>() + 1), s));
    MICV_TRY(down2d(window, cstride, dp.p, prb, rows, s));
    MICV_HIP(hipMemcpyAsync(rng_state, dw.as<int64_t>() + 1, 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_draw_match_lines_host(micv_ctx *ctx, uint8_t *canvas, int rows, int cols, size_t stride, const float *kp_a, int64_t na,
                               const float *kp_b, int64_t nb, const int32_t *matches_qt, int64_t n, const uint8_t *mask,
                               int x_offset, uint64_t seed) {
    HOST_PROLOGUE("micv_draw_match_lines_host");
    MICV_REQUIRE(canvas && rows > 0 && cols > 0 && stride >= (size_t)cols * 3 && na >= 0 && nb >= 0 && n >= 0,
                 "micv_draw_match_lines_host: bad argument");
    if (n == 0 || na == 0 || nb == 0) return MICV_OK;
    MICV_REQUIRE(kp_a && kp_b && matches_qt, "micv_draw_match_lines_host: null argument");
    const size_t rb = (size_t)cols * 3;
    DevBuf dc(rb * rows), da((size_t)na * 16), db((size_t)nb * 16), dm((size_t)n * 8), dk(mask ? (size_t)n : 16), dw(8);
    MICV_ALLOC_OK(dc); MICV_ALLOC_OK(da); MICV_ALLOC_OK(db); MICV_ALLOC_OK(dm); MICV_ALLOC_OK(dk); MICV_ALLOC_OK(dw);
    MICV_TRY(up2d(dc.p, canvas, stride, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(da.p, kp_a, (size_t)na * 16, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(db.p, kp_b, (size_t)nb * 16, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dm.p, matches_qt, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (mask) MICV_HIP(hipMemcpyAsync(dk.p, mask, (size_t)n, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dw.p, &n, 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_draw_match_lines_dev(ctx, dc.as<uint8_t>(), rows, cols, rb, da.as<float>(), na, db.as<float>(), nb, dm.as<int32_t>(),
                                       dw.as<int64_t>(), n, mask ? dk.as<uint8_t>() : nullptr, x_offset, seed, s));
    MICV_TRY(down2d(canvas, stride, dc.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_ps4_harris_display_host(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                                 double sigma, float alpha, int flags, double threshold, int min_distance, float *fields,
                                 int32_t *locs_yx, int64_t cap, int64_t *count, uint8_t *grad_panel, size_t gstride,
                                 uint8_t *resp_u8, size_t rstride, uint8_t *dots, size_t dstride) {
    HOST_PROLOGUE("micv_ps4_harris_display_host");
    MICV_REQUIRE(img && fields && count && grad_panel && resp_u8 && dots && rows > 0 && cols > 0 && cap >= 0 && (cap == 0 || locs_yx),
                 "micv_ps4_harris_display_host: bad argument");
    const size_t n = (size_t)rows * cols, rb = (size_t)cols * 4;
    MICV_REQUIRE(stride_ok(stride, cols, 4) && gstride >= (size_t)2 * cols && rstride >= (size_t)cols && dstride >= (size_t)cols * 3,
                 "micv_ps4_harris_display_host: bad stride");
    DevBuf di(n * 4), df(n * 16), dl(cap ? (size_t)cap * 8 : 16), dn(8), dg(2 * n), dr(n), dd(3 * n);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(df); MICV_ALLOC_OK(dl); MICV_ALLOC_OK(dn); MICV_ALLOC_OK(dg); MICV_ALLOC_OK(dr); MICV_ALLOC_OK(dd);
    MICV_TRY(up2d(di.p, img, stride, rb, rows, s));
    MICV_TRY(micv_ps4_harris_display_dev(ctx, di.as<float>(), rows, cols, rb, sobel_ksize, win, sigma, alpha, flags, threshold,
                                         min_distance, df.as<float>(), dl.as<int32_t>(), cap, dn.as<int64_t>(), dg.as<uint8_t>(),
                                         (size_t)2 * cols, dr.as<uint8_t>(), (size_t)cols, dd.as<uint8_t>(), (size_t)3 * cols, s));
    MICV_HIP(hipMemcpyAsync(fields, df.p, n * 16, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipMemcpyAsync(count, dn.p, 8, hipMemcpyDeviceToHost, s));
    MICV_TRY(down2d(grad_panel, gstride, dg.p, (size_t)2 * cols, rows, s));
    MICV_TRY(down2d(resp_u8, rstride, dr.p, (size_t)cols, rows, s));
    MICV_TRY(down2d(dots, dstride, dd.p, (size_t)3 * cols, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    if (cap) {
        const int64_t got = *count < cap ? *count : cap;
        if (got > 0) MICV_HIP(hipMemcpy(locs_yx, dl.p, (size_t)got * 8, hipMemcpyDeviceToHost));
    }
    return MICV_OK;
}

int micv_ps4_match_panels_host(micv_ctx *ctx, const uint8_t *img_a, size_t astride, int cols_a, const uint8_t *img_b, size_t bstride,
                               int cols_b, int rows, const float *kp_a, int64_t n_a, const float *kp_b, int64_t n_b,
                               const int32_t *matches_qt, int64_t n_matches, const uint8_t *mask, int flags, uint64_t seed,
                               uint64_t *rng_state, uint8_t *keypoint_panel, uint8_t *match_panel, size_t pstride) {
    HOST_PROLOGUE("micv_ps4_match_panels_host");
    MICV_REQUIRE(img_a && img_b && match_panel && rng_state && rows > 0 && cols_a > 0 && cols_b > 0 && n_a >= 0 && n_b >= 0 &&
                     n_matches >= 0 && (n_a == 0 || kp_a) && (n_b == 0 || kp_b) && (n_matches == 0 || matches_qt),
                 "micv_ps4_match_panels_host: bad argument");
    const size_t prb = ((size_t)cols_a + cols_b) * 3;
    MICV_REQUIRE(astride >= (size_t)cols_a && bstride >= (size_t)cols_b && pstride >= prb, "micv_ps4_match_panels_host: bad stride");
    DevBuf da((size_t)cols_a * rows), db((size_t)cols_b * rows), dka(n_a ? (size_t)n_a * 16 : 16), dkb(n_b ? (size_t)n_b * 16 : 16),
        dm(n_matches ? (size_t)n_matches * 8 : 16), dk(mask && n_matches ? (size_t)n_matches : 16), dw(32), dp1(keypoint_panel ? prb * rows : 16),
        dp2(prb * rows);
    MICV_ALLOC_OK(da); MICV_ALLOC_OK(db); MICV_ALLOC_OK(dka); MICV_ALLOC_OK(dkb); MICV_ALLOC_OK(dm); MICV_ALLOC_OK(dk); MICV_ALLOC_OK(dw);
    MICV_ALLOC_OK(dp1); MICV_ALLOC_OK(dp2);
    MICV_TRY(up2d(da.p, img_a, astride, (size_t)cols_a, rows, s));
    MICV_TRY(up2d(db.p, img_b, bstride, (size_t)cols_b, rows, s));
    if (n_a) MICV_HIP(hipMemcpyAsync(dka.p, kp_a, (size_t)n_a * 16, hipMemcpyHostToDevice, s));
    if (n_b) MICV_HIP(hipMemcpyAsync(dkb.p, kp_b, (size_t)n_b * 16, hipMemcpyHostToDevice, s));
    if (n_matches) MICV_HIP(hipMemcpyAsync(dm.p, matches_qt, (size_t)n_matches * 8, hipMemcpyHostToDevice, s));
    if (mask && n_matches) MICV_HIP(hipMemcpyAsync(dk.p, mask, (size_t)n_matches, hipMemcpyHostToDevice, s));
    const int64_t words[4] = {n_a, n_b, n_matches, (int64_t)*rng_state};
    MICV_HIP(hipMemcpyAsync(dw.p, words, 32, hipMemcpyHostToDevice, s));
    int64_t *w = dw.as<int64_t>();
    MICV_TRY(micv_ps4_match_panels_dev(ctx, da.as<uint8_t>(), (size_t)cols_a, cols_a, db.as<uint8_t>(), (size_t)cols_b, cols_b, rows,
                                       dka.as<float>(), w, n_a, dkb.as<float>(), w + 1, n_b, dm.as<int32_t>(), w + 2, n_matches,
                                       mask ? dk.as<uint8_t>() : nullptr, flags, seed, reinterpret_cast<uint64_t *>(w + 3),
                                       keypoint_panel ? dp1.as<uint8_t>() : nullptr, dp2.as<uint8_t>(), prb, s));
    if (keypoint_panel) MICV_TRY(down2d(keypoint_panel, pstride, dp1.p, prb, rows, s));
    MICV_TRY(down2d(match_panel, pstride, dp2.p, prb, rows, s));
    MICV_HIP(hipMemcpyAsync(rng_state, w + 3, 8, hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

// ---- ps6 driver (ps6.hip) ----------------------------------------------------------------------
// The image goes up with its pixels only; the padding of the caller's rows is never read or written.

int micv_draw_particles_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                             const double *color) {
    HOST_PROLOGUE("micv_draw_particles_host");
    MICV_REQUIRE(img && color && rows > 0 && cols > 0 && n >= 0 && (n == 0 || xy), "micv_draw_particles_host: bad argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_draw_particles_host: %d channels not supported (1, 3, 4)", channels);
    const size_t rb = (size_t)cols * channels;
    MICV_REQUIRE(stride >= rb, "micv_draw_particles_host: stride %zu < %zu", stride, rb);
    if (n == 0) return MICV_OK;
    DevBuf di(rb * rows), dp((size_t)n * 8);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dp);
    MICV_TRY(up2d(di.p, img, stride, rb, rows, s));
    MICV_HIP(hipMemcpyAsync(dp.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_draw_particles_dev(ctx, di.as<uint8_t>(), rows, cols, channels, rb, dp.as<float>(), n, color, s));
    MICV_TRY(down2d(img, stride, di.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_draw_rectangle_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, int x, int y, int w, int h,
                             const double *color) {
    HOST_PROLOGUE("micv_draw_rectangle_host");
    MICV_REQUIRE(img && color && rows > 0 && cols > 0, "micv_draw_rectangle_host: bad argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_draw_rectangle_host: %d channels not supported (1, 3, 4)", channels);
    const size_t rb = (size_t)cols * channels;
    MICV_REQUIRE(stride >= rb, "micv_draw_rectangle_host: stride %zu < %zu", stride, rb);
    DevBuf di(rb * rows);
    MICV_ALLOC_OK(di);
    MICV_TRY(up2d(di.p, img, stride, rb, rows, s));
    MICV_TRY(micv_draw_rectangle_dev(ctx, di.as<uint8_t>(), rows, cols, channels, rb, x, y, w, h, color, s));
    MICV_TRY(down2d(img, stride, di.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_ps6_overlay_list_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                               const double *dot_color, const float *centre, float bbox_w, float bbox_h, const double *box_color) {
    HOST_PROLOGUE("micv_ps6_overlay_list_host");
    MICV_REQUIRE(img && dot_color && centre && box_color && rows > 0 && cols > 0 && n >= 0 && (n == 0 || xy),
                 "micv_ps6_overlay_list_host: bad argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_ps6_overlay_list_host: %d channels not supported (1, 3, 4)",
                 channels);
    const size_t rb = (size_t)cols * channels;
    MICV_REQUIRE(stride >= rb, "micv_ps6_overlay_list_host: stride %zu < %zu", stride, rb);
    DevBuf di(rb * rows), dp(n ? (size_t)n * 8 : 16), dc(16);
    MICV_ALLOC_OK(di); MICV_ALLOC_OK(dp); MICV_ALLOC_OK(dc);
    MICV_TRY(up2d(di.p, img, stride, rb, rows, s));
    if (n) MICV_HIP(hipMemcpyAsync(dp.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, s));
    MICV_HIP(hipMemcpyAsync(dc.p, centre, 8, hipMemcpyHostToDevice, s));
    MICV_TRY(micv_ps6_overlay_list_dev(ctx, di.as<uint8_t>(), rows, cols, channels, rb, dp.as<float>(), n, dot_color, dc.as<float>(), bbox_w,
                                       bbox_h, box_color, s));
    MICV_TRY(down2d(img, stride, di.p, rb, rows, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

}  // extern "C"
