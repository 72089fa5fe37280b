// host_io.hpp -- the plumbing of every `_host` entry point: host pointers in, host pointers out, synchronous.
// This is the behaviour of the reference's cv::Mat functions (upload -> kernel -> sync -> download inside every call,
// e.g. Harris.cu:118-158, Pyramids.cu:45-72); it is PCIe-bound by construction.
//
// One HostCall per call.  It selects the context's device, owns the stream of the call (the null stream), every device
// block of the call (from the context's cache: a repeated call of the same shape does no hipMalloc / hipFree) and the
// event pair of the kernel log.  Whichever way the function returns, the destructor
//   1. drains the stream, so that no copy into the caller's memory is in flight and nothing still uses a block,
//   2. hands the timing to the micv_set_kernel_log sink,
//   3. gives the blocks back to the cache
// in that order.  The first failure sticks: a later up() / down() does nothing, and finish() returns its status.
//
//     HostCall h(ctx, "micv_x_host");
//     if (!h.ok()) return h.finish();              // ctx is null, or its device cannot be selected
//     MICV_REQUIRE(...);                           // the function's own argument checks
//     float *ds = h.up<float>(src, sstride, rb, rows), *dd = h.alloc<float>(rb * rows);
//     if (!h.ok()) return h.finish();              // no `_dev` call ever sees a null block
//     MICV_TRY(micv_x_dev(ctx, ds, ..., dd, ..., h.s));
//     h.down(dst, dstride, dd, rb, rows);
//     return h.finish();
#pragma once

#include <atomic>

#include "common.hpp"

namespace micv {

// Kernel-timing log lines: the reference brackets its kernels with a GpuTimer and logs
// "<kernel> execution took {} ms" (Harris.cu:144-155, DisparitySSD.cu:192-203, Hough.cu:277-289, Pyramids.cu:61-69).
// With a sink registered (micv_set_kernel_log, host_api.hip) the `_host` entry point of each of those functions records
// an event pair around its device call (MICV_TIMED) and, after the stream has drained, hands (the reference's kernel
// name, milliseconds) to the sink; without one nothing is recorded.
extern std::atomic<micv_kernel_log_fn> g_log_fn;
extern std::atomic<void *> g_log_user;

class HostCall {
  public:
    static constexpr int kMaxBlocks = 16;  // the largest user holds ten
    const hipStream_t s = nullptr;         // every `_host` call is synchronous, like the reference's

    HostCall(micv_ctx *ctx, const char *fn) : ctx_(ctx), fn_(fn) {
        if (!ctx) {
            set_error("%s: ctx is null", fn);
            status_ = MICV_EINVAL;
            return;
        }
        check(hipSetDevice(ctx->device), "hipSetDevice");
    }
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    ~HostCall() {
        drain();
        if (name_) {
            float ms = 0.f;
            const micv_kernel_log_fn fn = g_log_fn.load(std::memory_order_relaxed);
            if (fn && hipEventElapsedTime(&ms, e0_, e1_) == hipSuccess) fn(name_, ms, g_log_user.load(std::memory_order_relaxed));
        }
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
        for (int i = 0; i < nblocks_; i++) ctx_->io_release(blocks_[i]);
    }

    bool ok() const { return status_ == MICV_OK; }
    // The one synchronisation of the success path; the status of the call.  (A function that reads a count it has
    // downloaded calls it, then down() for the counted part, then finish() again.)
    int finish() {
        drain();
        return status_;
    }

    template <typename T>
    T *alloc(size_t bytes) {
        if (!ok()) return nullptr;
        if (nblocks_ == kMaxBlocks) {
            set_error("%s: more than %d device blocks in one call", fn_, kMaxBlocks);
            status_ = MICV_EINVAL;
            return nullptr;
        }
        void *p = ctx_->io_acquire(bytes);
        if (!p) {
            set_error("device allocation failed");
            status_ = MICV_ENOMEM;
            return nullptr;
        }
        blocks_[nblocks_++] = p;
        drained_ = false;  // whatever uses the block must have finished before it goes back
        return static_cast<T *>(p);
    }
    // A pitched host image into a dense block of its own.
    template <typename T>
    T *up(const void *host, size_t hstride, size_t row_bytes, int rows) {
        T *d = alloc<T>(row_bytes * (size_t)rows);
        up_to(d, host, hstride, row_bytes, rows);
        return d;
    }
    // A flat host array into a block of its own; no copy when there is nothing to copy (the block is still there).
    template <typename T>
    T *up(const void *host, size_t bytes) {
        T *d = alloc<T>(bytes);
        if (host && bytes) up_to(d, host, bytes, bytes, 1);
        return d;
    }
    // The same copies into / out of a part of a block.
    void up_to(void *dev, const void *host, size_t hstride, size_t row_bytes, int rows) {
        if (ok()) check(copy2d(dev, row_bytes, host, hstride, row_bytes, rows, hipMemcpyHostToDevice, s), "the upload");
    }
    void down(void *host, size_t hstride, const void *dev, size_t row_bytes, int rows) {
        if (!ok()) return;
        drained_ = false;
        check(copy2d(host, hstride, dev, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, s), "the download");
    }
    void down(void *host, const void *dev, size_t bytes) { down(host, bytes, dev, bytes, 1); }

    // A continuous cv::Mat (step == row bytes: what cv::Mat::create gives) goes as ONE linear copy; only a pitched view
    // (an ROI) needs the 2-D form.  Pageable host memory is fine: the runtime pins the pages for the transfer and reaches
    // the same 53 GB/s as hipHostMalloc'd memory on this platform (tools/probes/pcie_probe.py), so there is no staging
    // ring to copy through.  (Static: the sequence pipelines issue it on streams of their own.)
    static hipError_t copy2d(void *dst, size_t dstride, const void *src, size_t sstride, size_t row_bytes, int rows,
                             hipMemcpyKind kind, hipStream_t stream) {
        if ((dstride == row_bytes && sstride == row_bytes) || rows == 1)
            return hipMemcpyAsync(dst, src, row_bytes * (size_t)rows, kind, stream);
        return hipMemcpy2DAsync(dst, dstride, src, sstride, row_bytes, rows, kind, stream);
    }

    // Any other HIP call of a `_host` body (a memset): a failure sticks like a failed copy.
    void check(hipError_t e, const char *what) {
        if (e == hipSuccess || !ok()) return;
        set_error("%s: %s failed: %s", fn_, what, hipGetErrorString(e));
        status_ = e == hipErrorOutOfMemory ? MICV_ENOMEM : MICV_EHIP;
    }

    // The bracket of MICV_TIMED (a no-op without a sink).
    void begin(const char *kernel) {
        if (!g_log_fn.load(std::memory_order_relaxed)) return;
        if (hipEventCreate(&e0_) != hipSuccess || hipEventCreate(&e1_) != hipSuccess) return;
        name_ = kernel;
        (void)hipEventRecord(e0_, s);
    }
    void end() {
        if (name_) (void)hipEventRecord(e1_, s);
    }

  private:
    void drain() {
        if (drained_) return;
        drained_ = true;
        check(hipStreamSynchronize(s), "hipStreamSynchronize");
    }

    micv_ctx *ctx_;
    const char *fn_;
    int status_ = MICV_OK;
    bool drained_ = true;  // nothing enqueued yet
    void *blocks_[kMaxBlocks];
    int nblocks_ = 0;
    const char *name_ = nullptr;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

// The device call of a `_host` function, bracketed for the kernel log under the reference's kernel name.
#define MICV_TIMED(h, kernel, call)                 \
    do {                                            \
        (h).begin(kernel);                          \
        const int rc_timed_ = (call);               \
        (h).end();                                  \
        if (rc_timed_ != MICV_OK) return rc_timed_; \
    } while (0)

}  // namespace micv
