// ps6.hip -- what the ps6 driver (ProblemSets/ps6_cpp/src/Solution.cpp:16-107, pfDriver) does around ParticleFilter::tick:
//   * ParticleFilter::drawParticles (lib/ParticleFilter.cpp:82-86): a dot per particle;
//   * cv::rectangle around the estimate (:76-78): the one-pixel ring of the tracking box;
//   * the loop body as one call (tick, then the overlay), and the whole loop over a host sequence with the annotated
//     frames that the driver keeps (saveFrames, or every frame for the video writer) coming back.
// The contract is the host loops of the shim: ParticleFilter::drawParticles (shim/micv_shim.hpp) and micv_viz::rectangle
// (shim/micv_viz.hpp); DESIGN.md section 2 ("ps6 driver"), PARITY WITH OPENCV'S RASTERISER UNPINNED.  Nothing here
// synchronises the host between ticks or reads the particles or the estimate on the host.
//
// One launch paints both: a lane per particle (its centre and four neighbours) and a lane per pixel of the ring's four
// sides.  No owner plane and no atomics are needed, unlike ps4.hip: all dots share one colour, so overlapping dots store
// equal bytes, and so do the ring's corners, which two of its sides reach.  The painter draws the dots first and the ring
// second; here a dot lane skips every pixel that satisfies the ring's closed-form predicate, so the ring's lanes are the
// only writers of the ring and it wins wherever the two overlap, within one launch.
#include <climits>
#include <cmath>
#include <vector>

#include "pf.hpp"
#include "ps6_lane.hpp"

namespace micv {
namespace {

constexpr int kOverlayThreads = 256;

__global__ void __launch_bounds__(kOverlayThreads) ps6_overlay_kernel(const Overlay o) {
    overlay_lane(o, (long long)blockIdx.x * kOverlayThreads + threadIdx.x);
}

// draw.hpp's check with this file's largest side, and a stride that fits 32 bits
bool image_ok(int rows, int cols, int ch, size_t stride) {
    return draw::image_ok(rows, cols, ch, stride, 32767) && stride < (size_t)1 << 32;
}

int launch_overlay(const Overlay &o, hipStream_t s) {
    const long long lanes = (long long)o.n + (o.ring ? 2LL * o.t.cols + 2LL * o.t.rows : 0);
    if (lanes == 0) return MICV_OK;
    ps6_overlay_kernel<<<cdiv((unsigned)lanes, kOverlayThreads), kOverlayThreads, 0, s>>>(o);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

Overlay pf_overlay(micv_pf *pf, uint8_t *frame, size_t stride, const double *dot, float bw, float bh, const double *box) {
    Overlay o{};
    o.t = draw::Target{frame, stride, pf->rows, pf->cols, pf->ch};
    o.xy = reinterpret_cast<const float *>(pf->parts), o.n = pf->n;
    o.ring = 2, o.centre = &pf->state->x, o.bw = bw, o.bh = bh;
    o.dot = draw::pack_colour(dot), o.box = draw::pack_colour(box);
    return o;
}

// tick, then the overlay into `out` (device; may be the frame): the copy first, the overlay after pf_model_kernel in
// stream order, so the tracker never sees the paint.
int enqueue_tick_display(micv_pf *pf, const uint8_t *frame, size_t stride, uint8_t *out, size_t ostride, const double *dot,
                         float bw, float bh, const double *box, hipStream_t s, micv_pf_state *state_out) {
    if (out != frame)
        MICV_HIP(hipMemcpy2DAsync(out, ostride, frame, stride, (size_t)pf->cols * pf->ch, pf->rows, hipMemcpyDeviceToDevice, s));
    MICV_TRY(pf_enqueue_tick(pf, frame, stride, s, state_out));
    return launch_overlay(pf_overlay(pf, out, ostride, dot, bw, bh, box), s);
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_draw_particles_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                            const double *color, micv_stream stream) {
    MICV_REQUIRE(ctx && img && color && n >= 0 && (n == 0 || xy), "micv_draw_particles: null argument or n = %d < 0", n);
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_draw_particles: %d channels not supported (1, 3, 4)", channels);
    MICV_REQUIRE(image_ok(rows, cols, channels, stride), "micv_draw_particles: bad size %dx%d (1..32767) or stride %zu", rows, cols,
                 stride);
    MICV_HIP(hipSetDevice(ctx->device));
    Overlay o{};
    o.t = draw::Target{img, stride, rows, cols, channels}, o.xy = xy, o.n = n;
    o.dot = draw::pack_colour(color);
    return launch_overlay(o, static_cast<hipStream_t>(stream));
}

int micv_draw_rectangle_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, int x, int y, int w, int h,
                            const double *color, micv_stream stream) {
    MICV_REQUIRE(ctx && img && color, "micv_draw_rectangle: null argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_draw_rectangle: %d channels not supported (1, 3, 4)", channels);
    MICV_REQUIRE(image_ok(rows, cols, channels, stride), "micv_draw_rectangle: bad size %dx%d (1..32767) or stride %zu", rows, cols,
                 stride);
    MICV_HIP(hipSetDevice(ctx->device));
    Overlay o{};
    o.t = draw::Target{img, stride, rows, cols, channels};
    o.ring = 1, o.x = x, o.y = y, o.w = w, o.h = h;
    o.box = draw::pack_colour(color);
    return launch_overlay(o, static_cast<hipStream_t>(stream));
}

int micv_ps6_overlay_list_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                              const double *dot_color, const float *centre, float bbox_w, float bbox_h, const double *box_color,
                              micv_stream stream) {
    MICV_REQUIRE(ctx && img && dot_color && centre && box_color && n >= 0 && (n == 0 || xy),
                 "micv_ps6_overlay_list: null argument or n = %d < 0", n);
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_ps6_overlay_list: %d channels not supported (1, 3, 4)", channels);
    MICV_REQUIRE(image_ok(rows, cols, channels, stride), "micv_ps6_overlay_list: bad size %dx%d (1..32767) or stride %zu", rows, cols,
                 stride);
    MICV_HIP(hipSetDevice(ctx->device));
    Overlay o{};
    o.t = draw::Target{img, stride, rows, cols, channels}, o.xy = xy, o.n = n;
    o.ring = 2, o.centre = centre, o.bw = bbox_w, o.bh = bbox_h;
    o.dot = draw::pack_colour(dot_color), o.box = draw::pack_colour(box_color);
    return launch_overlay(o, static_cast<hipStream_t>(stream));
}

int micv_ps6_overlay_dev(micv_pf *pf, uint8_t *frame, size_t stride, const double *dot_color, float bbox_w, float bbox_h,
                         const double *box_color, micv_stream stream) {
    MICV_REQUIRE(pf && frame && dot_color && box_color, "micv_ps6_overlay_dev: null argument");
    MICV_REQUIRE(image_ok(pf->rows, pf->cols, pf->ch, stride), "micv_ps6_overlay_dev: stride %zu < %d, or a frame beyond 32767", stride,
                 pf->cols * pf->ch);
    MICV_HIP(hipSetDevice(pf->device));
    return launch_overlay(pf_overlay(pf, frame, stride, dot_color, bbox_w, bbox_h, box_color), static_cast<hipStream_t>(stream));
}

int micv_ps6_tick_display_dev(micv_pf *pf, const uint8_t *frame, size_t stride, uint8_t *out, size_t ostride, const double *dot_color,
                              float bbox_w, float bbox_h, const double *box_color, micv_stream stream, micv_pf_state *state_dev) {
    MICV_REQUIRE(pf && frame && out && dot_color && box_color, "micv_ps6_tick_display_dev: null argument");
    MICV_REQUIRE(image_ok(pf->rows, pf->cols, pf->ch, stride) && image_ok(pf->rows, pf->cols, pf->ch, ostride),
                 "micv_ps6_tick_display_dev: stride %zu or %zu < %d, or a frame beyond 32767", stride, ostride, pf->cols * pf->ch);
    MICV_REQUIRE(out != frame || ostride == stride, "micv_ps6_tick_display_dev: in place, but the strides differ");
    MICV_HIP(hipSetDevice(pf->device));
    return enqueue_tick_display(pf, frame, stride, out, ostride, dot_color, bbox_w, bbox_h, box_color, static_cast<hipStream_t>(stream),
                                state_dev);
}

int micv_ps6_tick_display_host(micv_pf *pf, const uint8_t *frame, size_t stride, uint8_t *out, size_t ostride, const double *dot_color,
                               float bbox_w, float bbox_h, const double *box_color, micv_pf_state *state) {
    MICV_REQUIRE(pf && frame && out && dot_color && box_color && state, "micv_ps6_tick_display_host: null argument");
    const size_t rb = (size_t)pf->cols * pf->ch;
    MICV_REQUIRE(image_ok(pf->rows, pf->cols, pf->ch, stride) && ostride >= rb, "micv_ps6_tick_display_host: stride %zu or %zu < %zu",
                 stride, ostride, rb);
    MICV_REQUIRE(out != frame || ostride == stride, "micv_ps6_tick_display_host: in place, but the strides differ");
    MICV_HIP(hipSetDevice(pf->device));
    MICV_TRY(pf_frame_buffers(pf));
    hipStream_t s = nullptr;
    uint8_t *buf = pf->frame_buf[0];
    MICV_HIP(hipMemcpy2DAsync(buf, rb, frame, stride, rb, pf->rows, hipMemcpyHostToDevice, s));
    int rc = enqueue_tick_display(pf, buf, rb, buf, rb, dot_color, bbox_w, bbox_h, box_color, s, nullptr);
    if (rc == MICV_OK && hipMemcpy2DAsync(out, ostride, buf, rb, rb, pf->rows, hipMemcpyDeviceToHost, s) != hipSuccess) rc = MICV_EHIP;
    if (rc == MICV_OK && hipMemcpyAsync(state, pf->state, sizeof(micv_pf_state), hipMemcpyDeviceToHost, s) != hipSuccess) rc = MICV_EHIP;
    MICV_HIP(hipStreamSynchronize(s));  // whichever way: nothing may still write into the caller's memory
    if (rc == MICV_EHIP) set_error("micv_ps6_tick_display_host: a copy failed");
    return rc;
}

int micv_ps6_track_display_seq_host(micv_pf *pf, const uint8_t *const *frames, int nframes, size_t stride, const double *dot_color,
                                    float bbox_w, float bbox_h, const double *box_color, const int *save, int nsave, int all_frames,
                                    uint8_t *const *out_frames, size_t ostride, micv_pf_state *states) {
    MICV_REQUIRE(pf && frames && states && dot_color && box_color && nframes >= 1 && nsave >= 0,
                 "micv_ps6_track_display_seq_host: bad argument");
    const size_t rb = (size_t)pf->cols * pf->ch;
    MICV_REQUIRE(image_ok(pf->rows, pf->cols, pf->ch, stride), "micv_ps6_track_display_seq_host: stride %zu < %zu", stride, rb);
    for (int t = 0; t < nframes; t++) MICV_REQUIRE(frames[t], "micv_ps6_track_display_seq_host: frame %d is null", t);
    const int nout = all_frames ? nframes : nsave;
    MICV_REQUIRE(nout == 0 || (out_frames && ostride >= rb && (all_frames || save)),
                 "micv_ps6_track_display_seq_host: frames are kept, but the output list is null or its stride %zu < %zu", ostride, rb);
    // the destinations of frame t: dest[first[t] .. first[t + 1])
    std::vector<int> first(nframes + 1, 0);
    std::vector<uint8_t *> dest(nout);
    for (int k = 0; k < nout; k++) {
        MICV_REQUIRE(out_frames[k], "micv_ps6_track_display_seq_host: output %d is null", k);
        const int t = all_frames ? k : save[k];
        MICV_REQUIRE(t >= 0 && t < nframes, "micv_ps6_track_display_seq_host: save index %d outside 0 .. %d", t, nframes - 1);
        first[t + 1]++;
    }
    for (int t = 0; t < nframes; t++) first[t + 1] += first[t];
    {
        std::vector<int> fill(first.begin(), first.end() - 1);
        for (int k = 0; k < nout; k++) dest[fill[all_frames ? k : save[k]]++] = out_frames[k];
    }
    MICV_HIP(hipSetDevice(pf->device));
    MICV_TRY(pf_frame_buffers(pf));
    struct Scope {  // released on every way out, after everything enqueued has finished
        hipStream_t copy = nullptr, run = nullptr;
        std::vector<hipEvent_t> ev;
        void *st = nullptr;
        ~Scope() {
            for (hipStream_t s : {copy, run})
                if (s) (void)hipStreamSynchronize(s);
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
            for (hipStream_t s : {copy, run})
                if (s) (void)hipStreamDestroy(s);
            if (st) (void)hipFree(st);
        }
    } sc;
    MICV_HIP(hipStreamCreateWithFlags(&sc.copy, hipStreamNonBlocking));
    MICV_HIP(hipStreamCreateWithFlags(&sc.run, hipStreamNonBlocking));
    MICV_HIP(hipMalloc(&sc.st, (size_t)nframes * sizeof(micv_pf_state)));
    std::vector<hipEvent_t> ev_up(nframes), ev_tick(nframes);
    sc.ev.reserve(2 * (size_t)nframes);
    for (auto *v : {&ev_up, &ev_tick})
        for (auto &e : *v) {
            MICV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            sc.ev.push_back(e);
        }
    micv_pf_state *dst = static_cast<micv_pf_state *>(sc.st);
    // Uploads and downloads share the copy stream.  The upload of frame t + 2 follows the download of frame t there, which
    // waits for tick t and its overlay: a buffer is written again only after its last reader and its download are done.
    auto upload = [&](int t) -> int {
        if (t >= 2) MICV_HIP(hipStreamWaitEvent(sc.copy, ev_tick[t - 2], 0));
        MICV_HIP(hipMemcpy2DAsync(pf->frame_buf[t & 1], rb, frames[t], stride, rb, pf->rows, hipMemcpyHostToDevice, sc.copy));
        MICV_HIP(hipEventRecord(ev_up[t], sc.copy));
        return MICV_OK;
    };
    MICV_TRY(upload(0));
    for (int t = 0; t < nframes; t++) {
        uint8_t *buf = pf->frame_buf[t & 1];
        MICV_HIP(hipStreamWaitEvent(sc.run, ev_up[t], 0));
        MICV_TRY(enqueue_tick_display(pf, buf, rb, buf, rb, dot_color, bbox_w, bbox_h, box_color, sc.run, dst + t));
        MICV_HIP(hipEventRecord(ev_tick[t], sc.run));
        if (t + 1 < nframes) MICV_TRY(upload(t + 1));  // beside tick t
        if (first[t + 1] > first[t]) {
            MICV_HIP(hipStreamWaitEvent(sc.copy, ev_tick[t], 0));
            for (int k = first[t]; k < first[t + 1]; k++)
                MICV_HIP(hipMemcpy2DAsync(dest[k], ostride, buf, rb, rb, pf->rows, hipMemcpyDeviceToHost, sc.copy));
        }
    }
    MICV_HIP(hipMemcpyAsync(states, sc.st, (size_t)nframes * sizeof(micv_pf_state), hipMemcpyDeviceToHost, sc.run));
    MICV_HIP(hipStreamSynchronize(sc.run));
    MICV_HIP(hipStreamSynchronize(sc.copy));
    return MICV_OK;
}

int micv_ps6_group_track_display_seq_host(micv_pf_group *g, const uint8_t *const *frames, int nframes, size_t stride,
                                          const double *dot_color, const float *bbox_wh, const double *box_color,
                                          const int *const *save, const int *nsave, int all_frames,
                                          uint8_t *const *const *out_frames, size_t ostride, micv_pf_state *states) {
    MICV_REQUIRE(g && frames && states && dot_color && bbox_wh && box_color && nframes >= 1 && (all_frames || nsave),
                 "micv_ps6_group_track_display_seq_host: bad argument");
    const int count = g->count;
    const size_t rb = (size_t)g->cols * g->ch;
    MICV_REQUIRE(image_ok(g->rows, g->cols, g->ch, stride), "micv_ps6_group_track_display_seq_host: stride %zu < %zu", stride, rb);
    for (int t = 0; t < nframes; t++) MICV_REQUIRE(frames[t], "micv_ps6_group_track_display_seq_host: frame %d is null", t);
    // the destinations of member k's frame t: dest[k][first[k][t] .. first[k][t + 1])
    std::vector<std::vector<int>> first(count, std::vector<int>(nframes + 1, 0));
    std::vector<std::vector<uint8_t *>> dest(count);
    for (int k = 0; k < count; k++) {
        MICV_REQUIRE(all_frames || nsave[k] >= 0, "micv_ps6_group_track_display_seq_host: member %d: nsave = %d", k, nsave[k]);
        const int nout = all_frames ? nframes : nsave[k];
        MICV_REQUIRE(nout == 0 || (out_frames && out_frames[k] && ostride >= rb && (all_frames || (save && save[k]))),
                     "micv_ps6_group_track_display_seq_host: member %d keeps frames, but a list is null or the stride %zu < %zu", k,
                     ostride, rb);
        dest[k].resize(nout);
        for (int j = 0; j < nout; j++) {
            MICV_REQUIRE(out_frames[k][j], "micv_ps6_group_track_display_seq_host: output %d of member %d is null", j, k);
            const int t = all_frames ? j : save[k][j];
            MICV_REQUIRE(t >= 0 && t < nframes, "micv_ps6_group_track_display_seq_host: member %d: save index %d outside 0 .. %d", k,
                         t, nframes - 1);
            first[k][t + 1]++;
        }
        for (int t = 0; t < nframes; t++) first[k][t + 1] += first[k][t];
        std::vector<int> fill(first[k].begin(), first[k].end() - 1);
        for (int j = 0; j < nout; j++) dest[k][fill[all_frames ? j : save[k][j]]++] = out_frames[k][j];
    }
    MICV_HIP(hipSetDevice(g->device));
    MICV_TRY(pf_group_frame_buffers(g));
    struct Scope {  // released on every way out, after everything enqueued has finished
        hipStream_t copy = nullptr, run = nullptr;
        std::vector<hipEvent_t> ev;
        std::vector<void *> mem;
        ~Scope() {
            for (hipStream_t s : {copy, run})
                if (s) (void)hipStreamSynchronize(s);
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
            for (hipStream_t s : {copy, run})
                if (s) (void)hipStreamDestroy(s);
            for (void *p : mem)
                if (p) (void)hipFree(p);
        }
    } sc;
    MICV_HIP(hipStreamCreateWithFlags(&sc.copy, hipStreamNonBlocking));
    MICV_HIP(hipStreamCreateWithFlags(&sc.run, hipStreamNonBlocking));
    // the states, then two scratch pictures (frame parity) for every member that keeps a frame
    sc.mem.assign(1 + 2 * (size_t)count, nullptr);
    MICV_HIP(hipMalloc(&sc.mem[0], (size_t)nframes * count * sizeof(micv_pf_state)));
    for (int k = 0; k < count; k++)
        if (!dest[k].empty())
            for (int b = 0; b < 2; b++) MICV_HIP(hipMalloc(&sc.mem[1 + 2 * k + b], g->frame_bytes()));
    std::vector<hipEvent_t> ev_up(nframes), ev_tick(nframes);
    sc.ev.reserve(2 * (size_t)nframes);
    for (auto *v : {&ev_up, &ev_tick})
        for (auto &e : *v) {
            MICV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            sc.ev.push_back(e);
        }
    micv_pf_state *dst = static_cast<micv_pf_state *>(sc.mem[0]);
    // Uploads and downloads share the copy stream; ticks, the copies into the scratch pictures and the overlays share the
    // run stream.  ev_tick[t] follows the last reader of frame buffer t & 1 (the tick and every copy out of it), and the
    // upload of frame t + 2 waits for it.  A scratch picture of parity t & 1 is painted again at frame t + 2 at the
    // earliest; tick t + 2 waits for upload t + 2, which follows the downloads of frame t on the copy stream.
    auto upload = [&](int t) -> int {
        if (t >= 2) MICV_HIP(hipStreamWaitEvent(sc.copy, ev_tick[t - 2], 0));
        MICV_HIP(hipMemcpy2DAsync(g->frame_buf[t & 1], rb, frames[t], stride, rb, g->rows, hipMemcpyHostToDevice, sc.copy));
        MICV_HIP(hipEventRecord(ev_up[t], sc.copy));
        return MICV_OK;
    };
    MICV_TRY(upload(0));
    for (int t = 0; t < nframes; t++) {
        const uint8_t *buf = g->frame_buf[t & 1];
        MICV_HIP(hipStreamWaitEvent(sc.run, ev_up[t], 0));
        MICV_TRY(pf_group_enqueue_tick(g, &buf, &rb, 1, sc.run, dst + (size_t)t * count));
        bool kept = false;
        for (int k = 0; k < count; k++) kept |= first[k][t + 1] > first[k][t];
        for (int k = 0; kept && k < count; k++) {
            if (first[k][t + 1] == first[k][t]) continue;
            uint8_t *pic = static_cast<uint8_t *>(sc.mem[1 + 2 * k + (t & 1)]);
            MICV_HIP(hipMemcpyAsync(pic, buf, g->frame_bytes(), hipMemcpyDeviceToDevice, sc.run));
            MICV_TRY(launch_overlay(pf_overlay(g->members[k], pic, rb, dot_color, bbox_wh[2 * k], bbox_wh[2 * k + 1], box_color), sc.run));
        }
        MICV_HIP(hipEventRecord(ev_tick[t], sc.run));
        if (t + 1 < nframes) MICV_TRY(upload(t + 1));  // beside tick t
        if (kept) {
            MICV_HIP(hipStreamWaitEvent(sc.copy, ev_tick[t], 0));
            for (int k = 0; k < count; k++)
                for (int j = first[k][t]; j < first[k][t + 1]; j++)
                    MICV_HIP(hipMemcpy2DAsync(dest[k][j], ostride, sc.mem[1 + 2 * k + (t & 1)], rb, rb, g->rows, hipMemcpyDeviceToHost,
                                              sc.copy));
        }
    }
    MICV_HIP(hipMemcpyAsync(states, sc.mem[0], (size_t)nframes * count * sizeof(micv_pf_state), hipMemcpyDeviceToHost, sc.run));
    MICV_HIP(hipStreamSynchronize(sc.run));
    MICV_HIP(hipStreamSynchronize(sc.copy));
    return MICV_OK;
}

}  // extern "C"
