// pf.hpp -- the particle filter's handle (pf.hip) for the files that work on its device state (ps6.hip: the driver's
// overlay reads the particles and the estimate where the tick left them).
#pragma once
#include <vector>

#include "common.hpp"

struct micv_pf {
    int device = 0;
    int mrows = 0, mcols = 0, ch = 0, rows = 0, cols = 0, n = 0, mode = 0;
    uint32_t flags = 0;
    double mse_sigma = 0;
    float fa = 0, fb = 0;  // (float)alpha, (float)(1 - alpha)
    float2 *parts = nullptr, *moved = nullptr;  // current particles; displaced particles of the running tick
    double2 *disp = nullptr;                    // displacement table
    float *uni = nullptr;                       // resampling uniforms
    double *sim = nullptr;
    float *weights = nullptr;
    uint8_t *model = nullptr, *model0 = nullptr;  // current model patch / last blend; the original patch
    float *hist = nullptr;                        // model histogram [ch][32]
    micv_pf_state *state = nullptr;
    uint8_t *frame_buf[2] = {nullptr, nullptr};   // host-frame staging of tick_host / track_seq_host
    ~micv_pf() {
        (void)hipSetDevice(device);
        for (void *p : {(void *)parts, (void *)moved, (void *)disp, (void *)uni, (void *)sim, (void *)weights,
                        (void *)model, (void *)model0, (void *)hist, (void *)state, (void *)frame_buf[0],
                        (void *)frame_buf[1]})
            if (p) (void)hipFree(p);
    }
    size_t patch_bytes() const { return (size_t)mrows * mcols * ch; }
    size_t frame_bytes() const { return (size_t)rows * cols * ch; }
};

namespace micv {
// What the three stages of a tick read of one filter: a row of a group's device table (pf.hip).  Pointers into the
// member's own buffers; the group owns none of them.  The row is a snapshot taken at micv_pf_group_create: everything in it
// is fixed for a micv_pf's lifetime today, and must stay so or be refreshed in every group (pf.hip, describe()).
struct PfMember {
    int rows, cols, ch, mrows, mcols, n, mode;
    uint32_t flags;
    double mse_sigma;
    float fa, fb;
    float2 *parts, *moved;
    const double2 *disp;
    const float *uni;
    double *sim;
    float *weights;
    uint8_t *model;
    const uint8_t *model0;
    float *hist;
    micv_pf_state *state;
};
}  // namespace micv

struct micv_pf_group {
    int device = 0, count = 0, max_n = 0;
    int rows = 0, cols = 0, ch = 0;  // the frame every member was made for
    std::vector<micv_pf *> members;  // borrowed
    micv::PfMember *table = nullptr;  // device, count rows
    uint8_t *frame_buf[2] = {nullptr, nullptr};  // host-frame staging of the sequence calls, allocated on first use
    ~micv_pf_group() {
        (void)hipSetDevice(device);
        for (void *p : {(void *)table, (void *)frame_buf[0], (void *)frame_buf[1]})
            if (p) (void)hipFree(p);
    }
    size_t frame_bytes() const { return (size_t)rows * cols * ch; }
};

namespace micv {
// The three launches of one tick on `s` (pf.hip); the state also goes to state_out (device, may be NULL).
int pf_enqueue_tick(micv_pf *pf, const uint8_t *frame, size_t stride, hipStream_t s, micv_pf_state *state_out);
// Allocates pf->frame_buf[0..1] (dense rows x cols x ch) on first use.
int pf_frame_buffers(micv_pf *pf);
// The three launches of a group's tick on `s`: nframes == 1 (a shared frame) or g->count (one each); the arguments
// are checked by the caller.  states_out: device, count entries, may be NULL.
int pf_group_enqueue_tick(micv_pf_group *g, const uint8_t *const *frames, const size_t *strides, int nframes, hipStream_t s,
                          micv_pf_state *states_out);
int pf_group_frame_buffers(micv_pf_group *g);
}  // namespace micv
