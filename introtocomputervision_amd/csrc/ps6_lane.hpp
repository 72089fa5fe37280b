// ps6_lane.hpp -- one lane of the ps6 overlay kernel (ps6.hip), in plain C++ so that the same text also compiles for the
// host: tools/probes/ps6_host_loops.cpp (`lanes`) runs every lane of every test case on the CPU under the address and
// undefined-behaviour sanitizers and the pictures must equal the host loops' (tests/test_ps6_driver_shim.py).
#pragma once
#include "draw.hpp"

namespace micv {

struct Overlay {
    draw::Target t;
    const float *xy;  // n x {x, y}
    int n;
    // the ring: none; the rectangle (x, y, w, h); or the driver's box around *centre (device), bw x bh
    int ring;  // 0, 1, 2
    int x, y, w, h;
    const float *centre;
    float bw, bh;
    uint32_t dot, box;  // bytes 0..3 of a pixel, byte k in bits 8k
};

// Lane i of the overlay: lanes 0 .. n - 1 are the particles, the next 2 cols + 2 rows the pixels of the ring's sides.
MICV_HD inline void overlay_lane(const Overlay &o, const long long i) {
    // the ring of [x0, x1] x [y0, y1], 64-bit: x may be INT_MIN; empty when w <= 0 or h <= 0
    long long x0 = 0, y0 = 0, x1 = -1, y1 = -1;
    if (o.ring) {
        int x = o.x, y = o.y, w = o.w, h = o.h;
        if (o.ring == 2) {  // cv::Rect(Point2f(c.x - w / 2, c.y - h / 2), Size2f(w, h)) -> cv::Rect: four cvRounds
            x = draw::cv_round_i32(o.centre[0] - o.bw / 2.f);
            y = draw::cv_round_i32(o.centre[1] - o.bh / 2.f);
            w = draw::cv_round_i32(o.bw);
            h = draw::cv_round_i32(o.bh);
        }
        if (w > 0 && h > 0) {
            x0 = x, y0 = y;
            x1 = x0 + w - 1, y1 = y0 + h - 1;
        }
    }
    const bool ring = x1 >= x0 && y1 >= y0;
    if (i < o.n) {
        const float px = o.xy[2 * i], py = o.xy[2 * i + 1];
        if (!(px > -2.f && px < (float)o.t.cols + 2.f && py > -2.f && py < (float)o.t.rows + 2.f)) return;  // (NaN too)
        const int cx = (int)rintf(px), cy = (int)rintf(py);
        for (int k = 0; k < 5; k++) {
            const int x = cx + (k == 1 ? -1 : (k == 2 ? 1 : 0)), y = cy + (k == 3 ? -1 : (k == 4 ? 1 : 0));
            if (x < 0 || y < 0 || x >= o.t.cols || y >= o.t.rows) continue;
            if (ring && x >= x0 && x <= x1 && y >= y0 && y <= y1 && (x == x0 || x == x1 || y == y0 || y == y1)) continue;
            draw::put(o.t, x, y, o.dot);
        }
        return;
    }
    if (!ring) return;
    // lanes n .. n + 2 cols - 1: the top and the bottom side by column; then 2 rows lanes: the left and the right by row
    long long j = i - o.n;
    if (j < 2LL * o.t.cols) {
        const long long x = j < o.t.cols ? j : j - o.t.cols, y = j < o.t.cols ? y0 : y1;
        if (y >= 0 && y < o.t.rows && x >= x0 && x <= x1) draw::put(o.t, x, y, o.box);
        return;
    }
    j -= 2LL * o.t.cols;
    if (j < 2LL * o.t.rows) {
        const long long y = j < o.t.rows ? j : j - o.t.rows, x = j < o.t.rows ? x0 : x1;
        if (x >= 0 && x < o.t.cols && y >= y0 && y <= y1) draw::put(o.t, x, y, o.box);
    }
}

}  // namespace micv
