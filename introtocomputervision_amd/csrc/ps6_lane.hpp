// ps6_lane.hpp -- one lane of the ps6 overlay kernel (ps6.hip), in plain C++ so that the same text also compiles for the
// host: tools/probes/ps6_host_loops.cpp (`lanes`) runs every lane of every test case on the CPU under the address and
// undefined-behaviour sanitizers and the pictures must equal the host loops' (tests/test_ps6_driver_shim.py).
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define MICV_PS6_HD __host__ __device__
#else
#define MICV_PS6_HD
#endif

namespace micv {

// cvRound of a float as draw.hpp states it: half to even; INT_MIN for NaN, +-inf and every value outside int.
MICV_PS6_HD inline int cv_round_i32(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)rintf(v);
}

struct Overlay {
    uint8_t *img;
    size_t stride;
    int rows, cols, ch;
    const float *xy;  // n x {x, y}
    int n;
    // the ring: none; the rectangle (x, y, w, h); or the driver's box around *centre (device), bw x bh
    int ring;  // 0, 1, 2
    int x, y, w, h;
    const float *centre;
    float bw, bh;
    uint32_t dot, box;  // bytes 0..3 of a pixel, byte k in bits 8k
};

MICV_PS6_HD inline void put(const Overlay &o, long long x, long long y, uint32_t c) {
    uint8_t *d = o.img + (size_t)y * o.stride + (size_t)x * o.ch;
    const int cn = o.ch < 4 ? o.ch : 4;
    for (int k = 0; k < cn; k++) d[k] = (uint8_t)(c >> (8 * k));
}

// Lane i of the overlay: lanes 0 .. n - 1 are the particles, the next 2 cols + 2 rows the pixels of the ring's sides.
MICV_PS6_HD inline void overlay_lane(const Overlay &o, const long long i) {
    // the ring of [x0, x1] x [y0, y1], 64-bit: x may be INT_MIN; empty when w <= 0 or h <= 0
    long long x0 = 0, y0 = 0, x1 = -1, y1 = -1;
    if (o.ring) {
        int x = o.x, y = o.y, w = o.w, h = o.h;
        if (o.ring == 2) {  // cv::Rect(Point2f(c.x - w / 2, c.y - h / 2), Size2f(w, h)) -> cv::Rect: four cvRounds
            x = cv_round_i32(o.centre[0] - o.bw / 2.f);
            y = cv_round_i32(o.centre[1] - o.bh / 2.f);
            w = cv_round_i32(o.bw);
            h = cv_round_i32(o.bh);
        }
        if (w > 0 && h > 0) {
            x0 = x, y0 = y;
            x1 = x0 + w - 1, y1 = y0 + h - 1;
        }
    }
    const bool ring = x1 >= x0 && y1 >= y0;
    if (i < o.n) {
        const float px = o.xy[2 * i], py = o.xy[2 * i + 1];
        if (!(px > -2.f && px < (float)o.cols + 2.f && py > -2.f && py < (float)o.rows + 2.f)) return;  // (NaN too)
        const int cx = (int)rintf(px), cy = (int)rintf(py);
        for (int k = 0; k < 5; k++) {
            const int x = cx + (k == 1 ? -1 : (k == 2 ? 1 : 0)), y = cy + (k == 3 ? -1 : (k == 4 ? 1 : 0));
            if (x < 0 || y < 0 || x >= o.cols || y >= o.rows) continue;
            if (ring && x >= x0 && x <= x1 && y >= y0 && y <= y1 && (x == x0 || x == x1 || y == y0 || y == y1)) continue;
            put(o, x, y, o.dot);
        }
        return;
    }
    if (!ring) return;
    // lanes n .. n + 2 cols - 1: the top and the bottom side by column; then 2 rows lanes: the left and the right by row
    long long j = i - o.n;
    if (j < 2LL * o.cols) {
        const long long x = j < o.cols ? j : j - o.cols, y = j < o.cols ? y0 : y1;
        if (y >= 0 && y < o.rows && x >= x0 && x <= x1) put(o, x, y, o.box);
        return;
    }
    j -= 2LL * o.cols;
    if (j < 2LL * o.rows) {
        const long long y = j < o.rows ? j : j - o.rows, x = j < o.rows ? x0 : x1;
        if (x >= 0 && x < o.cols && y >= y0 && y <= y1) put(o, x, y, o.box);
    }
}

}  // namespace micv
