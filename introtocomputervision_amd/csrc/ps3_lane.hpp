// ps3_lane.hpp -- one lane of the segment kernel (ps3.hip), in plain C++ so that the same text also compiles for the
// host: tools/probes/ps3_host_loops.cpp (`lanes`) runs every lane of every test case on the CPU under the address and
// undefined-behaviour sanitizers and the pictures must equal the host loop's (tests/test_ps3_driver_shim.py).
//
// The contract is micv_viz::line (shim/micv_viz.hpp) with its integers taken as wide as they need to be, which
// micv_ps3::line_wide (shim/micv_ps3.hpp) states in __int128.  With p1.x <= p2.x, major = max(dx, |dy|) and minor the
// other one, step i of the walk (0 <= i <= major) sits at major coordinate start +- i and at minor coordinate
// start +- m(i), m(i) = (2 minor i + major - 1) div (2 major)  (draw.hpp, line_minor_after).  The end points are any two
// int32 pairs, so major and minor reach 2^32 - 1 and 2 minor i reaches 2^65: nothing below forms that product.
//   * The steps whose MAJOR coordinate lies in the image are i0 .. i0 + count - 1, closed form, count <= max(rows, cols).
//   * N(i0) = 2 minor i0 + major - 1 is divided by D = 2 major once per segment, 16 bits of i0 at a time, each partial
//     dividend below 2^51: N(i0) = q0 D + r0.
//   * Lane j then has m(i0 + j) = q0 + (r0 + 2 minor j) div D, where r0 < 2^33 and 2 minor j < 2^48.
// Only 64-bit unsigned divisions, which the device compiler expands in line (a 128-bit one would call compiler-rt).
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define MICV_PS3_HD __host__ __device__
#else
#define MICV_PS3_HD
#endif

namespace micv {

// cvRound of a float as draw.hpp states it: half to even; INT_MIN for NaN, +-inf and every value outside int.
MICV_PS3_HD inline int ps3_cv_round(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)rintf(v);
}

struct SegTarget {
    uint8_t *img;
    size_t stride;
    int rows, cols, ch;
    uint32_t colour;  // bytes 0..3 of a pixel, byte k in bits 8k
};

// One segment's walk, cut to the steps whose major coordinate is in the image.
struct SegWalk {
    long long a_major, a_minor;  // the coordinates of step 0
    int s_major, s_minor;        // +1 or -1
    bool steep;                  // the major axis is y
    uint64_t minor2, D;          // 2 minor, 2 major (D = 0: a single point)
    long long i0, count;         // steps i0 .. i0 + count - 1
    uint64_t q0, r0;             // N(i0) = q0 D + r0
};

MICV_PS3_HD inline SegWalk seg_walk(int rows, int cols, float fx1, float fy1, float fx2, float fy2) {
    long long x1 = ps3_cv_round(fx1), y1 = ps3_cv_round(fy1), x2 = ps3_cv_round(fx2), y2 = ps3_cv_round(fy2);
    if (x1 > x2) {
        long long t = x1;
        x1 = x2, x2 = t;
        t = y1, y1 = y2, y2 = t;
    }
    const long long dx = x2 - x1, dys = y2 - y1;
    const int sy = dys < 0 ? -1 : 1;
    const long long dy = dys < 0 ? -dys : dys;
    SegWalk w;
    w.steep = dy > dx;
    const uint64_t major = (uint64_t)(w.steep ? dy : dx), minor = (uint64_t)(w.steep ? dx : dy);
    w.a_major = w.steep ? y1 : x1, w.a_minor = w.steep ? x1 : y1;
    w.s_major = w.steep ? sy : 1, w.s_minor = w.steep ? 1 : sy;
    w.minor2 = 2 * minor, w.D = 2 * major;
    // 0 <= a_major + s_major i < len and 0 <= i <= major
    const long long len = w.steep ? rows : cols;
    long long lo, hi;
    if (w.s_major > 0) lo = -w.a_major, hi = len - 1 - w.a_major;
    else lo = w.a_major - (len - 1), hi = w.a_major;
    if (lo < 0) lo = 0;
    if (hi > (long long)major) hi = (long long)major;
    w.i0 = lo, w.count = hi >= lo ? hi - lo + 1 : 0;
    w.q0 = 0, w.r0 = 0;
    if (w.count > 0 && major > 0) {
        // minor2 * i0 + major - 1 = ((minor2 * ih) * 2^16 + minor2 * il) + major - 1, i0 = ih 2^16 + il < 2^32
        const uint64_t ih = (uint64_t)w.i0 >> 16, il = (uint64_t)w.i0 & 0xFFFF;
        const uint64_t hi_part = w.minor2 * ih;  // < 2^33 * 2^16
        const uint64_t q1 = hi_part / w.D, r1 = hi_part % w.D;
        const uint64_t rest = (r1 << 16) + w.minor2 * il + (major - 1);  // < 2^49 + 2^49 + 2^32
        w.q0 = (q1 << 16) + rest / w.D;
        w.r0 = rest % w.D;
    }
    return w;
}

// Lane `lane` of `lanes` paints steps i0 + lane, i0 + lane + lanes, ...
MICV_PS3_HD inline void seg_lane(const SegTarget &t, const SegWalk &w, int lane, int lanes) {
    const long long len_minor = w.steep ? t.cols : t.rows;
    const int cn = t.ch < 4 ? t.ch : 4;
    for (long long j = lane; j < w.count; j += lanes) {
        const uint64_t m = w.D ? w.q0 + (w.r0 + w.minor2 * (uint64_t)j) / w.D : 0;  // <= i <= 2^32
        const long long cmaj = w.a_major + w.s_major * (w.i0 + j);
        const long long cmin = w.a_minor + w.s_minor * (long long)m;
        if (cmin < 0 || cmin >= len_minor) continue;
        const long long x = w.steep ? cmin : cmaj, y = w.steep ? cmaj : cmin;
        uint8_t *d = t.img + (size_t)y * t.stride + (size_t)x * t.ch;
        for (int k = 0; k < cn; k++) d[k] = (uint8_t)(t.colour >> (8 * k));
    }
}

}  // namespace micv
