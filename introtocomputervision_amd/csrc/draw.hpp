// draw.hpp -- the one rasteriser of the overlay kernels, in plain C++ that compiles for the host as well as the device: it
// includes the standard headers only, so tools/probes/draw_walk_check.cpp runs every lane of it on the CPU under the
// address and undefined-behaviour sanitizers against the contract (tests/test_draw_walk.py).  The contract is
// micv_viz::line (shim/micv_viz.hpp), cv::LineIterator's walk, and cv::circle's midpoint walk (shim/micv_ps4.hpp).
//
//   cv_round_i32, f32_to_u8   cvRound and saturate_cast<uchar>(cvRound)
//   pack_colour, size_ok, image_ok   host only: the colour rule and the size checks of the entry points
//   Target, put               an image and its one bounds-checked pixel writer, up to four bytes from a packed word.  A
//                             kernel of 3-channel images builds its Target with the literal 3: put's byte loop then
//                             unrolls to three stores (a Target passed as a kernel argument keeps the loop).
//   read_bgr                  a grey or BGR source pixel as three packed bytes (pixmap.hpp; ps4.hip's dots and glyphs)
//   LineWalk, line_walk       the clip, stated once: the steps of the walk whose MAJOR coordinate lies in the image
//   narrow_minor, wide_minor  the minor coordinate's advance after i major steps, two ways (below)
//   walk_steps                the one loop that deals steps to lanes
//   circle_walk, circle_reaches   the midpoint walk's first octant and the circle-reaches-the-image test
//
// With p1.x <= p2.x, major = max(dx, |dy|) (the tie goes to x) and minor the other one, step i of the walk (0 <= i <=
// major) sits at major coordinate start +- i and at minor coordinate start +- m(i),
//   m(i) = (2 minor i + major - 1) div (2 major)
// (err = major - 2 minor; a step moves the minor axis when err < 0, then err += 2 major - 2 minor, else err -= 2 minor).
//   * NARROW: one signed 64-bit division per step.  PRECONDITION: every end point coordinate has |c| <= 2^30.  Then
//     minor <= major <= 2^31 and an in-image step has i <= 2^30 + 2^15, so 2 minor i + major < 2^63.  ps1.hip (end points
//     within a few hundred image diagonals), ps4.hip (coord_ok: below 1e9) and ps5.hip (below 1e6 + cols) use it: their
//     strokes are mostly shorter than a wave, and the wide form's preparation would cost every lane two more division
//     pairs per stroke.
//   * WIDE: valid for any two int32 points, where major and minor reach 2^32 - 1 and 2 minor i reaches 2^65; nothing forms
//     that product.  N(i0) = 2 minor i0 + major - 1 is divided by D = 2 major once per segment, 16 bits of i0 at a time,
//     each partial dividend below 2^51: N(i0) = q0 D + r0.  Step i0 + j then has m = q0 + (r0 + 2 minor j) div D, where
//     r0 < 2^33 and 2 minor j < 2^48.  Only 64-bit unsigned divisions, which the device compiler expands in line (a
//     128-bit one would call compiler-rt).  ps3.hip uses it.
//
// Everything is in micv::draw: lk_device.hpp keeps a device-only cv_round_i32 of its own on the LK path (one conversion
// instruction), and ps5.hip includes both headers.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define MICV_HD __host__ __device__
#else
#define MICV_HD
#endif

namespace micv {
namespace draw {

// cvRound of a float is x86's cvtss2si: half to even; INT_MIN for NaN, +-inf and every value outside int.
MICV_HD inline int cv_round_i32(float v) { return v >= -2147483648.f && v < 2147483648.f ? (int)rintf(v) : INT_MIN; }

// saturate_cast<uchar>(cvRound(v)): INT_MIN saturates to 0.
MICV_HD inline uint8_t f32_to_u8(float v) {
    const int r = cv_round_i32(v);
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// saturate_cast<uchar>(nearbyint(color[k])), k < 4 (NaN gives 0), byte k in bits 8k: the colour rule of micv_draw_rectangle_*
inline uint32_t pack_colour(const double *c) {
    uint32_t out = 0;
    for (int k = 0; k < 4; k++) {
        const double v = std::nearbyint(c[k]);
        const uint32_t b = !(v > 0) ? 0u : (v > 255 ? 255u : (uint32_t)v);
        out |= b << (8 * k);
    }
    return out;
}

inline bool size_ok(int rows, int cols, int max_side) { return rows > 0 && cols > 0 && rows <= max_side && cols <= max_side; }
// ... and a stride that holds a row of ch-byte pixels
inline bool image_ok(int rows, int cols, int ch, size_t stride, int max_side) {
    return size_ok(rows, cols, max_side) && stride >= (size_t)cols * ch;
}

struct Target {
    uint8_t *img;
    size_t stride;
    int rows, cols, ch;
};

// One bounds-checked pixel (micv_viz::put_pixel): bytes 0 .. min(ch, 4) - 1 of `colour`, byte k in bits 8k.
MICV_HD inline void put(const Target &t, long long x, long long y, uint32_t colour) {
    if (x < 0 || x >= t.cols || y < 0 || y >= t.rows) return;
    uint8_t *d = t.img + (size_t)y * t.stride + (size_t)x * t.ch;
    const int cn = t.ch < 4 ? t.ch : 4;
    for (int k = 0; k < cn; k++) d[k] = (uint8_t)(colour >> (8 * k));
}

// Pixel x of a source row as B, G, R in bits 0, 8, 16: grey replicated (a float through f32_to_u8), or the three bytes.
template <typename T, int CN>
MICV_HD inline uint32_t read_bgr(const T *row, int x) {
    static_assert(CN == 1 || (CN == 3 && sizeof(T) == 1), "grey 8-bit or float, or 8-bit BGR");
    if (CN == 3) return (uint32_t)row[3 * (size_t)x] | (uint32_t)row[3 * (size_t)x + 1] << 8 | (uint32_t)row[3 * (size_t)x + 2] << 16;
    const uint32_t v = sizeof(T) == 4 ? f32_to_u8((float)row[x]) : (uint8_t)row[x];
    return v * 0x010101u;
}

// micv_viz::line(p1, p2), cut to the steps i0 .. i0 + count - 1 whose major coordinate is in a rows x cols image
// (count <= max(rows, cols)).  Any end points whose differences fit long long.
struct LineWalk {
    long long a_major, a_minor;  // the coordinates of step 0
    int s_major, s_minor;        // +1 or -1
    bool steep;                  // the major axis is y
    long long major, minor;      // major = 0: a single point
    long long i0, count;
};

MICV_HD inline LineWalk line_walk(int rows, int cols, long long x1, long long y1, long long x2, long long y2) {
    if (x1 > x2) {
        long long t = x1;
        x1 = x2, x2 = t;
        t = y1, y1 = y2, y2 = t;
    }
    const long long dx = x2 - x1, dys = y2 - y1;
    const int sy = dys < 0 ? -1 : 1;
    const long long dy = dys < 0 ? -dys : dys;
    LineWalk w;
    w.steep = dy > dx;
    w.major = w.steep ? dy : dx, w.minor = w.steep ? dx : dy;
    w.a_major = w.steep ? y1 : x1, w.a_minor = w.steep ? x1 : y1;
    w.s_major = w.steep ? sy : 1, w.s_minor = w.steep ? 1 : sy;
    // 0 <= a_major + s_major i < len and 0 <= i <= major
    const long long len = w.steep ? rows : cols;
    long long lo, hi;
    if (w.s_major > 0) lo = -w.a_major, hi = len - 1 - w.a_major;
    else lo = w.a_major - (len - 1), hi = w.a_major;
    if (lo < 0) lo = 0;
    if (hi > w.major) hi = w.major;
    w.i0 = lo, w.count = hi >= lo ? hi - lo + 1 : 0;
    return w;
}

// m(i), narrow form (the precondition is in the header comment).
struct NarrowMinor {
    long long minor, major;
    MICV_HD long long operator()(long long i) const { return major == 0 ? 0 : (2 * minor * i + major - 1) / (2 * major); }
};
MICV_HD inline NarrowMinor narrow_minor(const LineWalk &w) { return NarrowMinor{w.minor, w.major}; }

// m(i), wide form: prepared once per segment, then one unsigned 64-bit division per step.
struct WideMinor {
    uint64_t minor2, D;  // 2 minor, 2 major
    uint64_t q0, r0;     // N(i0) = q0 D + r0
    long long i0;
    MICV_HD long long operator()(long long i) const {
        return D ? (long long)(q0 + (r0 + minor2 * (uint64_t)(i - i0)) / D) : 0;  // <= i <= 2^32
    }
};
MICV_HD inline WideMinor wide_minor(const LineWalk &w) {
    WideMinor m{2 * (uint64_t)w.minor, 2 * (uint64_t)w.major, 0, 0, w.i0};
    if (w.count > 0 && w.major > 0) {
        // minor2 * i0 + major - 1 = ((minor2 * ih) * 2^16 + minor2 * il) + major - 1, i0 = ih 2^16 + il < 2^32
        const uint64_t ih = (uint64_t)w.i0 >> 16, il = (uint64_t)w.i0 & 0xFFFF;
        const uint64_t hi_part = m.minor2 * ih;  // < 2^33 * 2^16
        const uint64_t q1 = hi_part / m.D, r1 = hi_part % m.D;
        const uint64_t rest = (r1 << 16) + m.minor2 * il + ((uint64_t)w.major - 1);  // < 2^49 + 2^49 + 2^32
        m.q0 = (q1 << 16) + rest / m.D;
        m.r0 = rest % m.D;
    }
    return m;
}

// Lane `lane` of `lanes` visits steps i0 + lane, i0 + lane + lanes, ... as visit(x, y); the major coordinate is in the
// image, the minor one may not be (put checks both).  One step per thread is the same loop with lanes = the thread count.
template <typename Minor, typename Visit>
MICV_HD inline void walk_steps(const LineWalk &w, long long lane, long long lanes, Minor minor_after, Visit visit) {
    for (long long j = lane; j < w.count; j += lanes) {
        const long long i = w.i0 + j;
        const long long cmaj = w.a_major + w.s_major * i, cmin = w.a_minor + w.s_minor * minor_after(i);
        visit(w.steep ? cmin : cmaj, w.steep ? cmaj : cmin);
    }
}

// cv::circle, thickness 1: the first octant of the midpoint walk of OpenCV 3.4's drawing.cpp as visit(dx, dy), dx >= dy;
// the circle's pixels are centre + (+-dx, +-dy) and centre + (+-dy, +-dx).
template <typename Visit>
MICV_HD inline void circle_walk(long long radius, Visit visit) {
    long long err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        visit(dx, dy);
        dy++;
        err += plus;
        plus += 2;
        const long long mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// Every pixel of the walk is within 1 of `radius` from the centre: false for a circle that cannot reach the image, whose
// walk would only cost time.  The centre may be negative; for a centre with cx, cy >= 0 the last two terms always hold.
MICV_HD inline bool circle_reaches(long long cx, long long cy, long long radius, int rows, int cols) {
    return !(radius - 1 > (cx < 0 ? -cx : cx) + (cy < 0 ? -cy : cy) + rows + cols) && !(radius + 1 < cx - (cols - 1)) &&
           !(radius + 1 < cy - (rows - 1)) && !(radius + 1 < -cx) && !(radius + 1 < -cy);
}

}  // namespace draw
}  // namespace micv
