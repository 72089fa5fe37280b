// draw_walk_check.cpp -- csrc/draw.hpp against the contract, pixel for pixel, on one thread with no library and no GPU:
// the stand-alone program of tests/test_draw_walk.py (built there with -fsanitize=address,undefined and run on the CPU).
// Every lane of a walk is run, one by one, into a blank picture, and the picture must equal the one the contract's loop
// paints; a store outside the picture would trip the address sanitizer, an overflow of the 64-bit arithmetic the
// undefined-behaviour one.  Exits 1 at the first difference and prints the segment or circle.
//   lattice   6 x 8 image, every ordered pair of end points with x in [-6, 13], y in [-6, 11]: the narrow and the wide
//             walk with 64 lanes and the narrow walk with 256 lanes (a step per lane, ps1.hip's form) against micv_viz::line
//   long      33 x 65 image, ~1000 fixed-seed segments with end points up to +-2^30, the bounds +-2^30 and +-1e9 among
//             them: narrow against wide against micv_ps4::line and micv_ps3::line_wide
//   int32     the wide walk alone against line_wide up to INT_MIN / INT_MAX
//   circles   circle_walk + circle_reaches against micv_ps4::circle
//   cvRound   cv_round_i32 against micv_ps3::cvRound, f32_to_u8 against micv_ps4::f32_to_u8
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../introtocomputervision_amd/csrc/draw.hpp"
#define MICV_PS4_HOST_LOOPS_ONLY 1
#include "../../introtocomputervision_amd/shim/micv_ps3.hpp"
#include "../../introtocomputervision_amd/shim/micv_ps4.hpp"
#include "../../introtocomputervision_amd/shim/micv_viz.hpp"

namespace draw = micv::draw;
using micv_shim::Mat;

static const uint32_t kColour = 0x030201u;  // B, G, R = 1, 2, 3

struct Picture {
    std::vector<unsigned char> buf;
    int rows, cols;
    Picture(int r, int c) : buf((size_t)r * c * 3, 0), rows(r), cols(c) {}
    void clear() { std::memset(buf.data(), 0, buf.size()); }
    Mat mat() { return Mat(rows, cols, micv::make_type(micv::CV_8U, 3), buf.data(), (size_t)cols * 3); }
    draw::Target target() { return draw::Target{buf.data(), (size_t)cols * 3, rows, cols, 3}; }
    bool operator==(const Picture &o) const { return buf == o.buf; }
};

struct Seg {
    long long x1, y1, x2, y2;
};

static int fail(const char *what, const Seg &s) {
    std::printf("draw_walk_check: %s differs from the contract on (%lld, %lld) -> (%lld, %lld)\n", what, s.x1, s.y1, s.x2, s.y2);
    return 1;
}

// every lane of a launch of `lanes` lanes, one by one, as the kernels run them: each lane cuts the walk itself
template <bool WIDE>
static void header_line(Picture &p, const Seg &s, int lanes) {
    p.clear();
    const draw::Target t = p.target();
    for (int lane = 0; lane < lanes; lane++) {
        const draw::LineWalk w = draw::line_walk(p.rows, p.cols, s.x1, s.y1, s.x2, s.y2);
        const auto paint = [&](long long x, long long y) { draw::put(t, x, y, kColour); };
        if (WIDE) draw::walk_steps(w, lane, lanes, draw::wide_minor(w), paint);
        else draw::walk_steps(w, lane, lanes, draw::narrow_minor(w), paint);
    }
}

static void viz_line(Picture &p, const Seg &s) {
    p.clear();
    Mat m = p.mat();
    micv_viz::line(m, micv_viz::Point{(int)s.x1, (int)s.y1}, micv_viz::Point{(int)s.x2, (int)s.y2}, micv_viz::Scalar(1, 2, 3, 0));
}
static void ps4_line(Picture &p, const Seg &s) {
    p.clear();
    Mat m = p.mat();
    micv_ps4::line(micv_ps4::Window{&m, 0, p.cols}, s.x1, s.y1, s.x2, s.y2, micv_ps4::Colour{1, 2, 3});
}
static void ps3_line(Picture &p, const Seg &s) {
    p.clear();
    Mat m = p.mat();
    micv_ps3::line_wide(m, s.x1, s.y1, s.x2, s.y2, micv_shim::Scalar(1, 2, 3, 0));
}

static int lattice() {
    const int rows = 6, cols = 8;
    Picture want(rows, cols), got(rows, cols);
    long long n = 0;
    for (int x1 = -6; x1 <= 13; x1++)
        for (int y1 = -6; y1 <= 11; y1++)
            for (int x2 = -6; x2 <= 13; x2++)
                for (int y2 = -6; y2 <= 11; y2++, n++) {
                    const Seg s{x1, y1, x2, y2};
                    viz_line(want, s);
                    header_line<false>(got, s, 64);
                    if (!(got == want)) return fail("the narrow walk, 64 lanes,", s);
                    header_line<true>(got, s, 64);
                    if (!(got == want)) return fail("the wide walk, 64 lanes,", s);
                    header_line<false>(got, s, 256);
                    if (!(got == want)) return fail("the narrow walk, a step per lane,", s);
                }
    std::printf("lattice: %lld segments\n", n);
    return 0;
}

struct Lcg {  // the generator of the other probes
    unsigned s;
    unsigned next() { return s = s * 1664525u + 1013904223u; }
    long long within(long long lo, long long hi) {  // lo .. hi, 62 bits of state per draw
        const unsigned long long r = ((unsigned long long)next() << 31) ^ next();
        return lo + (long long)(r % (unsigned long long)(hi - lo + 1));
    }
};

static int long_strokes() {
    const int rows = 33, cols = 65;
    const long long B = 1ll << 30, E9 = 999999936;  // 2^30; the largest float below 1e9, which ps4.hip's coord_ok lets through
    std::vector<Seg> segs = {{-B, -B, B, B},   {-B, B, B, -B},   {B, 5, -B, 20},    {3, -B, 40, B},       {-B, 0, B, rows - 1}, {0, -B, cols - 1, B},
                             {-B, -B, 10, 10}, {B, B, 10, 10},   {-B, B, 64, 0},    {-E9, -E9, E9, E9},   {-E9, 7, E9, 25},     {11, E9, 50, -E9},
                             {E9, -E9, -E9, E9 - 40}, {-B, 16, B, 16}, {32, B, 32, -B}, {-B, -B, -B, -B}, {B, B, B, B},        {-B, -B + 30, B, B}};
    Lcg g{20240607u};
    while (segs.size() < 1000) {
        const unsigned kind = g.next() >> 30;
        const Seg far{g.within(-B, B), g.within(-B, B), g.within(-B, B), g.within(-B, B)};
        if (kind == 0) {  // anywhere: mostly past the image
            segs.push_back(far);
        } else if (kind == 1) {  // one end in or near the image
            segs.push_back(Seg{g.within(-10, cols + 10), g.within(-10, rows + 10), far.x2, far.y2});
        } else {  // through a point in the image: the far end mirrored at it, as far as the bound allows
            const long long px = g.within(0, cols - 1), py = g.within(0, rows - 1);
            const long long hx = far.x1 / 2, hy = far.y1 / 2;  // |p +- h| <= 2^29 + 64
            segs.push_back(Seg{px - hx, py - hy, px + hx, py + hy});
        }
    }
    Picture want(rows, cols), wide(rows, cols), got(rows, cols);
    size_t painted = 0;
    for (const Seg &s : segs) {
        ps3_line(want, s);
        ps4_line(wide, s);
        if (!(wide == want)) return fail("micv_ps4::line (against line_wide)", s);
        header_line<false>(got, s, 64);
        if (!(got == want)) return fail("the narrow walk, 64 lanes,", s);
        header_line<true>(got, s, 64);
        if (!(got == want)) return fail("the wide walk, 64 lanes,", s);
        for (unsigned char b : want.buf) painted += b == 1;
    }
    std::printf("long: %zu segments, %zu pixels\n", segs.size(), painted);
    return painted > 10000 ? 0 : 1;  // (the segments that cross the image do paint)
}

static int full_int32() {
    const int rows = 48, cols = 64;  // the image of tests/_ps3_driver_ref.py and its far cases
    const long long LO = INT_MIN, HI = INT_MAX, FAR = 2147483520ll;
    const std::vector<Seg> segs = {{0, -FAR, 63, FAR}, {-FAR, 0, FAR, 63}, {LO, LO, FAR, FAR}, {LO, FAR, FAR, LO}, {LO, 0, FAR, 47}, {31, LO, 32, FAR},
                                   {FAR, -FAR, -FAR, FAR - 128 * 40}, {-FAR, 24, FAR, 24}, {32, FAR, 32, -FAR},
                                   {-2000000000ll, -1234567936ll, 2100000000ll, 1296000000ll}, {-65536, -65537, 65535ll * 30000, 65536ll * 30000},
                                   {-16777216, -16777215, 16777216 + 60, 16777216 + 47},
                                   {LO, LO, HI, HI}, {LO, HI, HI, LO}, {HI, HI, LO, LO}, {HI, LO, LO, HI}, {LO, 0, HI, 47}, {0, LO, 63, HI}, {LO, LO, 63, 47},
                                   {0, 0, HI, HI}, {LO, 47, HI, 0}, {63, HI, 0, LO}, {LO, LO, LO, LO}, {HI, HI, HI, HI}, {LO, 10, LO, 20}, {5, LO, 5, HI}};
    Picture want(rows, cols), got(rows, cols);
    for (const Seg &s : segs) {
        ps3_line(want, s);
        header_line<true>(got, s, 64);
        if (!(got == want)) return fail("the wide walk, 64 lanes,", s);
    }
    std::printf("int32: %zu segments\n", segs.size());
    return 0;
}

static int one_circle(Picture &want, Picture &got, long long cx, long long cy, long long radius) {
    want.clear();
    Mat m = want.mat();
    micv_ps4::circle(micv_ps4::Window{&m, 0, want.cols}, cx, cy, radius, micv_ps4::Colour{1, 2, 3});
    got.clear();
    const draw::Target t = got.target();
    if (draw::circle_reaches(cx, cy, radius, got.rows, got.cols))
        draw::circle_walk(radius, [&](long long dx, long long dy) {
            for (int k = 0; k < 8; k++) {  // the eight reflections
                const long long a = (k & 4) ? dy : dx, b = (k & 4) ? dx : dy;
                draw::put(t, cx + ((k & 1) ? -a : a), cy + ((k & 2) ? -b : b), kColour);
            }
        });
    if (got == want) return 0;
    std::printf("draw_walk_check: the circle of radius %lld around (%lld, %lld) differs from the contract\n", radius, cx, cy);
    return 1;
}

static int circles() {
    Picture want(6, 8), got(6, 8);
    long long n = 0;
    for (int cx = -6; cx <= 13; cx++)
        for (int cy = -6; cy <= 11; cy++)
            for (int radius = 0; radius <= 40; radius++, n++)
                if (one_circle(want, got, cx, cy, radius)) return 1;
    // the largest radius, far outside: through the image from every side, and out of reach
    const long long far[][2] = {{-32760, 3}, {32770, 2}, {4, -32765}, {3, 32771}, {-23170, -23165}, {100000, 100000}, {-40000, -40000}, {4, 70000}};
    for (const auto &c : far)
        if (one_circle(want, got, c[0], c[1], 32767)) return 1;
    std::printf("circles: %lld and %zu far ones\n", n, sizeof far / sizeof far[0]);
    return 0;
}

static int rounding() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> v = {0.f, -0.f, 0.5f, -0.5f, 1.5f, -1.5f, 2.5f, -2.5f, 3.5f, 254.5f, 255.5f, 256.5f, 8388607.5f, -8388607.5f, 0.49999997f,
                            2147483648.f, -2147483648.f, 2147483520.f, -2147483520.f, -2147483904.f, 4294967296.f, 3e9f, -3e9f, 1e30f,
                            nan, -nan, inf, -inf, 100.f, -100.f, 1e9f, 999999936.f};
    for (float f : v) {
        if (draw::cv_round_i32(f) != micv_ps3::cvRound(f) || draw::f32_to_u8(f) != micv_ps4::f32_to_u8(f)) {
            std::printf("draw_walk_check: cvRound differs from the contract on %a: %d / %d, as a byte %d / %d\n", (double)f, draw::cv_round_i32(f),
                        micv_ps3::cvRound(f), draw::f32_to_u8(f), micv_ps4::f32_to_u8(f));
            return 1;
        }
    }
    std::printf("cvRound: %zu values\n", v.size());
    return 0;
}

int main() {
    if (rounding() || circles() || full_int32() || long_strokes() || lattice()) return 1;
    std::printf("draw_walk_check: ok\n");
    return 0;
}
