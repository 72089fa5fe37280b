// stereo_ncc_u8_demo.cpp -- disparityNCorr on the 8-bit Mats ps2's driver loads (ps2_cpp/src/main.cpp:227-229, 304-306),
// without the convertTo(CV_32FC1): an 8-bit ROI pair (views into larger images at odd offsets, steps that differ) through
// ps2::disparityNCorr8 and ps2::disparityNCorrPair8, with useGpuDisparity true and false, against the same images
// converted to float through cuda:: / serial::disparityNCorr and ps2::disparityNCorrPair.  Prints OK and exits 0 only when
// every 8-bit result equals its float counterpart byte for byte.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "../../introtocomputervision_amd/shim/micv_display.hpp"

using micv_shim::Mat;

static unsigned next_u32(unsigned &s) { return s = s * 1664525u + 1013904223u; }

static Mat to_float(const Mat &m) {  // convertTo(CV_32FC1)
    Mat f(m.rows, m.cols, micv_shim::F32);
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) f.at<float>(y, x) = (float)m.at<uint8_t>(y, x);
    return f;
}
static bool same(const Mat &a, const Mat &b, const char *what) {
    bool ok = a.rows == b.rows && a.cols == b.cols && a.type() == micv_shim::S8 && b.type() == micv_shim::S8;
    for (int y = 0; ok && y < a.rows; y++) ok = std::memcmp(a.ptr<int8_t>(y), b.ptr<int8_t>(y), (size_t)a.cols) == 0;
    if (!ok) std::fprintf(stderr, "%s: the 8-bit result differs from the float one\n", what);
    return ok;
}
// a map that holds one value only would compare equal whatever the search did
static bool varied(const Mat &d, const char *what) {
    for (int y = 0; y < d.rows; y++)
        for (int x = 0; x < d.cols; x++)
            if (d.at<int8_t>(y, x) != d.at<int8_t>(0, 0)) return true;
    std::fprintf(stderr, "%s: the map holds a single value\n", what);
    return false;
}

int main() {
    try {
        const int rows = 37, cols = 150, range = 30;
        // two larger 8-bit images; the pair is an ROI of each: first pixels 3 and 5 bytes into a row, steps 163 and 171
        Mat big_l(rows + 4, cols + 13, micv_shim::U8), big_r(rows + 6, cols + 21, micv_shim::U8);
        unsigned seed = 3;
        for (int y = 0; y < big_l.rows; y++)
            for (int x = 0; x < big_l.cols; x++) big_l.at<uint8_t>(y, x) = (uint8_t)(next_u32(seed) >> 24);
        for (int y = 0; y < big_r.rows; y++)
            for (int x = 0; x < big_r.cols; x++) big_r.at<uint8_t>(y, x) = (uint8_t)(next_u32(seed) >> 24);
        Mat left(rows, cols, micv_shim::U8, big_l.ptr<uint8_t>(2) + 3, big_l.step);
        Mat right(rows, cols, micv_shim::U8, big_r.ptr<uint8_t>(1) + 5, big_r.step);
        for (int y = 0; y < rows; y++)  // the right view: the left one 11 columns over, every fourth row its own
            for (int x = 0; x < cols; x++)
                if (y % 4) right.at<uint8_t>(y, x) = left.at<uint8_t>(y, (x + 11) % cols);
        const Mat lf = to_float(left), rf = to_float(right);

        bool ok = left.step != right.step;
        Mat d8, df;
        ps2::disparityNCorr8(left, right, 5, -range, 0, true, d8);
        cuda::disparityNCorr(lf, rf, 5, -range, 0, df);
        ok = same(d8, df, "disparityNCorr8 (cuda::)") && varied(df, "cuda::disparityNCorr") && ok;
        ps2::disparityNCorr8(left, right, 4, -range, 0, false, d8);
        serial::disparityNCorr(lf, rf, 4, -range, 0, df);
        ok = same(d8, df, "disparityNCorr8 (serial::)") && varied(df, "serial::disparityNCorr") && ok;
        ps2::disparityNCorr8(left, right, 12, 0, range, false, d8);  // a radius the tile kernels do not take
        serial::disparityNCorr(lf, rf, 12, 0, range, df);
        ok = same(d8, df, "disparityNCorr8, radius 12") && ok;

        ps2::DisparityConfig config;
        config._windowRadius = 7;
        config._disparityRange = range;
        for (int gpu = 0; gpu < 2; gpu++) {
            Mat l8, r8, l32, r32;
            ps2::disparityNCorrPair8(left, right, gpu != 0, config, l8, r8);
            ps2::disparityNCorrPair(lf, rf, gpu != 0, config, l32, r32);
            ok = same(l8, l32, "disparityNCorrPair8, left") && ok;
            ok = same(r8, r32, "disparityNCorrPair8, right") && ok;
            ok = varied(l32, "disparityNCorrPair, left") && ok;
        }
        if (!ok) return 1;
        std::puts("OK");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
}
