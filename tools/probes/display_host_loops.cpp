// display_host_loops.cpp -- what the display tail costs on the host path that existed before csrc/display.hip: the loops of
// shim/micv_viz.hpp on ONE thread, no device involved.
//   display_host_loops jet <rows> <cols> <reps>     normalize_minmax_u8 + apply_colormap_jet of one CV_32FC1 field
//   display_host_loops ps2 <rows> <cols> <reps>     the tail of a ps2 block: two int8 maps -> float -> normalize_minmax_u8,
//                                                   and 255 - x of the left one
// Prints one JSON line: median, minimum and standard deviation of the repetitions in ms.
//   g++ -std=c++17 -O2 tools/probes/display_host_loops.cpp -o display_host_loops -Lintrotocomputervision_amd -lmicv
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../introtocomputervision_amd/shim/micv_viz.hpp"

using micv_shim::Mat;

static unsigned g_sink = 0;

static Mat as_float(const Mat &m) {  // convertTo(CV_32F) of a CV_8SC1 map
    Mat f(m.rows, m.cols, micv::CV_32FC1);
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) f.at<float>(y, x) = (float)m.at<signed char>(y, x);
    return f;
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const bool ps2 = std::strcmp(argv[1], "ps2") == 0;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), reps = std::atoi(argv[4]);
    Mat field(rows, cols, micv::CV_32FC1), dl(rows, cols, micv::CV_8S), dr(rows, cols, micv::CV_8S);
    unsigned s = 12345u;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            s = s * 1664525u + 1013904223u;
            field.at<float>(y, x) = (float)(s >> 8) * (6.f / 16777216.f) - 2.5f;
            dl.at<signed char>(y, x) = (signed char)(-(int)((s >> 9) % 96));
            dr.at<signed char>(y, x) = (signed char)((s >> 17) % 96);
        }
    std::vector<double> ms;
    for (int r = 0; r < reps + 1; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        if (ps2) {
            Mat a = micv_viz::normalize_minmax_u8(as_float(dl)), b = micv_viz::normalize_minmax_u8(as_float(dr));
            Mat inv(rows, cols, micv::CV_8UC1);
            for (int y = 0; y < rows; y++)
                for (int x = 0; x < cols; x++) inv.at<unsigned char>(y, x) = (unsigned char)(255 - a.at<unsigned char>(y, x));
            g_sink += inv.at<unsigned char>(rows / 2, cols / 2) + b.at<unsigned char>(rows / 2, cols / 2);
        } else {
            Mat c = micv_viz::apply_colormap_jet(micv_viz::normalize_minmax_u8(field));
            g_sink += c.at<unsigned char>(rows / 2, cols / 2);
        }
        const auto t1 = std::chrono::steady_clock::now();
        if (r) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());  // the first one warms the pages
    }
    std::sort(ms.begin(), ms.end());
    double mean = 0, var = 0;
    for (double v : ms) mean += v / ms.size();
    for (double v : ms) var += (v - mean) * (v - mean) / ms.size();
    std::printf("{\"mode\": \"%s\", \"rows\": %d, \"cols\": %d, \"reps\": %d, \"ms\": %.4f, \"ms_min\": %.4f, \"ms_std\": %.4f, \"sink\": %u}\n",
                argv[1], rows, cols, reps, ms[ms.size() / 2], ms.front(), std::sqrt(var), g_sink & 1u);
    return 0;
}
