// ps5_host_loops.cpp -- what the tail of one denseLKWrapper costs on the host path that existed before csrc/ps5.hip: the
// loops of shim/micv_viz.hpp on ONE thread, no device involved.
//   ps5_host_loops arrows <rows> <cols> <reps>     clone + drawVelocityVectors of a grey 8-bit frame (flow amplitude 3)
//   ps5_host_loops montage <rows> <cols> <reps>    savePyramid's work without the file: four f32 levels -> the 2R x 2C image
// Prints one JSON line: median and minimum of the repetitions in ms.
//   g++ -std=c++17 -O2 tools/probes/ps5_host_loops.cpp -o ps5_host_loops -Lintrotocomputervision_amd -lmicv
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../introtocomputervision_amd/shim/micv_viz.hpp"

using micv_shim::Mat;

static unsigned g_sink = 0;

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const bool montage = std::strcmp(argv[1], "montage") == 0;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), reps = std::atoi(argv[4]);
    unsigned s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.f / 16777216.f); };
    Mat frame(rows, cols, micv::CV_8UC1), u(rows, cols, micv::CV_32FC1), v(rows, cols, micv::CV_32FC1);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            frame.at<unsigned char>(y, x) = (unsigned char)(255 * next());
            u.at<float>(y, x) = 6.f * next() - 3.f;
            v.at<float>(y, x) = 6.f * next() - 3.f;
        }
    std::vector<Mat> levels;
    for (int l = 0; l < 4; l++) {
        levels.emplace_back(rows >> l, cols >> l, micv::CV_32FC1);
        for (int y = 0; y < levels[l].rows; y++)
            for (int x = 0; x < levels[l].cols; x++) levels[l].at<float>(y, x) = 255.f * next();
    }
    std::vector<double> ms;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        if (montage) {
            Mat all(2 * rows, 2 * cols, micv::CV_8UC1);
            for (int k = 0; k < 4; k++) {
                Mat big = micv_viz::resize_nearest(micv_viz::normalize_minmax_u8(levels[k]), rows, cols);
                for (int y = 0; y < rows; y++)
                    std::memcpy(all.ptr<unsigned char>((k / 2) * rows + y) + (k % 2) * cols, big.ptr<unsigned char>(y), (size_t)cols);
            }
            g_sink += all.at<unsigned char>(rows, cols);
        } else {
            Mat img = frame.clone();
            micv_viz::drawVelocityVectors(img, u, v, micv_viz::Scalar(0, 255, 0, 255));
            g_sink += img.at<unsigned char>(rows / 2, cols / 2);
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("{\"probe\": \"%s\", \"rows\": %d, \"cols\": %d, \"reps\": %d, \"ms_median\": %.4f, \"ms_min\": %.4f, \"sink\": %u}\n",
                argv[1], rows, cols, reps, ms[ms.size() / 2], ms[0], g_sink);
    return 0;
}
