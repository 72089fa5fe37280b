// ps2_demo.cpp -- the five problems of the reference's ps2 driver (ProblemSets/ps2_cpp/src/main.cpp:80-327) end to end on
// shim/micv_display.hpp and libmicv.so, without OpenCV:
//   ps2_demo <left.pgm> <right.pgm> <out_dir> [max_radius] [max_range]
// One grey pair stands for pair0, pair1 and pair2.  Window radius and disparity range are those of config/ps2.yaml
// (problem 1: 6 / 3; problems 2-4: 7 / 95; problem 5: 7 / 80, use_gpu_disparity: true), each clipped to the optional
// maxima so that a test can run small images.  Every pair-and-display block is ONE library call
// (ps2::pairAndDisplay -> micv_disparity_pair_display_host): it uploads the two grey images (and the two noise images of
// addNoise, drawn on the host from cv::theRNG()'s continuing state) and downloads the two int8 maps and the 8-bit
// images.  Writes the reference's set of images as PGM: ps2-1-a-{1,2}, ps2-2-a-{1,1-inverted,2}, ps2-3-{a,b}-...,
// ps2-4-{a,b,c}-..., ps2-5-a-...; and the maps of the last block as disp-left.i8 / disp-right.i8.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../../introtocomputervision_amd/shim/micv_display.hpp"
#include "../../introtocomputervision_amd/shim/micv_viz.hpp"

using micv_shim::Mat;

static std::string g_out;

static void write_block(const std::string &stem, const ps2::PairDisplay &d, bool inverted = true) {
    micv_viz::imwrite(g_out + "/" + stem + "-1.pgm", d.left);
    if (inverted) micv_viz::imwrite(g_out + "/" + stem + "-1-inverted.pgm", d.leftInverted);
    micv_viz::imwrite(g_out + "/" + stem + "-2.pgm", d.right);
}

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s left.pgm right.pgm out_dir [max_radius] [max_range]\n", argv[0]);
        return 2;
    }
    try {
        g_out = argv[3];
        const size_t max_r = argc > 4 ? (size_t)std::atoi(argv[4]) : 31, max_d = argc > 5 ? (size_t)std::atoi(argv[5]) : 127;
        auto conf = [&](size_t r, size_t d) {
            ps2::DisparityConfig c;
            c._windowRadius = std::min(r, max_r);
            c._disparityRange = std::min(d, max_d);
            return c;
        };
        const ps2::DisparityConfig p1 = conf(6, 3), p2 = conf(7, 95), p3 = conf(7, 95), p4 = conf(7, 95), p5 = conf(7, 80);
        const bool gpu = true;  // use_gpu_disparity
        // convertTo(CV_32FC1) of the grey images (main.cpp:87-88; cvtColor + convertTo on colour ones, :114-117)
        const Mat left = micv_shim::to_f32(micv_viz::imread(argv[1])), right = micv_shim::to_f32(micv_viz::imread(argv[2]));
        const float contrastFactor = 1.1f;
        Mat noiseL, noiseR;

        // runProblem1
        write_block("ps2-1-a", ps2::pairAndDisplay(false, left, right, gpu, p1, 1.f, Mat(), Mat(), false), false);
        // runProblem2
        write_block("ps2-2-a", ps2::pairAndDisplay(false, left, right, gpu, p2));
        // runProblem3: addNoise(left, right, 0, 10, ...), then the contrast gain
        ps2::drawNoise(left, right, 0, 10, noiseL, noiseR);
        write_block("ps2-3-a", ps2::pairAndDisplay(false, left, right, gpu, p3, 1.f, noiseL, noiseR));
        write_block("ps2-3-b", ps2::pairAndDisplay(false, left, right, gpu, p3, contrastFactor));
        // runProblem4: normalized cross correlation, plain, noisy, contrast-boosted
        write_block("ps2-4-a", ps2::pairAndDisplay(true, left, right, gpu, p4));
        ps2::drawNoise(left, right, 0, 10, noiseL, noiseR);
        write_block("ps2-4-b", ps2::pairAndDisplay(true, left, right, gpu, p4, 1.f, noiseL, noiseR));
        write_block("ps2-4-c", ps2::pairAndDisplay(true, left, right, gpu, p4, contrastFactor));
        // runProblem5
        const ps2::PairDisplay last = ps2::pairAndDisplay(true, left, right, gpu, p5);
        write_block("ps2-5-a", last);
        for (int k = 0; k < 2; k++) {
            const Mat &m = k ? last.rightDisparity : last.leftDisparity;
            std::ofstream f(g_out + (k ? "/disp-right.i8" : "/disp-left.i8"), std::ios::binary);
            for (int y = 0; y < m.rows; y++) f.write(reinterpret_cast<const char *>(m.ptr<int8_t>(y)), m.cols);
        }
        std::printf("ps2_demo: %dx%d, five problems -> %s/ps2-*.pgm\n", left.cols, left.rows, g_out.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ps2_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
