// harris_u8_demo.cpp -- the ps4 corner chain on the 8-bit picture the driver loads (ps4_cpp/src/Solution.cpp:73-74), without
// the convertTo(CV_32F): micv_ps4::harrisCorners8 (one micv_harris_corners_u8_host call) against the harris:: three-call
// path of harrisHelper on the same PGM, as read back by micv_viz::imread -- once whole, once as an ROI at an odd offset
// whose step is the larger picture's, in both arithmetics.  Prints OK and exits 0 only when gradientX, gradientY,
// cornerResponse, corners and cornerLocs are equal byte for byte (and there are corners to compare).
//   harris_u8_demo <directory to write the PGM into>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../introtocomputervision_amd/shim/micv_ps4.hpp"

using micv_shim::Mat;

static unsigned next_u32(unsigned &s) { return s = s * 1664525u + 1013904223u; }

static bool same_plane(const Mat &a, const Mat &b, const char *what) {
    bool ok = a.rows == b.rows && a.cols == b.cols && a.type() == micv_shim::F32 && b.type() == micv_shim::F32;
    for (int y = 0; ok && y < a.rows; y++) ok = std::memcmp(a.ptr<float>(y), b.ptr<float>(y), (size_t)a.cols * 4) == 0;
    if (!ok) std::fprintf(stderr, "%s: the 8-bit result differs from the float one\n", what);
    return ok;
}

static bool compare(const Mat &img8, const micv_config::Harris &h, bool gpu, const char *what) {
    micv_ps4::FeaturesContainer a(img8, h, gpu, ".", "u8"), b(img8, h, gpu, ".", "f32");
    micv_ps4::harrisCorners8(a);
    // harrisHelper's computing steps (micv_ps4.hpp), without its pictures
    const Mat input = micv_shim::to_f32(b.input);
    harris::getGradients(input, h.sobel_kernel_size, b.gradientX, b.gradientY);
    if (gpu) harris::gpu::getCornerResponse(b.gradientX, b.gradientY, h.window_size, h.gaussian_sigma, h.alpha, b.cornerResponse);
    else harris::cpu::getCornerResponse(b.gradientX, b.gradientY, h.window_size, h.gaussian_sigma, h.alpha, b.cornerResponse);
    harris::gpu::refineCorners(b.cornerResponse, h.response_threshold, h.min_distance, b.corners, b.cornerLocs);
    bool ok = same_plane(a.gradientX, b.gradientX, "gradientX") && same_plane(a.gradientY, b.gradientY, "gradientY");
    ok = same_plane(a.cornerResponse, b.cornerResponse, "cornerResponse") && ok;
    ok = same_plane(a.corners, b.corners, "corners") && ok;
    if (a.cornerLocs != b.cornerLocs) {
        std::fprintf(stderr, "%s: cornerLocs differ (%zu against %zu)\n", what, a.cornerLocs.size(), b.cornerLocs.size());
        ok = false;
    }
    if (b.cornerLocs.size() < 3) {  // lists that are empty would compare equal whatever the chain did
        std::fprintf(stderr, "%s: only %zu corners\n", what, b.cornerLocs.size());
        ok = false;
    }
    if (!ok) std::fprintf(stderr, "%s: FAILED\n", what);
    return ok;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: harris_u8_demo <directory>\n");
        return 2;
    }
    try {
        // 8 x 8 blocks of random bytes with two random low bits: block corners are Harris corners
        const int rows = 75, cols = 150;
        Mat pic(rows, cols, micv_shim::U8);
        unsigned seed = 7;
        unsigned char block[16][32];
        for (auto &r : block)
            for (auto &v : r) v = (unsigned char)(next_u32(seed) >> 24);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++) pic.at<uint8_t>(y, x) = block[(y + 3) / 8][(x + 5) / 8] ^ (unsigned char)(next_u32(seed) >> 30);
        const std::string path = std::string(argv[1]) + "/harris_u8_demo.pgm";
        micv_viz::imwrite(path, pic);
        const Mat img = micv_viz::imread(path);
        if (img.type() != micv::CV_8UC1 || img.rows != rows || img.cols != cols) throw std::runtime_error("the PGM did not come back as written");
        const micv_config::Harris h(micv_config::Node::parse("sobel_kernel_size: 3\nwindow_size: 5\ngaussian_sigma: 1.5\nalpha: 0.04\n"
                                                             "response_threshold: 5e8\nmin_distance: 5\n"));
        const micv_config::Harris h7(micv_config::Node::parse("sobel_kernel_size: 5\nwindow_size: 9\ngaussian_sigma: 1.5\nalpha: 0.04\n"
                                                              "response_threshold: 5e8\nmin_distance: 3\n"));
        // an ROI: first pixel 3 bytes into row 2, the step of the whole picture
        const Mat roi(rows - 6, cols - 13, micv_shim::U8, const_cast<uint8_t *>(img.ptr<uint8_t>(2)) + 3, img.step);
        bool ok = roi.step != (size_t)roi.cols;
        ok = compare(img, h, true, "whole picture, harris::gpu") && ok;
        ok = compare(img, h, false, "whole picture, harris::cpu") && ok;
        ok = compare(roi, h, true, "ROI, harris::gpu") && ok;
        ok = compare(roi, h, false, "ROI, harris::cpu") && ok;
        ok = compare(roi, h7, true, "ROI, Sobel 5, window 9") && ok;
        if (!ok) return 1;
        std::puts("OK");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
}
