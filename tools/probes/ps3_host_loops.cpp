// ps3_host_loops.cpp -- the host loop that states the contract of the "ps3: driver" block (micv_ps3::line_wide and
// drawSegments of shim/micv_ps3.hpp) on one thread, with no library and no GPU, and the kernel's lane beside it.  The
// stand-alone program of tests/test_ps3_driver_shim.py (built there with -fsanitize=address,undefined and run on the CPU)
// and the one-thread timing probe of tools/ps0_ps3_driver_profile.py.
//   ps3_host_loops run <cases.txt> <dir>     every case's picture as <dir>/<name>.u8 (the rows with their padding)
//   ps3_host_loops lanes <cases.txt> <dir>   the same pictures from csrc/ps3_lane.hpp, the kernel's lane compiled for the
//                                            host: the 64 lanes of every segment's wave, one by one
//   ps3_host_loops time <rows> <cols> <n> <repeats>   milliseconds per picture of clone + n lines through the picture
// cases.txt: `image <rows> <cols>`, then per case `case <name> <ch> <pad> <n> <colour x 4>` and n x 4 float32 bit
// patterns in hexadecimal.  The image of a case is (x * 7 + y * 13 + c * 29 + 5) % 251, the padding 0xA5.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../introtocomputervision_amd/csrc/ps3_lane.hpp"
#include "../../introtocomputervision_amd/shim/micv_ps3.hpp"
#include "../../introtocomputervision_amd/shim/micv_viz.hpp"

using micv_shim::Mat;

struct Image {
    std::vector<unsigned char> buf;
    Mat view;
    Image(int rows, int cols, int ch, int pad) : buf((size_t)rows * ((size_t)cols * ch + pad), 0xA5) {
        const size_t step = (size_t)cols * ch + pad;
        view = Mat(rows, cols, micv::make_type(micv::CV_8U, ch), buf.data(), step);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++)
                for (int c = 0; c < ch; c++) view.ptr<unsigned char>(y)[x * ch + c] = (unsigned char)((x * 7 + y * 13 + c * 29 + 5) % 251);
    }
    void write(const std::string &path) const {
        std::ofstream f(path, std::ios::binary);
        f.write(reinterpret_cast<const char *>(buf.data()), (std::streamsize)buf.size());
    }
};

// The launch of csrc/ps3.hip, lane by lane: colours packed as pack_colour does, a wave of 64 lanes per segment.
static uint32_t pack(const micv_shim::Scalar &c) {
    uint32_t out = 0;
    for (int k = 0; k < 4; k++) out |= (uint32_t)micv_ps3::colourByte(c.val[k]) << (8 * k);
    return out;
}
static void run_lanes(Mat &img, const std::vector<float> &seg, int n, const micv_shim::Scalar &colour) {
    const micv::draw::Target t{img.data, img.step, img.rows, img.cols, img.channels()};
    for (int k = 0; k < n; k++) {
        const float *s = &seg[4 * (size_t)k];
        for (int lane = 0; lane < 64; lane++) micv::seg_lane(t, pack(colour), s[0], s[1], s[2], s[3], lane, 64);
    }
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "time" && argc == 6) {
        const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), n = std::atoi(argv[4]), repeats = std::atoi(argv[5]);
        std::vector<float> seg(4 * (size_t)n);
        unsigned s = 12345;
        for (int i = 0; i < n; i++) {  // left border to right border, as drawEpipolarLines hands them over
            s = s * 1664525u + 1013904223u;
            seg[4 * i] = 0.f, seg[4 * i + 1] = (float)((int)(s >> 8) % (2 * rows) - rows / 2);
            s = s * 1664525u + 1013904223u;
            seg[4 * i + 2] = (float)(cols - 1), seg[4 * i + 3] = (float)((int)(s >> 8) % (2 * rows) - rows / 2);
        }
        Image frame(rows, cols, 3, 0);
        unsigned long long sum = 0;
        double ms[2];
        for (int wide = 0; wide < 2; wide++) {  // micv_viz::line in int (the end points are small here), then line_wide
            const auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < repeats; r++) {
                Mat shown = frame.view.clone();
                if (wide) micv_ps3::drawSegments(shown, seg.data(), n, micv_ps3::kLineColor);
                else
                    for (int i = 0; i < n; i++)
                        micv_viz::line(shown, micv_viz::Point{micv_ps3::cvRound(seg[4 * i]), micv_ps3::cvRound(seg[4 * i + 1])},
                                       micv_viz::Point{micv_ps3::cvRound(seg[4 * i + 2]), micv_ps3::cvRound(seg[4 * i + 3])},
                                       micv_viz::Scalar(0, 255, 0, 0));
                sum += shown.at<unsigned char>(rows / 2, 3 * (cols / 2) + 1);
            }
            ms[wide] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / repeats;
        }
        std::printf("{\"viz_line_ms_per_picture\": %.6f, \"line_wide_ms_per_picture\": %.6f, \"rows\": %d, \"cols\": %d, \"n\": %d, "
                    "\"repeats\": %d, \"check\": %llu}\n", ms[0], ms[1], rows, cols, n, repeats, sum);
        return 0;
    }
    const bool lanes = mode == "lanes";
    if ((mode != "run" && !lanes) || argc != 4) {
        std::fprintf(stderr, "usage: %s run|lanes cases.txt dir | time rows cols n repeats\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[2]);
    std::vector<std::string> tk((std::istream_iterator<std::string>(in)), std::istream_iterator<std::string>());
    size_t at = 0;
    const std::string dir = argv[3];
    int rows = 0, cols = 0, done = 0;
    while (at < tk.size()) {
        const std::string kind = tk.at(at++);
        if (kind == "image") {
            rows = std::atoi(tk.at(at++).c_str());
            cols = std::atoi(tk.at(at++).c_str());
            continue;
        }
        if (kind != "case" || rows <= 0 || cols <= 0) {
            std::fprintf(stderr, "ps3_host_loops: unexpected token %s\n", kind.c_str());
            return 3;
        }
        const std::string name = tk.at(at++);
        const int ch = std::atoi(tk.at(at++).c_str()), pad = std::atoi(tk.at(at++).c_str()), n = std::atoi(tk.at(at++).c_str());
        double c[4];
        for (double &d : c) d = std::strtod(tk.at(at++).c_str(), nullptr);
        const micv_shim::Scalar colour(c[0], c[1], c[2], c[3]);
        std::vector<float> seg(4 * (size_t)n);
        for (float &f : seg) {
            const uint32_t bits = (uint32_t)std::strtoul(tk.at(at++).c_str(), nullptr, 16);
            std::memcpy(&f, &bits, 4);
        }
        Image img(rows, cols, ch, pad);
        if (lanes) run_lanes(img.view, seg, n, colour);
        else micv_ps3::drawSegments(img.view, seg.data(), n, colour);
        img.write(dir + "/" + name + ".u8");
        done++;
    }
    std::printf("cases %d\n", done);
    return 0;
}
