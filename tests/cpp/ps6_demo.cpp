// runProblem1 of ps6 (ProblemSets/ps6_cpp/src/Solution.cpp:17-136) on the shim, with synthetic frames in place of
// the videos: for each of the two configurations (pfconf1 on the clean sequence, pfconf1_noisy on the noisy one) the
// model is frame 0 at cv::Rect(bbox, bboxSize) (float -> int by cvRound, as cv::Rect_<float> converts), the filter
// starts GAUSSIAN at the bbox, and every tick's state and the last tick's particles are printed as hex floats for
// tests/test_pf_shim.py.  drawParticles runs on each frame as the driver does.
//   ps6_demo <ps6.yaml> <bbox.txt> <dir with clean_<t>.u8 / noisy_<t>.u8> <rows> <cols> <nframes>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <tuple>
#include <vector>

#include "../../introtocomputervision_amd/shim/micv_config.hpp"
#include "../../introtocomputervision_amd/shim/micv_shim.hpp"

using micv_shim::Mat;
using micv_shim::Point2f;

static Mat read_frame(const std::string &path, int rows, int cols) {
    Mat m(rows, cols, micv::CV_8UC3);
    std::ifstream f(path, std::ios::binary);
    if (!f.read(reinterpret_cast<char *>(m.data), (std::streamsize)m.step * rows)) throw std::runtime_error(path);
    return m;
}

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    const micv_config::Node cfg = micv_config::Node::load(argv[1]);
    micv_config::BBox box;
    if (!micv_config::load_bbox(argv[2], box)) return 3;
    const std::string dir = argv[3];
    const int rows = std::stoi(argv[4]), cols = std::stoi(argv[5]), nframes = std::stoi(argv[6]);
    const char *runs[2][2] = {{"pfconf1", "clean"}, {"pfconf1_noisy", "noisy"}};
    for (const auto &run : runs) {
        const micv_config::PFConf conf(cfg.child(run[0]));
        std::vector<Mat> frames;
        for (int t = 0; t < nframes; t++) frames.push_back(read_frame(dir + "/" + run[1] + "_" + std::to_string(t) + ".u8", rows, cols));
        const int x = (int)std::nearbyint(box.x), y = (int)std::nearbyint(box.y);
        const int w = (int)std::nearbyint(box.width), h = (int)std::nearbyint(box.height);
        Mat model(h, w, micv::CV_8UC3, frames[0].ptr<unsigned char>(y) + (size_t)x * 3, frames[0].step);
        ParticleFilter pf(model, frames[0].size(), conf.num_particles, ParticleFilter::SimilarityMode::MEAN_SQ_ERR,
                          conf.mse_sigma, conf.dynamics_sigma, Point2f(box.x, box.y));
        for (int t = 0; t < nframes; t++) {
            Point2f c;
            float xv, yv;
            std::tie(c, xv, yv) = pf.tick(frames[t]);
            std::printf("state %s %d %a %a %a %a\n", run[0], t, (double)c.x, (double)c.y, (double)xv, (double)yv);
            Mat shown = frames[t].clone();
            pf.drawParticles(shown, micv_shim::Scalar(0, 255, 0, 0));
        }
        std::printf("particles %s", run[0]);
        for (const Point2f &p : pf.getParticles()) std::printf(" %a %a", (double)p.x, (double)p.y);
        std::printf("\n");
    }
    return 0;
}
