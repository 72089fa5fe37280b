// ps6_host_loops.cpp -- the host loops that state the contract of the "ps6: driver" block (ParticleFilter::drawParticles of
// shim/micv_shim.hpp, micv_viz::rectangle, and pfDriver of shim/micv_ps6.hpp) on one thread, with no library and no GPU:
// the handful of micv_* calls the shim's ParticleFilter makes are defined HERE and hand back fixed particle lists and
// fixed estimates, so the shim's own loops run as they are.  The stand-alone program of tests/test_ps6_driver_shim.py
// (built there with -fsanitize=address,undefined and run on the CPU) and the one-thread timing probe of
// tools/ps6_driver_profile.py.
//   ps6_host_loops run <cases.txt> <dir>       every case's picture as <dir>/<name>.u8 (the rows with their padding)
//   ps6_host_loops lanes <cases.txt> <dir>     the same pictures from csrc/ps6_lane.hpp, the kernel's lane compiled for the
//                                              host: every lane of the launch (padded to whole workgroups), one by one
//   ps6_host_loops time <rows> <cols> <n> <repeats>   milliseconds per frame of clone + dots + ring
// cases.txt: white-space separated tokens, floats as C99 hex / nan / inf:
//   overlay <name> <ch> <pad> <dots 0|1> <n> <n x, y> <dot colour x 4> <box 0|1> <cx> <cy> <bw> <bh> <box colour x 4>
//   rect <name> <ch> <pad> <x> <y> <w> <h> <colour x 4>
//   driver <name> <rows> <cols> <nframes> <n> <bbox x, y, w, h> then per frame <estimate x, y> <n x, y>
//          (3-channel frames; every frame is kept: <dir>/<name>-f<t>.ppm)
// The image of a case is (x * 7 + y * 13 + c * 29 + 5) % 251 (+ t for a driver frame), the padding 0xA5.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../introtocomputervision_amd/csrc/ps6_lane.hpp"
#include "../../introtocomputervision_amd/shim/micv_ps6.hpp"

using micv_shim::Mat;
using micv_shim::Point2f;

// ---- the library calls of the shim's ParticleFilter, answered from fixed lists ---------------------------------------
static std::vector<std::vector<float>> g_lists;  // the particles after create, after tick 0, ...
static std::vector<Point2f> g_estimates;         // the estimate of tick 0, 1, ...
static size_t g_ticks = 0;
struct micv_pf {
    int n;
};
struct micv_ctx {
    int unused;
};
extern "C" {
const char *micv_last_error(void) { return "ps6_host_loops: no library"; }
int micv_ctx_create(int, micv_ctx **out) {
    static micv_ctx ctx{0};
    *out = &ctx;
    return MICV_OK;
}
int micv_pf_create(micv_ctx *, const uint8_t *, int, int, size_t, int, int, int, int n, int, double, double, float, float, double,
                   uint32_t, uint64_t, micv_pf **out) {
    g_ticks = 0;
    *out = new micv_pf{n};
    return MICV_OK;
}
void micv_pf_destroy(micv_pf *pf) { delete pf; }
int micv_pf_tick_host(micv_pf *, const uint8_t *, size_t, micv_pf_state *state) {
    const Point2f c = g_estimates.at(g_ticks++);
    *state = micv_pf_state{c.x, c.y, 0.f, 0.f, 0u};
    return MICV_OK;
}
int micv_pf_particles_host(micv_pf *pf, float *xy) {
    const std::vector<float> &l = g_lists.at(g_ticks);
    for (int i = 0; i < 2 * pf->n; i++) xy[i] = l.at(i);
    return MICV_OK;
}
}

// ---- the cases -------------------------------------------------------------------------------------------------------
struct Tokens {
    std::vector<std::string> t;
    size_t at = 0;
    bool more() const { return at < t.size(); }
    std::string str() { return t.at(at++); }
    double num() { return std::strtod(t.at(at++).c_str(), nullptr); }
    long long integer() { return std::strtoll(t.at(at++).c_str(), nullptr, 10); }
};

struct Image {
    std::vector<unsigned char> buf;
    Mat view;
    Image(int rows, int cols, int ch, int pad, int add = 0) : buf((size_t)rows * ((size_t)cols * ch + pad), 0xA5) {
        const size_t step = (size_t)cols * ch + pad;
        view = Mat(rows, cols, micv::make_type(micv::CV_8U, ch), buf.data(), step);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++)
                for (int c = 0; c < ch; c++) view.ptr<unsigned char>(y)[x * ch + c] = (unsigned char)((x * 7 + y * 13 + c * 29 + 5) % 251 + add);
    }
    void write(const std::string &path) const {
        std::ofstream f(path, std::ios::binary);
        f.write(reinterpret_cast<const char *>(buf.data()), (std::streamsize)buf.size());
    }
};

static micv_shim::Scalar colour(Tokens &tk) {
    double v[4];
    for (double &d : v) d = tk.num();
    return micv_shim::Scalar(v[0], v[1], v[2], v[3]);
}

static std::vector<float> floats(Tokens &tk, int count) {
    std::vector<float> v(count);
    for (float &f : v) f = (float)tk.num();
    return v;
}

// A filter whose particles are `xy` (at least one slot: the shim refuses an empty filter).
static ParticleFilter filter_with(const std::vector<float> &xy, int rows, int cols) {
    g_lists.assign(1, xy);
    Mat model = Mat::zeros(1, 1, micv::CV_8UC1);
    return ParticleFilter(model, micv_shim::Size(cols, rows), xy.size() / 2, ParticleFilter::SimilarityMode::MEAN_SQ_ERR, 1.0, 1.0);
}

static const int kRows = 37, kCols = 53;

// The launch of csrc/ps6.hip, lane by lane: colours packed by its pack_colour, 256 lanes per workgroup.
static uint32_t pack(const micv_shim::Scalar &c) { return micv::draw::pack_colour(c.val); }
static void run_lanes(micv::Overlay o) {
    const long long lanes = (long long)o.n + (o.ring ? 2LL * o.t.cols + 2LL * o.t.rows : 0);
    for (long long i = 0; i < (lanes + 255) / 256 * 256; i++) micv::overlay_lane(o, i);
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "time" && argc == 6) {
        const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), n = std::atoi(argv[4]), repeats = std::atoi(argv[5]);
        std::vector<float> xy(2 * (size_t)n);
        unsigned s = 12345;
        for (int i = 0; i < n; i++) {
            s = s * 1664525u + 1013904223u;
            xy[2 * i] = (float)(cols / 2 + (int)(s >> 8) % 81 - 40);
            s = s * 1664525u + 1013904223u;
            xy[2 * i + 1] = (float)(rows / 2 + (int)(s >> 8) % 81 - 40);
        }
        ParticleFilter pf = filter_with(xy, rows, cols);
        Image frame(rows, cols, 3, 0);
        unsigned long long sum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < repeats; r++) {
            Mat shown = frame.view.clone();
            micv_ps6::paint(pf, shown, Point2f(cols / 2.f, rows / 2.f), micv_ps6::Size2f(73, 87));
            sum += shown.at<unsigned char>(rows / 2, 3 * (cols / 2) + 1);
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / repeats;
        std::printf("{\"host_loops_ms_per_frame\": %.6f, \"rows\": %d, \"cols\": %d, \"n\": %d, \"repeats\": %d, \"check\": %llu}\n", ms, rows,
                    cols, n, repeats, sum);
        return 0;
    }
    const bool lanes = mode == "lanes";
    if ((mode != "run" && !lanes) || argc != 4) {
        std::fprintf(stderr, "usage: %s run cases.txt dir | time rows cols n repeats\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[2]);
    Tokens tk;
    tk.t.assign(std::istream_iterator<std::string>(in), std::istream_iterator<std::string>());
    const std::string dir = argv[3];
    int done = 0;
    while (tk.more()) {
        const std::string kind = tk.str(), name = tk.str();
        if (kind == "overlay") {
            const int ch = (int)tk.integer(), pad = (int)tk.integer();
            const bool dots = tk.integer() != 0;
            const int n = (int)tk.integer();
            const std::vector<float> xy = floats(tk, 2 * n);
            const micv_shim::Scalar dot = colour(tk);
            const bool box = tk.integer() != 0;
            const std::vector<float> b = floats(tk, 4);
            const micv_shim::Scalar bc = colour(tk);
            Image img(kRows, kCols, ch, pad);
            if (lanes) {
                micv::Overlay o{};
                o.t = micv::draw::Target{img.view.data, img.view.step, kRows, kCols, ch};
                o.xy = xy.data(), o.n = dots ? n : 0;
                o.ring = box ? 2 : 0, o.centre = b.data(), o.bw = b[2], o.bh = b[3];
                o.dot = pack(dot), o.box = pack(bc);
                run_lanes(o);
                img.write(dir + "/" + name + ".u8");
                done++;
                continue;
            }
            if (dots && n > 0) {
                ParticleFilter pf = filter_with(xy, kRows, kCols);
                pf.drawParticles(img.view, dot);
            }
            if (box)
                micv_viz::rectangle(img.view, micv_ps6::boxRect(Point2f(b[0], b[1]), micv_ps6::Size2f(b[2], b[3])),
                                    micv_viz::Scalar(bc.val[0], bc.val[1], bc.val[2], bc.val[3]));
            img.write(dir + "/" + name + ".u8");
        } else if (kind == "rect") {
            const int ch = (int)tk.integer(), pad = (int)tk.integer();
            const int x = (int)tk.integer(), y = (int)tk.integer(), w = (int)tk.integer(), h = (int)tk.integer();
            const micv_shim::Scalar bc = colour(tk);
            Image img(kRows, kCols, ch, pad);
            if (lanes) {
                micv::Overlay o{};
                o.t = micv::draw::Target{img.view.data, img.view.step, kRows, kCols, ch};
                o.ring = 1, o.x = x, o.y = y, o.w = w, o.h = h, o.box = pack(bc);
                run_lanes(o);
                img.write(dir + "/" + name + ".u8");
                done++;
                continue;
            }
            micv_viz::rectangle(img.view, micv_viz::Rect(x, y, w, h), micv_viz::Scalar(bc.val[0], bc.val[1], bc.val[2], bc.val[3]));
            img.write(dir + "/" + name + ".u8");
        } else if (kind == "driver") {
            const int rows = (int)tk.integer(), cols = (int)tk.integer(), nframes = (int)tk.integer(), n = (int)tk.integer();
            const std::vector<float> bb = floats(tk, 4);
            micv_ps6::Tracking tracking;
            tracking.bbox = Point2f(bb[0], bb[1]);
            tracking.bboxSize = micv_ps6::Size2f(bb[2], bb[3]);
            g_estimates.clear();
            std::vector<std::vector<float>> lists(1, std::vector<float>(2 * (size_t)n, 0.f));  // after create: never drawn
            std::vector<Image> frames;
            frames.reserve(nframes);
            std::unordered_set<int> save;
            for (int t = 0; t < nframes; t++) {
                const std::vector<float> c = floats(tk, 2);
                g_estimates.emplace_back(c[0], c[1]);
                lists.push_back(floats(tk, 2 * n));
                frames.emplace_back(rows, cols, 3, 0, t);
                tracking.frames.push_back(frames.back().view);
                save.insert(t);
            }
            // (ParticleFilter's constructor starts from g_lists: set after the last use of filter_with)
            g_lists = lists;
            if (lanes) {
                done++;
                continue;  // (the driver's loop is the shim's; its painting is the overlay cases')
            }
            const std::string conf = "c:\n  num_particles: " + std::to_string(n) + "\n  mse_sigma: 1\n  dynamics_sigma: 1\n  alpha: 0.1\n";
            const micv_config::PFConf pfconf(micv_config::Node::parse(conf).child("c"));
            micv_ps6::pfDriver(tracking, pfconf, ParticleFilter::SimilarityMode::MEAN_SQ_ERR, dir + "/" + name, save);
        } else {
            std::fprintf(stderr, "ps6_host_loops: unknown case kind %s\n", kind.c_str());
            return 3;
        }
        done++;
    }
    std::printf("cases %d\n", done);
    return 0;
}
