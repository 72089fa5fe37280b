// micv_ps7.hpp -- the MHI stage of the ps7 driver (ProblemSets/ps7_cpp/src/Solution.cpp:16-146) without OpenCV, twice:
//   mhiHelper          the reference's loop as written, on the shim's mhi::frameDifference and mhi::calcMotionHistory:
//                      two synchronous calls per frame, the frames as the capture hands them over (CV_8UC3);
//   mhiHelperDevice    the same two vectors from ONE library call (micv_mhi_history_seq_c_host): every frame uploaded
//                      once, no host synchronisation between the updates, a download of only what is kept;
//   getAllMHIs         the reference's loop over 3 actions x 3 persons x 3 trials around mhiHelper;
//   getAllMHIsDevice   the same histories from one micv_mhi_history_batch_dev call per blur.
// Frames come from a std::vector<Mat> instead of cv::VideoCapture (frame 0 is the capture's first frame).
#pragma once

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "micv_config.hpp"
#include "micv_shim.hpp"

namespace micv_ps7 {

using micv_shim::Mat;
using Video = std::vector<Mat>;
using Videos = std::map<std::string, Video>;  // "PS7A<a>P<p>T<t>" -> decoded frames

// mhiHelper (Solution.cpp:16-101): first the difference frames, then the histories, at the frame numbers of the two
// sets that the video reaches, in frame order.
inline std::pair<std::vector<Mat>, std::vector<Mat>> mhiHelper(const Video &vid, const micv_config::MHI &mhiConf,
                                                               const std::unordered_set<size_t> &saveDiffFrames,
                                                               const std::unordered_set<size_t> &saveMHIFrames) {
    std::vector<Mat> diffFrames, mhiFrames;
    if (vid.empty()) return std::make_pair(diffFrames, mhiFrames);
    Mat lastFrame = vid[0];
    Mat history = Mat::zeros(lastFrame.rows, lastFrame.cols, micv::CV_8UC1);
    size_t frameNum = 1;
    for (size_t i = 1; i < vid.size(); i++, frameNum++) {
        const Mat &frame = vid[i];
        Mat diff;
        mhi::frameDifference(lastFrame, frame, mhiConf.diff_threshold, diff,
                             micv_shim::Size(mhiConf.pre_blur_size, mhiConf.pre_blur_size), mhiConf.pre_blur_sigma);
        mhi::calcMotionHistory(history, diff, mhiConf.tau);
        lastFrame = frame;
        if (saveDiffFrames.count(frameNum)) diffFrames.push_back(diff.clone());
        if (saveMHIFrames.count(frameNum)) mhiFrames.push_back(history.clone());
    }
    return std::make_pair(diffFrames, mhiFrames);
}

namespace detail {
inline std::vector<int> reached(const std::unordered_set<size_t> &save, size_t nframes) {
    std::vector<int> out;
    for (size_t s : save)
        if (s >= 1 && s + 1 <= nframes) out.push_back((int)s);
    std::sort(out.begin(), out.end());
    return out;
}
// The frames of one video, rows dense, one behind the other.
inline std::vector<uint8_t> packed(const Video &vid, size_t row_bytes) {
    const Mat &f0 = vid[0];
    std::vector<uint8_t> buf(vid.size() * row_bytes * (size_t)f0.rows);
    for (size_t i = 0; i < vid.size(); i++) {
        micv_shim::require(vid[i].type() == f0.type() && vid[i].rows == f0.rows && vid[i].cols == f0.cols,
                           "micv_ps7: the frames of a video differ in type or size");
        for (int y = 0; y < f0.rows; y++)
            std::memcpy(buf.data() + (i * f0.rows + y) * row_bytes, vid[i].ptr<uint8_t>(y), row_bytes);
    }
    return buf;
}
inline std::vector<Mat> planes(const std::vector<uint8_t> &buf, int n, int rows, int cols) {
    std::vector<Mat> out;
    for (int i = 0; i < n; i++) {
        Mat m(rows, cols, micv::CV_8UC1);
        for (int y = 0; y < rows; y++) std::memcpy(m.ptr<uint8_t>(y), buf.data() + ((size_t)i * rows + y) * cols, cols);
        out.push_back(m);
    }
    return out;
}
}  // namespace detail

inline std::pair<std::vector<Mat>, std::vector<Mat>> mhiHelperDevice(const Video &vid, const micv_config::MHI &mhiConf,
                                                                     const std::unordered_set<size_t> &saveDiffFrames,
                                                                     const std::unordered_set<size_t> &saveMHIFrames) {
    std::vector<Mat> none;
    if (vid.size() < 2) return std::make_pair(none, none);
    const std::vector<int> sd = detail::reached(saveDiffFrames, vid.size()), sm = detail::reached(saveMHIFrames, vid.size());
    if (sd.empty() && sm.empty()) return std::make_pair(none, none);
    const Mat &f0 = vid[0];
    const int rows = f0.rows, cols = f0.cols, cn = f0.channels();
    micv_shim::require(f0.depth() == micv_shim::U8, "micv_ps7::mhiHelperDevice: CV_8U frames expected");
    const size_t rb = (size_t)cols * cn, n = (size_t)rows * cols;
    const std::vector<uint8_t> buf = detail::packed(vid, rb);
    std::vector<uint8_t> hist(n * std::max<size_t>(sm.size(), 1)), diff(n * std::max<size_t>(sd.size(), 1));
    micv_shim::check(micv_mhi_history_seq_c_host(
        micv_shim::context(), buf.data(), (int)vid.size(), rb * rows, rb, rows, cols, cn, mhiConf.diff_threshold,
        mhiConf.pre_blur_size, mhiConf.pre_blur_size, mhiConf.pre_blur_sigma, mhiConf.tau, sm.empty() ? nullptr : sm.data(),
        (int)sm.size(), sm.empty() ? nullptr : hist.data(), n, cols, sd.empty() ? nullptr : sd.data(), (int)sd.size(),
        sd.empty() ? nullptr : diff.data(), n, cols));
    return std::make_pair(detail::planes(diff, (int)sd.size(), rows, cols), detail::planes(hist, (int)sm.size(), rows, cols));
}

inline std::string videoName(int action, int person, int trial) {
    return "PS7A" + std::to_string(action) + "P" + std::to_string(person) + "T" + std::to_string(trial);
}

// getAllMHIs (Solution.cpp:113-146).  A video that is missing or ends before its last frame of action is left out.
inline void getAllMHIs(const micv_config::Node &cfg, const Videos &videos, std::vector<Mat> &mhiFrames,
                       std::vector<int> &actions, std::vector<int> &people) {
    const std::map<std::string, int> last = micv_config::last_frames(cfg);
    for (int action = 1; action <= 3; action++) {
        const micv_config::MHI curConf(cfg.child("mhi_action" + std::to_string(action)));
        for (int person = 1; person <= 3; person++)
            for (int trial = 1; trial <= 3; trial++) {
                const std::string vidFile = videoName(action, person, trial);
                const auto v = videos.find(vidFile);
                const auto lf = last.find(vidFile);
                if (v == videos.end() || lf == last.end() || lf->second < 1) continue;
                const std::vector<Mat> frame = mhiHelper(v->second, curConf, {}, {(size_t)lf->second}).second;
                if (frame.size() == 1) {
                    mhiFrames.push_back(frame[0]);
                    actions.push_back(action);
                    people.push_back(person);
                }
            }
    }
}

// The same through micv_mhi_history_batch_dev: every video uploaded once, one call per blur (one for config/ps7.yaml),
// the histories downloaded at the end.
inline void getAllMHIsDevice(const micv_config::Node &cfg, const Videos &videos, std::vector<Mat> &mhiFrames,
                             std::vector<int> &actions, std::vector<int> &people) {
    const std::map<std::string, int> last = micv_config::last_frames(cfg);
    struct Item {
        const Video *vid;
        micv_config::MHI conf;
        int save, action, person;
    };
    std::vector<Item> items;
    for (int action = 1; action <= 3; action++) {
        const micv_config::MHI curConf(cfg.child("mhi_action" + std::to_string(action)));
        for (int person = 1; person <= 3; person++)
            for (int trial = 1; trial <= 3; trial++) {
                const std::string vidFile = videoName(action, person, trial);
                const auto v = videos.find(vidFile);
                const auto lf = last.find(vidFile);
                if (v == videos.end() || lf == last.end() || lf->second < 1 || (size_t)lf->second + 1 > v->second.size()) continue;
                items.push_back(Item{&v->second, curConf, lf->second, action, person});
            }
    }
    if (items.empty()) return;
    micv_ctx *ctx = micv_shim::context();
    const Mat &f0 = (*items[0].vid)[0];
    const int rows = f0.rows, cols = f0.cols, cn = f0.channels();
    micv_shim::require(f0.depth() == micv_shim::U8, "micv_ps7::getAllMHIsDevice: CV_8U frames expected");
    const size_t rb = (size_t)cols * cn, n = (size_t)rows * cols, V = items.size();
    std::vector<void *> blocks;  // freed on every way out
    struct Free {
        micv_ctx *ctx;
        std::vector<void *> &b;
        ~Free() {
            for (void *p : b) micv_device_free(ctx, p);
        }
    } guard{ctx, blocks};
    std::vector<const uint8_t *> dptr(V);
    for (size_t i = 0; i < V; i++) {
        const Video &vid = *items[i].vid;
        micv_shim::require(vid[0].type() == f0.type() && vid[0].rows == rows && vid[0].cols == cols,
                           "micv_ps7::getAllMHIsDevice: the videos differ in type or size");
        const size_t nf = (size_t)items[i].save + 1;  // the frames behind the last frame of action are never read
        const std::vector<uint8_t> buf = detail::packed(Video(vid.begin(), vid.begin() + nf), rb);
        void *p = nullptr;
        micv_shim::check(micv_device_malloc(ctx, buf.size(), &p));
        blocks.push_back(p);
        micv_shim::check(micv_memcpy2d_h2d(ctx, p, buf.size(), buf.data(), buf.size(), buf.size(), 1));
        dptr[i] = static_cast<const uint8_t *>(p);
    }
    void *dout = nullptr;
    micv_shim::check(micv_device_malloc(ctx, n * V, &dout));
    blocks.push_back(dout);
    std::vector<bool> done(V, false);
    for (size_t i0 = 0; i0 < V; i0++) {
        if (done[i0]) continue;
        std::vector<size_t> grp;  // the videos with i0's blur, in order
        for (size_t i = i0; i < V; i++)
            if (!done[i] && items[i].conf.pre_blur_size == items[i0].conf.pre_blur_size &&
                items[i].conf.pre_blur_sigma == items[i0].conf.pre_blur_sigma)
                grp.push_back(i);
        std::vector<const uint8_t *> fr;
        std::vector<int> nfr, tau, save;
        std::vector<double> thresh;
        for (size_t i : grp) {
            done[i] = true;
            fr.push_back(dptr[i]);
            nfr.push_back(items[i].save + 1);
            tau.push_back(items[i].conf.tau);
            save.push_back(items[i].save);
            thresh.push_back(items[i].conf.diff_threshold);
        }
        // a group's outputs are consecutive only when the group is; one plane at a time otherwise
        const bool run = grp.back() - grp.front() + 1 == grp.size();
        for (size_t g = 0; g < (run ? 1 : grp.size()); g++) {
            const int cnt = run ? (int)grp.size() : 1;
            micv_shim::check(micv_mhi_history_batch_dev(ctx, fr.data() + g, nfr.data() + g, rb * rows, rb, cnt, rows, cols, cn,
                                                        thresh.data() + g, tau.data() + g, save.data() + g,
                                                        items[i0].conf.pre_blur_size, items[i0].conf.pre_blur_size,
                                                        items[i0].conf.pre_blur_sigma,
                                                        static_cast<uint8_t *>(dout) + n * grp[g], n, cols, nullptr));
        }
    }
    std::vector<uint8_t> host(n * V);
    micv_shim::check(micv_memcpy2d_d2h(ctx, host.data(), host.size(), dout, host.size(), host.size(), 1));
    for (Mat &m : detail::planes(host, (int)V, rows, cols)) mhiFrames.push_back(m);
    for (const Item &it : items) {
        actions.push_back(it.action);
        people.push_back(it.person);
    }
}

}  // namespace micv_ps7
