// micv_ps6.hpp -- the ps6 driver (ProblemSets/ps6_cpp/src/Solution.cpp:16-107, pfDriver) without OpenCV, twice:
//   pfDriver         the reference's loop as written, on the shim's ParticleFilter: one synchronous tick per frame, the
//                    particles downloaded, ParticleFilter::drawParticles and micv_viz::rectangle on this thread.  With
//                    those two host loops it is the statement of the contract (parity with OpenCV's rasteriser unpinned);
//   pfDriverDevice   the same files from ONE library call (micv_ps6_track_display_seq_host): one upload per frame, no
//                    host synchronisation between ticks, a download of only the frames that are kept.
//   pfDriverGroupDevice  several such runs over one frame list from ONE library call on a filter group
//                    (micv_ps6_group_track_display_seq_host): the video uploaded once, every frame ticked for all runs in
//                    three launches, the same files as one pfDriverDevice call per run.
// Frames come from a std::vector<Mat> instead of cv::VideoCapture; pictures are written through micv_viz::imwrite
// (PGM / PPM instead of PNG).  Frames handed to the reference's video writer are appended to `video` when it is given.
#pragma once

#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include <unordered_set>
#include <vector>

#include "micv_config.hpp"
#include "micv_shim.hpp"
#include "micv_viz.hpp"

namespace micv_ps6 {

using micv_shim::Mat;
using micv_shim::Point2f;

struct Size2f {
    float width = 0, height = 0;
    Size2f() = default;
    Size2f(float w, float h) : width(w), height(h) {}
};

// cvRound as csrc/draw.hpp states it: half to even; INT_MIN for NaN, +-inf and every value outside int.
inline int cvRound(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return static_cast<int>(std::nearbyint(v));
}

// cv::Rect(cv::Rect_<float>(tl, size)): each of the four values through cvRound.
inline micv_viz::Rect toRect(const Point2f &tl, const Size2f &size) {
    return micv_viz::Rect(cvRound(tl.x), cvRound(tl.y), cvRound(size.width), cvRound(size.height));
}

// The driver's box around the estimate (Solution.cpp:76-78): the subtraction and the halving in float.
inline micv_viz::Rect boxRect(const Point2f &centre, const Size2f &size) {
    const Point2f bbox(centre.x - size.width / 2, centre.y - size.height / 2);
    return toRect(bbox, size);
}

// Config::Tracking (ps6_cpp/include/Config.h) with the frames in place of the capture.
struct Tracking {
    std::vector<Mat> frames;
    Point2f bbox;
    Size2f bboxSize;
};

inline const micv_shim::Scalar kDotColor(0, 255, 0, 0);     // Solution.cpp:74
inline const micv_viz::Scalar kBoxColor(255, 0, 255, 0);    // Solution.cpp:78

inline std::string framePath(const std::string &outputPrefix, int index, const Mat &frame, const std::string &ext) {
    return outputPrefix + "-f" + std::to_string(index) + (ext.empty() ? (frame.channels() == 3 ? ".ppm" : ".pgm") : ext);
}

// The painting of one pass of the loop (Solution.cpp:73-78): dots first, box second.
inline void paint(ParticleFilter &pf, Mat &frame, const Point2f &bboxCenter, const Size2f &bboxSize) {
    pf.drawParticles(frame, kDotColor);
    micv_viz::rectangle(frame, boxRect(bboxCenter, bboxSize), kBoxColor);
}

// pfDriver as written.  Every frame is painted in a clone, as the reference paints the capture's fresh frame; the model
// is a copy of frame 0 at cv::Rect(bbox, bboxSize), not a view (shim/micv_shim.hpp, ParticleFilter).
inline std::vector<micv_pf_state> pfDriver(const Tracking &tracking, const micv_config::PFConf &pfConf,
                                           const ParticleFilter::SimilarityMode simMode, const std::string &outputPrefix,
                                           const std::unordered_set<int> &saveFrames, std::vector<Mat> *video = nullptr,
                                           const std::string &ext = "") {
    std::unique_ptr<ParticleFilter> pf;
    std::vector<micv_pf_state> states;
    int numFrames = 0;
    for (const Mat &captured : tracking.frames) {
        Mat frame = captured.clone();
        if (!pf) {
            const micv_viz::Rect r = toRect(tracking.bbox, tracking.bboxSize);
            micv_shim::require(r.x >= 0 && r.y >= 0 && r.width > 0 && r.height > 0 && r.x + r.width <= frame.cols &&
                                   r.y + r.height <= frame.rows,
                               "pfDriver: the bounding box does not lie in the frame");
            Mat model(r.height, r.width, frame.type(), frame.ptr<unsigned char>(r.y) + (size_t)r.x * frame.channels(), frame.step);
            pf.reset(new ParticleFilter(model, frame.size(), pfConf.num_particles, simMode, pfConf.mse_sigma, pfConf.dynamics_sigma,
                                        tracking.bbox));
        }
        Point2f bboxCenter;
        float xVar, yVar;
        std::tie(bboxCenter, xVar, yVar) = pf->tick(frame);
        states.push_back(micv_pf_state{bboxCenter.x, bboxCenter.y, xVar, yVar, 0u});
        paint(*pf, frame, bboxCenter, tracking.bboxSize);
        if (video) video->push_back(frame);
        if (saveFrames.count(numFrames)) micv_viz::imwrite(framePath(outputPrefix, numFrames, frame, ext), frame);
        numFrames++;
    }
    return states;
}

// pfDriver through micv_ps6_track_display_seq_host.  Same files, same bytes, same states.
inline std::vector<micv_pf_state> pfDriverDevice(const Tracking &tracking, const micv_config::PFConf &pfConf,
                                                 const ParticleFilter::SimilarityMode simMode, const std::string &outputPrefix,
                                                 const std::unordered_set<int> &saveFrames, std::vector<Mat> *video = nullptr,
                                                 const std::string &ext = "") {
    micv_shim::require(!tracking.frames.empty(), "pfDriver: no frames");
    const Mat &f0 = tracking.frames[0];
    const int nframes = static_cast<int>(tracking.frames.size());
    std::vector<const uint8_t *> fp;
    for (const Mat &f : tracking.frames) {
        micv_shim::require(f.rows == f0.rows && f.cols == f0.cols && f.type() == f0.type() && f.step == f0.step,
                           "pfDriver: frames of one size, type and row pitch expected");
        fp.push_back(f.data);
    }
    const micv_viz::Rect r = toRect(tracking.bbox, tracking.bboxSize);
    micv_shim::require(f0.depth() == micv_shim::U8 && r.x >= 0 && r.y >= 0 && r.width > 0 && r.height > 0 && r.x + r.width <= f0.cols &&
                           r.y + r.height <= f0.rows,
                       "pfDriver: 8-bit frames expected, and a bounding box inside them");
    micv_pf *raw = nullptr;
    micv_shim::check(micv_pf_create(micv_shim::context(), f0.ptr<unsigned char>(r.y) + (size_t)r.x * f0.channels(), r.height, r.width, f0.step,
                                    f0.channels(), f0.rows, f0.cols, static_cast<int>(pfConf.num_particles), static_cast<int>(simMode),
                                    pfConf.mse_sigma, pfConf.dynamics_sigma, tracking.bbox.x, tracking.bbox.y, 0.1, 0, MICV_PF_DEFAULT_SEED,
                                    &raw));
    std::shared_ptr<micv_pf> pf(raw, micv_pf_destroy);
    std::vector<int> save;
    if (!video)
        for (int t = 0; t < nframes; t++)
            if (saveFrames.count(t)) save.push_back(t);
    const int nout = video ? nframes : static_cast<int>(save.size());
    std::vector<Mat> kept;
    std::vector<uint8_t *> out;
    for (int k = 0; k < nout; k++) {
        kept.emplace_back(f0.rows, f0.cols, f0.type());
        out.push_back(kept.back().data);
    }
    std::vector<micv_pf_state> states(nframes);
    micv_shim::check(micv_ps6_track_display_seq_host(pf.get(), fp.data(), nframes, f0.step, kDotColor.val, tracking.bboxSize.width,
                                                     tracking.bboxSize.height, kBoxColor.v, save.data(), static_cast<int>(save.size()),
                                                     video ? 1 : 0, out.data(), nout ? kept[0].step : 0, states.data()));
    for (int k = 0; k < nout; k++) {
        const int t = video ? k : save[k];
        if (video) video->push_back(kept[k]);
        if (saveFrames.count(t)) micv_viz::imwrite(framePath(outputPrefix, t, kept[k], ext), kept[k]);
    }
    return states;
}

// `count` pfDriverDevice runs over ONE frame list as one group (micv_ps6_group_track_display_seq_host): the frames of
// trackings[0] are the video (every other tracking must carry the same frames: count, size, type and bytes are checked, so
// runs over two videos are two calls), every tracking brings its own bounding box, and run k writes under prefixes[k] the files
// that pfDriverDevice(trackings[k], confs[k], modes[k], prefixes[k], saveSets[k]) writes.  -> the states of each run.
inline std::vector<std::vector<micv_pf_state>> pfDriverGroupDevice(const std::vector<Tracking> &trackings,
                                                                   const std::vector<micv_config::PFConf> &confs,
                                                                   const std::vector<ParticleFilter::SimilarityMode> &modes,
                                                                   const std::vector<std::string> &prefixes,
                                                                   const std::vector<std::unordered_set<int>> &saveSets,
                                                                   const std::string &ext = "") {
    const size_t count = trackings.size();
    micv_shim::require(count >= 1 && confs.size() == count && modes.size() == count && prefixes.size() == count && saveSets.size() == count,
                       "pfDriverGroup: one configuration, mode, prefix and save set per tracking expected");
    const std::vector<Mat> &video = trackings[0].frames;
    micv_shim::require(!video.empty(), "pfDriver: no frames");
    const Mat &f0 = video[0];
    const int nframes = static_cast<int>(video.size());
    std::vector<const uint8_t *> fp;
    for (const Mat &f : video) {
        micv_shim::require(f.rows == f0.rows && f.cols == f0.cols && f.type() == f0.type() && f.step == f0.step,
                           "pfDriver: frames of one size, type and row pitch expected");
        fp.push_back(f.data);
    }
    // one video: a tracking that brings other frames (another video, another length or size) is a mistake, not a request
    for (size_t k = 1; k < count; k++) {
        const std::vector<Mat> &other = trackings[k].frames;
        micv_shim::require(other.size() == video.size(), "pfDriverGroup: every tracking must carry the frames of trackings[0]");
        for (size_t t = 0; t < other.size(); t++) {
            const Mat &a = other[t], &b = video[t];
            bool same = a.rows == b.rows && a.cols == b.cols && a.type() == b.type();
            for (int r = 0; same && a.data != b.data && r < b.rows; r++)
                same = std::memcmp(a.data + (size_t)r * a.step, b.data + (size_t)r * b.step, (size_t)b.cols * b.elemSize()) == 0;
            micv_shim::require(same, "pfDriverGroup: every tracking must carry the frames of trackings[0] (one group per video)");
        }
    }
    std::vector<std::shared_ptr<micv_pf>> filters;
    std::vector<micv_pf *> members;
    std::vector<float> bboxWH;
    for (size_t k = 0; k < count; k++) {
        const Tracking &tr = trackings[k];
        const micv_viz::Rect r = toRect(tr.bbox, tr.bboxSize);
        micv_shim::require(f0.depth() == micv_shim::U8 && r.x >= 0 && r.y >= 0 && r.width > 0 && r.height > 0 && r.x + r.width <= f0.cols &&
                               r.y + r.height <= f0.rows,
                           "pfDriver: 8-bit frames expected, and a bounding box inside them");
        micv_pf *raw = nullptr;
        micv_shim::check(micv_pf_create(micv_shim::context(), f0.ptr<unsigned char>(r.y) + (size_t)r.x * f0.channels(), r.height, r.width,
                                        f0.step, f0.channels(), f0.rows, f0.cols, static_cast<int>(confs[k].num_particles),
                                        static_cast<int>(modes[k]), confs[k].mse_sigma, confs[k].dynamics_sigma, tr.bbox.x, tr.bbox.y, 0.1,
                                        0, MICV_PF_DEFAULT_SEED, &raw));
        filters.emplace_back(raw, micv_pf_destroy);
        members.push_back(raw);
        bboxWH.push_back(tr.bboxSize.width);
        bboxWH.push_back(tr.bboxSize.height);
    }
    micv_pf_group *rawGroup = nullptr;
    micv_shim::check(micv_pf_group_create(members.data(), static_cast<int>(count), &rawGroup));
    std::shared_ptr<micv_pf_group> group(rawGroup, micv_pf_group_destroy);  // declared after the filters: destroyed first
    std::vector<std::vector<int>> save(count);
    std::vector<std::vector<Mat>> kept(count);
    std::vector<std::vector<uint8_t *>> out(count);
    std::vector<const int *> savePtr;
    std::vector<uint8_t *const *> outPtr;
    std::vector<int> nsave;
    size_t ostride = 0;
    for (size_t k = 0; k < count; k++) {
        for (int t = 0; t < nframes; t++)
            if (saveSets[k].count(t)) save[k].push_back(t);
        kept[k].reserve(save[k].size());
        for (size_t j = 0; j < save[k].size(); j++) {
            kept[k].emplace_back(f0.rows, f0.cols, f0.type());
            ostride = kept[k].back().step;
            out[k].push_back(kept[k].back().data);
        }
        savePtr.push_back(save[k].data());
        outPtr.push_back(out[k].data());
        nsave.push_back(static_cast<int>(save[k].size()));
    }
    std::vector<micv_pf_state> flat((size_t)nframes * count);
    micv_shim::check(micv_ps6_group_track_display_seq_host(group.get(), fp.data(), nframes, f0.step, kDotColor.val, bboxWH.data(),
                                                           kBoxColor.v, savePtr.data(), nsave.data(), 0, outPtr.data(),
                                                           ostride, flat.data()));
    std::vector<std::vector<micv_pf_state>> states(count, std::vector<micv_pf_state>(nframes));
    for (size_t k = 0; k < count; k++) {
        for (int t = 0; t < nframes; t++) states[k][t] = flat[(size_t)t * count + k];
        for (size_t j = 0; j < save[k].size(); j++) micv_viz::imwrite(framePath(prefixes[k], save[k][j], kept[k][j], ext), kept[k][j]);
    }
    return states;
}

}  // namespace micv_ps6
