// micv_shim.hpp -- header-only drop-in for the reference's cv::Mat-in / cv::Mat-out functions,
// implemented on the C ABI of libmicv.so (include/mi_cv.h).
//
// Same namespaces, names, argument order, defaults and ownership rules as the reference:
//   lk::      ProblemSets/ps5_cpp/include/OpticalFlow.h:5-19
//   pyr::     ProblemSets/ps5_cpp/include/Pyramids.h:7-12
//   harris::  ProblemSets/ps4_cpp/include/Harris.h:18-96   (cpu:: and gpu:: are the same code here)
//   sift::    ProblemSets/ps4_cpp/include/Descriptors.h:8-23
//   ransac::  ProblemSets/ps4_cpp/include/RANSAC.h:10-28
//   ParticleFilter  ProblemSets/ps6_cpp/include/ParticleFilter.h (the class, in the global namespace)
//   cuda:: / serial::  ps2_cpp/include/DisparitySSD.h:18-43, DisparityNCorr.h:19-44,
//                      ps1_cpp/src/Hough.h:22-84
//   mhi::, moments::, matching::  ps7_cpp/include/{MotionHistory,Moments,Matching}.h
// Inputs are const references and never retained; outputs are (re)allocated by the callee like
// the reference does (Mat::create / assignment of a fresh Mat).  Errors: the reference asserts or
// exit(-1)s (CudaCommon.cuh:13-22); the shim throws std::runtime_error carrying micv_last_error().
//
// With -DMICV_SHIM_WITH_OPENCV the functions take real cv::Mat / cv::KeyPoint; without it they
// take the minimal micv::Mat of micv_mat.hpp (this image has no OpenCV).
#pragma once

#include <cmath>
#include <cstring>
#include <fstream>
#include <algorithm>
#include <cstdio>
#include <functional>
#include <iostream>
#include <memory>
#include <random>
#include <stdexcept>
#include <tuple>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mi_cv.h"

#ifdef MICV_SHIM_WITH_OPENCV
#include <opencv2/core/core.hpp>
#include <opencv2/core/cuda.hpp>
#include <opencv2/core/types.hpp>
#include <opencv2/imgproc/imgproc.hpp>
namespace micv_shim {
using Mat = cv::Mat;
using KeyPoint = cv::KeyPoint;
using Point2f = cv::Point2f;
using Size = cv::Size;
using Scalar = cv::Scalar;
// cv::cuda::GpuMat's data pointer must be memory this library's device can address (an OpenCV
// built against HIP, or unified memory); the overloads below only pass it through.
using GpuMat = cv::cuda::GpuMat;
enum { F32 = CV_32F, S8 = CV_8S, U8 = CV_8U, S32 = CV_32S, U8C3 = CV_8UC3 };
inline micv_ctx *context() {  // one context per thread, like the reference's per-call streams
    thread_local micv_ctx *ctx = nullptr;
    if (!ctx && micv_ctx_create(0, &ctx) != MICV_OK)
        throw std::runtime_error(std::string("micv: ") + micv_last_error());
    return ctx;
}
inline void create_continuous(GpuMat &m, int rows, int cols, int type) { cv::cuda::createContinuous(rows, cols, type, m); }
}  // namespace micv_shim
#else
#include "micv_mat.hpp"
namespace micv_shim {
using Mat = micv::Mat;
using KeyPoint = micv::KeyPoint;
using Point2f = micv::Point2f;
using Size = micv::Size;
using Scalar = micv::Scalar;
using GpuMat = micv::GpuMat;
enum { F32 = micv::CV_32F, S8 = micv::CV_8S, U8 = micv::CV_8U, S32 = micv::CV_32S, U8C3 = micv::CV_8UC3 };
inline micv_ctx *context() { return micv::thread_context(); }
inline void create_continuous(GpuMat &m, int rows, int cols, int type) { m.create(rows, cols, type); }
}  // namespace micv_shim
#endif

namespace micv_shim {

// The reference's kernel-timing log lines (ps4_cpp/lib/Harris.cu:155,290, ps2_cpp/lib/DisparitySSD.cu:203,
// DisparityNCorr.cu:247, ps1_cpp/src/Hough.cu:289,345,391, ps5_cpp/lib/Pyramids.cu:69,123):
//     micv_shim::log_kernel_times_to([](const std::string &line) { spdlog::get("file_logger")->info(line); });
// makes every shim call of those functions emit "<kernel> execution took <ms> ms" ("<kernel> took <ms> ms"
// for the two pyramid kernels, as the reference words them) through the given sink; an empty function
// removes it.  One sink per process (the drivers log from their main thread only).
inline std::function<void(const std::string &)> &kernel_log_sink() {
    static std::function<void(const std::string &)> sink;
    return sink;
}
inline void log_kernel_times_to(std::function<void(const std::string &)> sink) {
    kernel_log_sink() = std::move(sink);
    if (!kernel_log_sink()) {
        micv_set_kernel_log(nullptr, nullptr);
        return;
    }
    micv_set_kernel_log(
        [](const char *kernel, float ms, void *) {
            const std::string k(kernel);
            const bool pyr = k.compare(0, 3, "pyr") == 0;
            if (kernel_log_sink()) kernel_log_sink()(k + (pyr ? " took " : " execution took ") + std::to_string(ms) + " ms");
        },
        nullptr);
}

inline void check(int rc) {
    if (rc != MICV_OK) throw std::runtime_error(std::string("micv: ") + micv_last_error());
}
inline void require(bool ok, const char *what) {
    if (!ok) throw std::invalid_argument(what);
}
// Multi-GPU (include/mi_cv.h, "multi-GPU"): one process per GPU.  With a communicator set, lk::calcOpticalFlowPyr on
// CV_32F frames splits every call by rows over the ranks (each computes its band, the coarse-flow halo travels over
// RCCL, the bands are gathered) and still returns whole fields -- the reference's caller (ps5_cpp/src/Solution.cpp:
// 60-64) does not change.  Rank 0 makes the id (micv_comm_unique_id) and ships its MICV_COMM_ID_BYTES bytes to the
// others by whatever the application has (MPI, a file); every rank then calls init_comm(id, rank, world) --
// collective -- or use_comm() with an ncclComm_t / micv_comm it already owns.
inline micv_comm *&comm_slot() {
    static micv_comm *c = nullptr;
    return c;
}
inline void use_comm(micv_comm *c) { comm_slot() = c; }
inline void init_comm(const void *unique_id, int rank, int world) {
    micv_comm *c = nullptr;
    check(micv_comm_create(context(), nullptr, unique_id, rank, world, &c));
    comm_slot() = c;
    check(micv_comm_selftest(context(), c, nullptr));  // a broken fabric is reported here, not as a wrong flow later
}
inline void close_comm() {
    if (comm_slot()) micv_comm_destroy(comm_slot());
    comm_slot() = nullptr;
}
inline bool frame_type_ok(const Mat &m) {  // what cvtColor(COLOR_RGB2GRAY) + convertTo(CV_32F) take here
    return (m.depth() == U8 || m.depth() == F32) && (m.channels() == 1 || m.channels() == 3 || m.channels() == 4);
}
inline int depth_code(const Mat &m) { return m.depth() == U8 ? MICV_DEPTH_8U : MICV_DEPTH_32F; }
// The reference converts its inputs itself: pyr::makeGaussianPyramid runs
// cv::cvtColor(COLOR_RGB2GRAY) on multi-channel frames and convertTo(CV_32F) (Pyramids.cpp:9-15),
// lk::calcOpticalFlow convertTo(CV_32F) (OpticalFlow.cpp:51-52).  Single-channel CV_32F passes
// through untouched; everything else goes through micv_to_gray_f32_host.
inline Mat to_f32(const Mat &m) {
    if (m.type() == F32) return m;
    require(frame_type_ok(m), "micv shim: 1/3/4-channel CV_8U or CV_32F input expected");
    Mat f(m.rows, m.cols, F32);
    check(micv_to_gray_f32_host(context(), m.data, m.rows, m.cols, m.step, m.channels(), depth_code(m),
                                f.ptr<float>(), f.step));
    return f;
}

}  // namespace micv_shim

namespace lk {
using micv_shim::Mat;

inline void calcOpticalFlow(const Mat &prevImg, const Mat &nextImg, Mat &u, Mat &v,
                            const size_t winSize = 21) {
    micv_shim::require(prevImg.rows == nextImg.rows && prevImg.cols == nextImg.cols &&
                           prevImg.type() == nextImg.type(),
                       "lk::calcOpticalFlow: size/type mismatch");  // OpticalFlow.cpp:47
    micv_shim::require(winSize % 2 == 1, "lk::calcOpticalFlow: winSize must be odd");  // :48
    const Mat p = micv_shim::to_f32(prevImg), n = micv_shim::to_f32(nextImg);
    micv_shim::require(p.step == n.step, "lk::calcOpticalFlow: inputs need equal row pitch");
    u.create(p.rows, p.cols, micv_shim::F32);  // :53-54
    v.create(p.rows, p.cols, micv_shim::F32);
    micv_shim::check(micv_lk_flow_host(micv_shim::context(), p.ptr<float>(), n.ptr<float>(), p.rows,
                                       p.cols, p.step, static_cast<int>(winSize), u.ptr<float>(),
                                       v.ptr<float>(), u.step));
}

inline void warp(const Mat &src, const Mat &du, const Mat &dv, Mat &dst) {
    micv_shim::require(du.rows == dv.rows && du.cols == dv.cols && src.rows == du.rows &&
                           src.cols == du.cols,
                       "lk::warp: size mismatch");  // OpticalFlow.cpp:107
    micv_shim::require(du.type() == micv_shim::F32 && dv.type() == micv_shim::F32 &&
                           src.type() == micv_shim::F32 && du.step == dv.step,
                       "lk::warp: CV_32F expected");  // :108
    Mat out(src.rows, src.cols, micv_shim::F32);
    micv_shim::check(micv_lk_warp_host(micv_shim::context(), src.ptr<float>(), src.step,
                                       du.ptr<float>(), dv.ptr<float>(), du.step, src.rows, src.cols,
                                       out.ptr<float>(), out.step));
    dst = out;
}

// An extension, not a reference function: the pyramid depth the reference hard-codes (pyrDepth = 4,
// OpticalFlow.cpp:127) as a parameter.  lk::calcOpticalFlowPyr below has the reference's exact type
// (tests/cpp/shim_signatures.cpp) and calls this with 4.
inline void calcOpticalFlowPyrLevels(const Mat &prevImg, const Mat &nextImg, Mat &u, Mat &v,
                                     const size_t winSize, const size_t levels) {
    micv_shim::require(prevImg.rows == nextImg.rows && prevImg.cols == nextImg.cols,
                       "lk::calcOpticalFlowPyr: size mismatch");
    Mat uu(prevImg.rows, prevImg.cols, micv_shim::F32), vv(prevImg.rows, prevImg.cols, micv_shim::F32);
    if (prevImg.type() == nextImg.type() && prevImg.type() != micv_shim::F32 && prevImg.step == nextImg.step) {
        // the ps5 driver's call (Solution.cpp:63): colour and/or 8-bit frames, converted by
        // makeGaussianPyramid (Pyramids.cpp:9-15) -- one upload, conversion on the device
        micv_shim::require(micv_shim::frame_type_ok(prevImg),
                           "lk::calcOpticalFlowPyr: 1/3/4-channel CV_8U or CV_32F frames expected");
        micv_shim::check(micv_lk_flow_pyr_frames_host(
            micv_shim::context(), prevImg.data, nextImg.data, prevImg.rows, prevImg.cols, prevImg.step,
            prevImg.channels(), micv_shim::depth_code(prevImg), static_cast<int>(winSize),
            static_cast<int>(levels), uu.ptr<float>(), vv.ptr<float>(), uu.step));
        u = uu;
        v = vv;
        return;
    }
    const Mat p = micv_shim::to_f32(prevImg), n = micv_shim::to_f32(nextImg);
    micv_shim::require(p.step == n.step, "lk::calcOpticalFlowPyr: inputs need equal row pitch");
    if (micv_shim::comm_slot())  // row-sharded over the ranks of the communicator, whole fields on every rank
        micv_shim::check(micv_lk_flow_pyr_rowshard_host(micv_shim::context(), micv_shim::comm_slot(), p.ptr<float>(),
                                                        n.ptr<float>(), p.rows, p.cols, p.step, static_cast<int>(winSize),
                                                        static_cast<int>(levels), uu.ptr<float>(), vv.ptr<float>(), uu.step));
    else
        micv_shim::check(micv_lk_flow_pyr_host(micv_shim::context(), p.ptr<float>(), n.ptr<float>(),
                                               p.rows, p.cols, p.step, static_cast<int>(winSize),
                                               static_cast<int>(levels), uu.ptr<float>(),
                                               vv.ptr<float>(), uu.step));
    u = uu;  // :165-166
    v = vv;
}
// ps5_cpp/include/OpticalFlow.h:14-18
inline void calcOpticalFlowPyr(const Mat &prevImg, const Mat &nextImg, Mat &u, Mat &v, const size_t winSize = 21) {
    calcOpticalFlowPyrLevels(prevImg, nextImg, u, v, winSize, 4);
}
// An extension for the driver's frame loops (ps5_cpp/src/Solution.cpp:255-285: pairs (0, 1), (1, 2), ... of the frames
// Config.cpp:17-46 loaded from a directory): the same flows as calling lk::calcOpticalFlowPyr pair by pair, with every
// frame uploaded once and transfers overlapped with the chains (micv_lk_flow_seq_host).  u[p], v[p]: pair (p, p + 1).
inline void calcOpticalFlowPyrSequence(const std::vector<Mat> &frames, std::vector<Mat> &u, std::vector<Mat> &v,
                                       const size_t winSize = 21, const size_t levels = 4) {
    micv_shim::require(frames.size() >= 2, "lk::calcOpticalFlowPyrSequence: at least two frames expected");
    const Mat &f0 = frames[0];
    micv_shim::require(micv_shim::frame_type_ok(f0), "lk::calcOpticalFlowPyrSequence: 1/3/4-channel CV_8U or CV_32F frames expected");
    std::vector<const void *> fp;
    for (const Mat &f : frames) {
        micv_shim::require(f.rows == f0.rows && f.cols == f0.cols && f.type() == f0.type() && f.step == f0.step,
                           "lk::calcOpticalFlowPyrSequence: frames of one size, type and row pitch expected");
        fp.push_back(f.data);
    }
    const size_t n = frames.size() - 1;
    std::vector<Mat> uu, vv;
    std::vector<float *> up, vp;
    for (size_t p = 0; p < n; p++) {
        uu.emplace_back(f0.rows, f0.cols, micv_shim::F32);
        vv.emplace_back(f0.rows, f0.cols, micv_shim::F32);
        up.push_back(uu.back().ptr<float>());
        vp.push_back(vv.back().ptr<float>());
    }
    micv_shim::check(micv_lk_flow_seq_host(micv_shim::context(), fp.data(), static_cast<int>(frames.size()), f0.rows, f0.cols,
                                           f0.step, f0.channels(), micv_shim::depth_code(f0), static_cast<int>(winSize),
                                           static_cast<int>(levels), up.data(), vp.data(), uu[0].step));
    u = uu;
    v = vv;
}
}  // namespace lk

namespace pyr {
using micv_shim::Mat;

inline void pyrDown(const Mat &src, Mat &dst) {
    micv_shim::require(src.type() == micv_shim::F32, "pyr::pyrDown: CV_32F expected");  // Pyramids.cu:35
    Mat out(src.rows / 2, src.cols / 2, micv_shim::F32);
    micv_shim::check(micv_pyr_down_host(micv_shim::context(), src.ptr<float>(), src.rows, src.cols,
                                        src.step, out.ptr<float>(), out.step));
    dst = out;
}
inline void pyrUp(const Mat &src, Mat &dst) {
    micv_shim::require(src.type() == micv_shim::F32, "pyr::pyrUp: CV_32F expected");  // Pyramids.cu:95
    Mat out(src.rows * 2, src.cols * 2, micv_shim::F32);  // may alias src: written after the read
    micv_shim::check(micv_pyr_up_host(micv_shim::context(), src.ptr<float>(), src.rows, src.cols,
                                      src.step, out.ptr<float>(), out.step));
    dst = out;
}
inline std::vector<Mat> makeGaussianPyramid(const Mat &src, const size_t levels) {
    const Mat grey = micv_shim::to_f32(src);  // Pyramids.cpp:9-15: cvtColor(RGB2GRAY) if colour, convertTo(CV_32F)
    std::vector<Mat> pyramid;
    std::vector<float *> ptrs;
    for (size_t l = 0; l < levels; l++) {
        pyramid.emplace_back(grey.rows >> l, grey.cols >> l, micv_shim::F32);
        ptrs.push_back(pyramid.back().ptr<float>());
    }
    micv_shim::check(micv_gaussian_pyramid_host(micv_shim::context(), grey.ptr<float>(), grey.rows,
                                                grey.cols, grey.step, static_cast<int>(levels),
                                                ptrs.data()));
    return pyramid;
}
}  // namespace pyr

namespace harris {
using micv_shim::Mat;

inline void getGradients(const Mat &in, int kernelSize, Mat &diffX, Mat &diffY) {
    micv_shim::require(kernelSize == 1 || kernelSize == 3 || kernelSize == 5 || kernelSize == 7,
                       "harris::getGradients: kernelSize must be 1, 3, 5 or 7");  // Harris.cpp:16
    micv_shim::require(in.type() == micv_shim::F32, "harris::getGradients: CV_32F expected");  // :17
    diffX.create(in.rows, in.cols, micv_shim::F32);
    diffY.create(in.rows, in.cols, micv_shim::F32);
    micv_shim::check(micv_sobel_host(micv_shim::context(), in.ptr<float>(), in.rows, in.cols, in.step,
                                     kernelSize, 1.f, diffX.ptr<float>(), diffY.ptr<float>(),
                                     diffX.step));
}

namespace detail {
inline void response(const Mat &gradX, const Mat &gradY, const size_t windowSize,
                     const double gaussianSigma, const float harrisScore, Mat &cornerResponse, int flags) {
    micv_shim::require(gradX.rows == gradY.rows && gradX.cols == gradY.cols &&
                           gradX.type() == micv_shim::F32 && gradY.type() == micv_shim::F32 &&
                           gradX.step == gradY.step,
                       "harris::getCornerResponse: gradient mismatch");  // Harris.cpp:49-50
    micv_shim::require(windowSize % 2 == 1, "harris::getCornerResponse: windowSize must be odd");
    Mat out(gradX.rows, gradX.cols, micv_shim::F32);
    micv_shim::check(micv_harris_response_ex_host(micv_shim::context(), gradX.ptr<float>(),
                                                  gradY.ptr<float>(), gradX.rows, gradX.cols, gradX.step,
                                                  static_cast<int>(windowSize), gaussianSigma,
                                                  harrisScore, flags, out.ptr<float>(), out.step));
    cornerResponse = out;
}
inline void refine(const Mat &cornerResponse, const double threshold, const int minDistance,
                   Mat &corners, std::vector<std::pair<int, int>> &cornerLocs, bool append) {
    micv_shim::require(cornerResponse.type() == micv_shim::F32,
                       "harris::refineCorners: CV_32F expected");  // Harris.cpp:105
    Mat out(cornerResponse.rows, cornerResponse.cols, micv_shim::F32);
    const int64_t cap = static_cast<int64_t>(cornerResponse.rows) * cornerResponse.cols;
    std::vector<int32_t> locs(static_cast<size_t>(cap) * 2);
    int64_t n = 0;
    micv_shim::check(micv_harris_refine_host(micv_shim::context(), cornerResponse.ptr<float>(),
                                             cornerResponse.rows, cornerResponse.cols,
                                             cornerResponse.step, threshold, minDistance,
                                             out.ptr<float>(), out.step, locs.data(), cap, &n));
    corners = out;
    if (!append) cornerLocs.clear();  // gpu:: resizes (Harris.cu:324), cpu:: appends (Harris.cpp:138)
    for (int64_t i = 0; i < n; i++) cornerLocs.emplace_back(locs[2 * i], locs[2 * i + 1]);
}
}  // namespace detail

namespace cpu {
// harris::cpu's own arithmetic (Harris.cpp:78-92: unfused accumulation, double determinant, one rounding),
// computed on the GPU: MICV_HARRIS_CPU.  -DMICV_SHIM_HARRIS_CPU_AS_GPU=1 routes it to harris::gpu's instead.
inline void getCornerResponse(const Mat &gradX, const Mat &gradY, const size_t windowSize,
                              const double gaussianSigma, const float harrisScore,
                              Mat &cornerResponse) {
#if defined(MICV_SHIM_HARRIS_CPU_AS_GPU) && MICV_SHIM_HARRIS_CPU_AS_GPU
    detail::response(gradX, gradY, windowSize, gaussianSigma, harrisScore, cornerResponse, 0);
#else
    detail::response(gradX, gradY, windowSize, gaussianSigma, harrisScore, cornerResponse, MICV_HARRIS_CPU);
#endif
}
inline void refineCorners(const Mat &cornerResponse, const double threshold, const int minDistance,
                          Mat &corners, std::vector<std::pair<int, int>> &cornerLocs) {
    detail::refine(cornerResponse, threshold, minDistance, corners, cornerLocs, true);
}
}  // namespace cpu
namespace gpu {
inline void getCornerResponse(const Mat &gradX, const Mat &gradY, const size_t windowSize,
                              const double gaussianSigma, const float harrisScore,
                              Mat &cornerResponse) {
    detail::response(gradX, gradY, windowSize, gaussianSigma, harrisScore, cornerResponse, 0);
}
inline void refineCorners(const Mat &cornerResponse, const double threshold, const int minDistance,
                          Mat &corners, std::vector<std::pair<int, int>> &cornerLocs) {
    detail::refine(cornerResponse, threshold, minDistance, corners, cornerLocs, false);
}
}  // namespace gpu
}  // namespace harris

namespace sift {
using micv_shim::KeyPoint;
using micv_shim::Mat;

inline void getAnglesFromGradients(const Mat &gradX, const Mat &gradY, Mat &angles) {
    micv_shim::require(gradX.rows == gradY.rows && gradX.cols == gradY.cols &&
                           gradX.type() == micv_shim::F32 && gradY.type() == micv_shim::F32 &&
                           gradX.step == gradY.step,
                       "sift::getAnglesFromGradients: gradient mismatch");  // Descriptors.cpp:9-10
    angles.create(gradX.rows, gradX.cols, micv_shim::F32);
    micv_shim::check(micv_sift_angles_host(micv_shim::context(), gradX.ptr<float>(),
                                           gradY.ptr<float>(), gradX.rows, gradX.cols, gradX.step,
                                           angles.ptr<float>(), angles.step));
}
inline void getKeypoints(const Mat &gradX, const Mat &gradY,
                         const std::vector<std::pair<int, int>> &cornerLocs, const size_t size,
                         std::vector<KeyPoint> &keypoints) {
    keypoints.clear();  // Descriptors.cpp:36
    std::vector<int32_t> locs;
    for (const auto &c : cornerLocs) {
        locs.push_back(c.first);
        locs.push_back(c.second);
    }
    std::vector<float> kp(cornerLocs.size() * 4);
    micv_shim::check(micv_sift_keypoints_host(micv_shim::context(), gradX.ptr<float>(),
                                              gradY.ptr<float>(), gradX.rows, gradX.cols, gradX.step,
                                              locs.data(), static_cast<int64_t>(cornerLocs.size()),
                                              static_cast<float>(size), kp.data()));
    for (size_t i = 0; i < cornerLocs.size(); i++)
        keypoints.emplace_back(kp[4 * i], kp[4 * i + 1], kp[4 * i + 2], kp[4 * i + 3], 0.f);  // :45
}
// The descriptor step of Solution::siftHelper (ps4_cpp/src/Solution.cpp:166-169): where the
// reference calls cv::xfeatures2d::SIFT::compute(img, keypoints, descriptors), a build without
// opencv_contrib calls this on the gradient fields it already has.  descriptors: CV_32F, one row of
// 128 values per keypoint (the layout of OpenCV's SIFT output, ready for the BFMatcher step).
inline void computeDescriptors(const Mat &gradX, const Mat &gradY, const std::vector<KeyPoint> &keypoints,
                               Mat &descriptors) {
    micv_shim::require(gradX.rows == gradY.rows && gradX.cols == gradY.cols &&
                           gradX.type() == micv_shim::F32 && gradY.type() == micv_shim::F32 &&
                           gradX.step == gradY.step,
                       "sift::computeDescriptors: gradient mismatch");
    std::vector<float> kp(keypoints.size() * 4);
    for (size_t i = 0; i < keypoints.size(); i++) {
        kp[4 * i] = keypoints[i].pt.x;
        kp[4 * i + 1] = keypoints[i].pt.y;
        kp[4 * i + 2] = keypoints[i].size;
        kp[4 * i + 3] = keypoints[i].angle;
    }
    Mat out(static_cast<int>(keypoints.size()), 128, micv_shim::F32);
    if (!keypoints.empty())
        micv_shim::check(micv_sift_descriptors_host(micv_shim::context(), gradX.ptr<float>(), gradY.ptr<float>(),
                                                    gradX.rows, gradX.cols, gradX.step, kp.data(),
                                                    static_cast<int64_t>(keypoints.size()), out.ptr<float>(),
                                                    out.step));
    descriptors = out;
}
}  // namespace sift

namespace ransac {  // ProblemSets/ps4_cpp/include/RANSAC.h:10-28, RANSAC.cpp:11-152
using micv_shim::Mat;
using micv_shim::Point2f;
enum class TransformType { TRANSLATION = 1, SIMILARITY = 2, AFFINE = 3 };
namespace detail {
// The file-static engine and `seeded` flag of RANSAC.cpp:12-13 (one per process).
inline micv_ransac_rng *&engine() {
    static micv_ransac_rng *rng = nullptr;
    if (!rng) micv_shim::check(micv_ransac_rng_create(nullptr, 0, &rng));  // `static std::mt19937 rng;`
    return rng;
}
inline bool &seeded() {
    static bool s = false;
    return s;
}
}  // namespace detail

// Seeds the engine from the seed sequence's words; every later call is ignored (RANSAC.cpp:20-25).
inline void seed(std::shared_ptr<std::seed_seq> seq) {
    if (detail::seeded()) return;
    std::vector<uint32_t> words(seq->size());
    seq->param(words.begin());
    micv_ransac_rng *rng = nullptr;
    micv_shim::check(micv_ransac_rng_create(words.data(), static_cast<int>(words.size()), &rng));
    micv_ransac_rng_destroy(detail::engine());
    detail::engine() = rng;
    detail::seeded() = true;
}

// ransac::solve as written: the LAST iteration's transform (an empty Mat when none ran), the best
// iteration's consensus positions, its ratio; "RANSAC took {} iterations" goes to the kernel-log sink
// (RANSAC.cpp:148-149).  The reference asserts equal sizes (:34).
inline std::tuple<Mat, std::vector<int>, double> solve(const std::vector<Point2f> &srcPts,
                                                       const std::vector<Point2f> &destPts,
                                                       const TransformType whichTransform,
                                                       const int ransacReprojThresh = 3, const int maxIters = 2000,
                                                       const double minConsensusRatio = 0.75) {
    micv_shim::require(srcPts.size() == destPts.size(), "ransac::solve: point lists of different sizes");
    const int k = static_cast<int>(whichTransform);
    const int64_t n = static_cast<int64_t>(srcPts.size());
    micv_shim::require(n >= k && maxIters >= 1, "ransac::solve: fewer points than the sample, or maxIters < 1");
    std::vector<float> src(2 * n), dst(2 * n);
    for (int64_t i = 0; i < n; i++) {
        src[2 * i] = srcPts[i].x;
        src[2 * i + 1] = srcPts[i].y;
        dst[2 * i] = destPts[i].x;
        dst[2 * i + 1] = destPts[i].y;
    }
    micv_ransac_rng *rng = detail::engine();
    std::vector<int32_t> samples((size_t)maxIters * k);
    micv_shim::check(micv_ransac_rng_samples(rng, n, k, maxIters, samples.data()));
    float tr[12];
    std::vector<uint8_t> mask(n);
    int32_t stats[3];
    micv_shim::check(micv_ransac_solve_host(micv_shim::context(), src.data(), dst.data(), n, samples.data(), maxIters,
                                            k, ransacReprojThresh, minConsensusRatio, tr, mask.data(), stats));
    std::vector<int> consensusSet;
    if (stats[2] > 0) {
        std::vector<int32_t> perm(n);
        micv_shim::check(micv_ransac_rng_permutation(rng, n, stats[1], perm.data()));
        for (int64_t p = k; p < n; p++)
            if (mask[perm[p]]) consensusSet.push_back(static_cast<int>(p));
    }
    micv_shim::check(micv_ransac_rng_advance(rng, n, stats[0]));
    if (micv_shim::kernel_log_sink())
        micv_shim::kernel_log_sink()("RANSAC took " + std::to_string(stats[0]) + " iterations");
    Mat transform;
    if (stats[0] > 0) {
        transform.create(2, 3, micv_shim::F32);
        for (int r = 0; r < 2; r++) std::memcpy(transform.ptr<float>(r), tr + 3 * r, 12);
    }
    return std::make_tuple(transform, consensusSet, stats[2] > 0 ? double(stats[2]) / double(n) : 0.0);
}
}  // namespace ransac

// ParticleFilter, ProblemSets/ps6_cpp/include/ParticleFilter.h and lib/ParticleFilter.cpp, on micv_pf_* (the
// arithmetic of mi_cv.h's "ps6: particle filter" block).  The model (8-bit, 1 or 3 channels) is copied: the
// reference keeps a view into the caller's frame, into which its driver then paints.  Errors throw
// std::runtime_error (the reference asserts or divides by zero).
class ParticleFilter {
public:
    enum class SimilarityMode { MEAN_SQ_ERR, MEAN_SHIFT_LT };
    ParticleFilter(const micv_shim::Mat &model,
                   const micv_shim::Size &imSize,
                   const size_t numParticles,
                   const SimilarityMode simMode,
                   const double mseSigma,
                   const double sampleSigma,
                   const micv_shim::Point2f &initModelPos = micv_shim::Point2f(-1, -1),
                   const double alpha = 0.1)
        : _imSize(imSize), _numParticles(numParticles) {
        micv_shim::require(model.depth() == micv_shim::U8 && (model.channels() == 1 || model.channels() == 3),
                           "ParticleFilter: the model must be 8-bit with 1 or 3 channels");
        micv_shim::require(numParticles >= 1 && numParticles <= MICV_PF_MAX_PARTICLES,
                           "ParticleFilter: numParticles outside 1 .. MICV_PF_MAX_PARTICLES");
        micv_pf *pf = nullptr;
        micv_shim::check(micv_pf_create(micv_shim::context(), model.data, model.rows, model.cols,
                                        static_cast<size_t>(model.step), model.channels(), imSize.height, imSize.width,
                                        static_cast<int>(numParticles), static_cast<int>(simMode), mseSigma,
                                        sampleSigma, initModelPos.x, initModelPos.y, alpha, 0, MICV_PF_DEFAULT_SEED,
                                        &pf));
        _pf = std::shared_ptr<micv_pf>(pf, micv_pf_destroy);
        _channels = model.channels();
        std::cout << "Initialized" << std::endl;  // ParticleFilter.cpp:29
        fetchParticles();
    }

    // Update the particle filter with a new frame: {(x, y) mean of the particles, x variance, y variance}
    std::tuple<micv_shim::Point2f, float, float> tick(const micv_shim::Mat &frame) {
        micv_shim::require(frame.depth() == micv_shim::U8 && frame.channels() == _channels &&
                               frame.rows == _imSize.height && frame.cols == _imSize.width,
                           "ParticleFilter::tick: the frame's size or type differs from the filter's");
        micv_pf_state st;
        micv_shim::check(micv_pf_tick_host(_pf.get(), frame.data, static_cast<size_t>(frame.step), &st));
        fetchParticles();
        return std::make_tuple(micv_shim::Point2f(st.x, st.y), st.x_var, st.y_var);
    }

    const std::vector<micv_shim::Point2f> &getParticles() const { return _particles; }

    // cv::circle(img, p, 1, color, -1) per particle (ParticleFilter.cpp:82-86).  Without OpenCV: the pixels within
    // distance 1 of cvRound(p), the centre and its four neighbours (parity with OpenCV's rasteriser unpinned).
    void drawParticles(micv_shim::Mat &img, const micv_shim::Scalar &color) {
#ifdef MICV_SHIM_WITH_OPENCV
        for (const auto &p : _particles) cv::circle(img, p, 1, color, -1);
#else
        micv_shim::require(img.depth() == micv_shim::U8, "ParticleFilter::drawParticles: 8-bit images only");
        const int cn = img.channels() < 4 ? img.channels() : 4;
        for (const auto &p : _particles) {
            if (!(p.x > -2.f && p.x < img.cols + 2.f && p.y > -2.f && p.y < img.rows + 2.f)) continue;
            const int cx = static_cast<int>(std::nearbyint(p.x)), cy = static_cast<int>(std::nearbyint(p.y));
            const int off[5][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}};
            for (const auto &o : off) {
                const int x = cx + o[0], y = cy + o[1];
                if (x < 0 || y < 0 || x >= img.cols || y >= img.rows) continue;
                unsigned char *d = img.ptr<unsigned char>(y) + static_cast<size_t>(x) * img.channels();
                for (int k = 0; k < cn; k++) {
                    const double v = std::nearbyint(color.val[k]);
                    d[k] = static_cast<unsigned char>(v < 0 ? 0 : (v > 255 ? 255 : v));
                }
            }
        }
#endif
    }

private:
    void fetchParticles() {
        std::vector<float> xy(2 * _numParticles);
        micv_shim::check(micv_pf_particles_host(_pf.get(), xy.data()));
        _particles.resize(xy.size() / 2);
        for (size_t i = 0; i < _particles.size(); i++) _particles[i] = micv_shim::Point2f(xy[2 * i], xy[2 * i + 1]);
    }
    std::shared_ptr<micv_pf> _pf;
    const micv_shim::Size _imSize;
    const size_t _numParticles;
    int _channels = 0;
    std::vector<micv_shim::Point2f> _particles;
};

namespace micv_shim {
inline void disparity(bool ncc, const Mat &left, const Mat &right, const size_t windowRad,
                      const int minDisparity, const int maxDisparity, int flags, Mat &disparity) {
    // The 8-bit images main.cpp loads, without its convertTo(CV_32FC1) (main.cpp:87-88): SSD takes them as they are, each
    // with its own step (an ROI starts at any byte); the disparities are those of the converted pair.
    if (left.type() == U8 || right.type() == U8) {
        require(!ncc, "disparityNCorr: CV_32FC1 images expected (8-bit pairs are taken by disparitySSD, and by "
                      "ps2::disparityNCorr8 / ps2::disparityNCorrPair8 of micv_display.hpp)");
        require(left.type() == U8 && right.type() == U8 && left.rows == right.rows && left.cols == right.cols,
                "disparitySSD: CV_8UC1 pair of equal size expected");
        disparity.create(left.rows, left.cols, S8);
        check(micv_disparity_ssd_u8_host(context(), left.ptr<uint8_t>(), left.step, right.ptr<uint8_t>(), right.step, left.rows,
                                         left.cols, static_cast<int>(windowRad), minDisparity, maxDisparity, flags,
                                         disparity.ptr<int8_t>(), disparity.step));
        return;
    }
    require(left.type() == F32 && right.type() == F32 && left.rows == right.rows &&
                left.cols == right.cols && left.step == right.step,
            "disparity: CV_32FC1 pair of equal size expected");  // DisparitySSD.cpp:15
    disparity.create(left.rows, left.cols, S8);                   // :32
    auto fn = ncc ? micv_disparity_ncorr_host : micv_disparity_ssd_host;
    check(fn(context(), left.ptr<float>(), right.ptr<float>(), left.rows, left.cols, left.step,
             static_cast<int>(windowRad), minDisparity, maxDisparity, flags,
             disparity.ptr<int8_t>(), disparity.step));
}
}  // namespace micv_shim

// `cuda::` = the CUDA kernels as written (2r-column window, 5e6 cut-off); `serial::` = the CPU
// functions as written.  micv_disparity_*(flags = 0) is the corrected (2r+1)^2 definition.
// The CUDA kernels also keep ROLLING column sums down 40-row strips (DisparitySSD.cu:97-138), which
// round differently from fresh sums on non-integer images.  ps2's inputs are 8-bit images converted to
// float (ps2_cpp/src/main.cpp:21-48), where both give the same disparities, so the shim stays on the fast
// kernel; build with -DMICV_SHIM_STEREO_ROLLING=1 to get the strip-serial sums for arbitrary f32 input.
#ifndef MICV_SHIM_STEREO_ROLLING
#define MICV_SHIM_STEREO_ROLLING 0
#endif
namespace cuda {
using micv_shim::Mat;
constexpr int kStereoRolling = MICV_SHIM_STEREO_ROLLING ? MICV_STEREO_ROLLING : 0;
inline void disparitySSD(const Mat &left, const Mat &right, const size_t windowRad,
                         const int minDisparity, const int maxDisparity, Mat &disparity) {
    micv_shim::disparity(false, left, right, windowRad, minDisparity, maxDisparity,
                         MICV_STEREO_COLS_2R | MICV_STEREO_MIN_SSD_5E6 | kStereoRolling, disparity);
}
inline void disparityNCorr(const Mat &left, const Mat &right, const size_t windowRad,
                           const int minDisparity, const int maxDisparity, Mat &disparity) {
    micv_shim::disparity(true, left, right, windowRad, minDisparity, maxDisparity,
                         MICV_STEREO_COLS_2R | kStereoRolling, disparity);
}
inline void houghLinesAccumulate(const Mat &edgeMask, const unsigned int rhoBinSize,
                                 const unsigned int thetaBinSize, Mat &accumulator) {
    micv_shim::require(edgeMask.type() == micv_shim::U8, "cuda::houghLinesAccumulate: CV_8UC1 expected");
    int rb = 0, tb = 0;
    micv_shim::check(micv_hough_lines_dims(edgeMask.rows, edgeMask.cols, rhoBinSize, thetaBinSize, &rb, &tb));
    Mat acc(rb, tb, micv_shim::S32);
    micv_shim::check(micv_hough_lines_host(micv_shim::context(), edgeMask.ptr<uint8_t>(), edgeMask.rows,
                                           edgeMask.cols, edgeMask.step, rhoBinSize, thetaBinSize,
                                           acc.ptr<int32_t>()));
    accumulator = acc;
}
inline void houghCirclesAccumulate(const Mat &edgeMask, const size_t radius, Mat &accumulator) {
    micv_shim::require(edgeMask.type() == micv_shim::U8, "cuda::houghCirclesAccumulate: CV_8UC1 expected");
    Mat acc(edgeMask.rows, edgeMask.cols, micv_shim::S32);
    micv_shim::check(micv_hough_circles_host(micv_shim::context(), edgeMask.ptr<uint8_t>(),
                                             edgeMask.rows, edgeMask.cols, edgeMask.step,
                                             static_cast<unsigned>(radius), acc.ptr<int32_t>()));
    accumulator = acc;
}
inline void findLocalMaxima(const Mat &accumulator, const unsigned int numPeaks, const int threshold,
                            std::vector<std::pair<unsigned int, unsigned int>> &localMaxima) {
    micv_shim::require(accumulator.type() == micv_shim::S32 && accumulator.isContinuous(),
                       "cuda::findLocalMaxima: continuous CV_32SC1 expected");
    std::vector<uint32_t> peaks(static_cast<size_t>(numPeaks) * 2 + 2);
    int64_t n = 0;
    micv_shim::check(micv_hough_peaks_host(micv_shim::context(), accumulator.ptr<int32_t>(),
                                           accumulator.rows, accumulator.cols, numPeaks, threshold,
                                           peaks.data(), &n));
    for (int64_t i = 0; i < n; i++) localMaxima.emplace_back(peaks[2 * i], peaks[2 * i + 1]);  // appended, Hough.cu:413
}

// The cv::cuda::GpuMat overloads (ps1_cpp/src/Hough.h:22-25, 48-51, 73-75; Hough.cu:251-286,
// 311-340, 366-426): device-resident in and out, nothing crosses PCIe except the peak list.
using micv_shim::GpuMat;
inline void houghLinesAccumulate(const GpuMat &edgeMask, const unsigned int rhoBinSize,
                                 const unsigned int thetaBinSize, GpuMat &accumulator) {
    micv_shim::require(edgeMask.type() == micv_shim::U8, "cuda::houghLinesAccumulate: CV_8UC1 expected");  // Hough.cu:255
    int rb = 0, tb = 0;
    micv_shim::check(micv_hough_lines_dims(edgeMask.rows, edgeMask.cols, rhoBinSize, thetaBinSize, &rb, &tb));
    micv_shim::create_continuous(accumulator, rb, tb, micv_shim::S32);  // :263
    micv_shim::check(micv_hough_lines_dev(micv_shim::context(), edgeMask.ptr<uint8_t>(), edgeMask.rows,
                                          edgeMask.cols, edgeMask.step, rhoBinSize, thetaBinSize,
                                          accumulator.ptr<int32_t>(), nullptr));
}
inline void houghCirclesAccumulate(const GpuMat &edgeMask, const size_t radius, GpuMat &accumulator) {
    micv_shim::require(edgeMask.type() == micv_shim::U8, "cuda::houghCirclesAccumulate: CV_8UC1 expected");
    micv_shim::create_continuous(accumulator, edgeMask.rows, edgeMask.cols, micv_shim::S32);  // Hough.cu:318
    micv_shim::check(micv_hough_circles_dev(micv_shim::context(), edgeMask.ptr<uint8_t>(), edgeMask.rows,
                                            edgeMask.cols, edgeMask.step, static_cast<unsigned>(radius),
                                            accumulator.ptr<int32_t>(), nullptr));
}
inline void findLocalMaxima(const GpuMat &accumulator, const unsigned int numPeaks, const int threshold,
                            std::vector<std::pair<unsigned int, unsigned int>> &localMaxima) {
    micv_shim::require(accumulator.type() == micv_shim::S32 && accumulator.isContinuous(),
                       "cuda::findLocalMaxima: continuous CV_32SC1 expected");
    // peaks (2 x u32 each) followed by the int64 count, in one device block
    const size_t peak_bytes = (static_cast<size_t>(numPeaks) * 2 + 2) * sizeof(uint32_t);
    void *blk = nullptr;
    micv_shim::check(micv_device_malloc(micv_shim::context(), peak_bytes + 8, &blk));
    std::vector<uint32_t> host(peak_bytes / 4 + 2);
    int rc = micv_hough_peaks_dev(micv_shim::context(), accumulator.ptr<int32_t>(), accumulator.rows,
                                  accumulator.cols, numPeaks, threshold, static_cast<uint32_t *>(blk),
                                  reinterpret_cast<int64_t *>(static_cast<char *>(blk) + peak_bytes), nullptr);
    if (rc == MICV_OK)
        rc = micv_memcpy2d_d2h(micv_shim::context(), host.data(), peak_bytes + 8, blk, peak_bytes + 8,
                               peak_bytes + 8, 1);
    micv_device_free(micv_shim::context(), blk);
    micv_shim::check(rc);
    int64_t n = 0;
    std::memcpy(&n, reinterpret_cast<const char *>(host.data()) + peak_bytes, 8);
    for (int64_t i = 0; i < n; i++) localMaxima.emplace_back(host[2 * i], host[2 * i + 1]);  // appended, Hough.cu:413
}
}  // namespace cuda

namespace serial {
using micv_shim::Mat;
inline void disparitySSD(const Mat &left, const Mat &right, const size_t windowRad,
                         const int minDisparity, const int maxDisparity, Mat &disparity) {
    micv_shim::disparity(false, left, right, windowRad, minDisparity, maxDisparity,
                         MICV_STEREO_SERIAL, disparity);
}
// serial::disparityNCorr calls cv::matchTemplate per pixel (DisparityNCorr.cpp:60-64), whose
// arithmetic is OpenCV's; the shim routes it to the (2r+1)^2 NCC defined in DESIGN.md.
inline void disparityNCorr(const Mat &left, const Mat &right, const size_t windowRad,
                           const int minDisparity, const int maxDisparity, Mat &disparity) {
    micv_shim::disparity(true, left, right, windowRad, minDisparity, maxDisparity, 0, disparity);
}
}  // namespace serial

// ---- "next" rows -----------------------------------------------------------------

namespace mhi {  // ProblemSets/ps7_cpp/include/MotionHistory.h:7-28
using micv_shim::Mat;
using micv_shim::Size;
// CV_8UC1, or the capture's CV_8UC3 / CV_8UC4 (MotionHistory.cpp:50-64: blur and subtract per channel, RGB2GRAY on the
// difference); ROIs of a larger frame included, the two with one step.  diff is CV_8UC1.
inline void frameDifference(const Mat &f1, const Mat &f2, const double thresh, Mat &diff,
                            const Size &blurSize = Size(3, 3), const double blurSigma = 1.0) {  // MotionHistory.h:10-15
    const int cn = f1.channels();
    micv_shim::require(f1.depth() == micv_shim::U8 && (cn == 1 || cn == 3 || cn == 4) && f2.type() == f1.type() &&
                           f1.rows == f2.rows && f1.cols == f2.cols && f1.step == f2.step,
                       "mhi::frameDifference: two CV_8UC1 / CV_8UC3 / CV_8UC4 frames of one type and size expected");
    Mat out(f1.rows, f1.cols, micv_shim::U8);
    if (cn == 1)
        micv_shim::check(micv_mhi_frame_difference_host(micv_shim::context(), f1.ptr<uint8_t>(), f2.ptr<uint8_t>(),
                                                        f1.rows, f1.cols, f1.step, thresh, blurSize.width,
                                                        blurSize.height, blurSigma, out.ptr<uint8_t>(), out.step));
    else
        micv_shim::check(micv_mhi_frame_difference_c_host(micv_shim::context(), f1.ptr<uint8_t>(), f2.ptr<uint8_t>(),
                                                          f1.rows, f1.cols, cn, f1.step, thresh, blurSize.width,
                                                          blurSize.height, blurSigma, out.ptr<uint8_t>(), out.step));
    diff = out;
}
inline void calcMotionHistory(Mat &history, const Mat &binaryMask, const int tau) {
    micv_shim::require(history.type() == micv_shim::U8 && binaryMask.type() == micv_shim::U8 &&
                           history.rows == binaryMask.rows && history.cols == binaryMask.cols,
                       "mhi::calcMotionHistory: CV_8UC1 history and mask of one size expected");
    micv_shim::check(micv_mhi_update_host(micv_shim::context(), history.ptr<uint8_t>(), history.step,
                                          binaryMask.ptr<uint8_t>(), binaryMask.step, history.rows,
                                          history.cols, tau));
}
inline void energyFromHistory(const Mat &mhi, Mat &mei) {  // MotionHistory.h:23, MotionHistory.cpp:98-105
    micv_shim::require(mhi.type() == micv_shim::U8, "mhi::energyFromHistory: CV_8UC1 expected");
    Mat out(mhi.rows, mhi.cols, micv_shim::U8);
    micv_shim::check(micv_mhi_energy_host(micv_shim::context(), mhi.ptr<uint8_t>(), mhi.rows, mhi.cols, mhi.step,
                                          out.ptr<uint8_t>(), out.step));
    mei = out;
}
inline void energyFromHistory(const std::vector<Mat> &mhis, std::vector<Mat> &meis) {  // :27, .cpp:107-112
    for (const auto &m : mhis) {
        Mat mei;
        energyFromHistory(m, mei);
        meis.push_back(mei);  // appended, like the reference
    }
}
}  // namespace mhi

namespace moments {  // ProblemSets/ps7_cpp/include/Moments.h:9-12, lib/Moments.cpp:7-67
using micv_shim::Mat;
// One image, CV_8UC1 or CV_32FC1 (the driver passes its cv::normalize-d MHIs as CV_32FC1 and its MEIs as CV_8UC1).
// The arithmetic is mi_cv.h's "ps7: central moments" with the reference's xFull - yBar kept as written.
inline std::vector<std::pair<float, float>> centralMoment(const Mat &img,
                                                          const std::vector<std::pair<int, int>> &momentOrders) {
    micv_shim::require(img.type() == micv_shim::U8 || img.type() == micv_shim::F32,
                       "moments::centralMoment: CV_8UC1 or CV_32FC1 expected");
    std::vector<std::pair<float, float>> out;
    const size_t n = momentOrders.size();
    std::vector<int> orders;
    for (const auto &o : momentOrders) {
        orders.push_back(o.first);
        orders.push_back(o.second);
    }
    std::vector<float> mu(MICV_MOMENTS_MAX_ORDERS), eta(MICV_MOMENTS_MAX_ORDERS);
    for (size_t j0 = 0; j0 < n; j0 += MICV_MOMENTS_MAX_ORDERS) {  // the C ABI takes up to 16 orders per call
        const int m = (int)std::min<size_t>(MICV_MOMENTS_MAX_ORDERS, n - j0);
        micv_shim::check(micv_central_moments_host(micv_shim::context(), img.data, 1, 0, img.step, img.rows, img.cols,
                                                   img.type() == micv_shim::F32 ? MICV_MOMENTS_F32 : MICV_MOMENTS_U8,
                                                   orders.data() + 2 * j0, m, 0, mu.data(), eta.data(), nullptr));
        for (int j = 0; j < m; j++) out.emplace_back(mu[j], eta[j]);
    }
    return out;
}
}  // namespace moments

namespace matching {  // ProblemSets/ps7_cpp/include/Matching.h:5-27, lib/Matching.cpp (k = 3, three actions)
using micv_shim::Mat;
namespace detail {
constexpr int kLabels = 3, kK = 3;  // Matching.cpp: cv::Mat::zeros(3, 3, CV_32F), findNearest(.., 3, ..)
// features CV_32FC1 (rows = samples); labels CV_32FC1 (arrangeTrainingData's convertTo) or CV_32SC1, one column
inline std::vector<int32_t> labels_of(const Mat &features, const Mat &labels) {
    micv_shim::require(features.type() == micv_shim::F32 && features.cols >= 1 && features.cols <= MICV_KNN_MAX_DIMS,
                       "matching: CV_32FC1 features of 1..64 columns expected");
    micv_shim::require(labels.rows == features.rows && labels.cols == 1 &&
                           (labels.type() == micv_shim::F32 || labels.type() == micv_shim::S32),
                       "matching: one CV_32FC1 / CV_32SC1 label per feature row expected");
    std::vector<int32_t> out(labels.rows);
    for (int r = 0; r < labels.rows; r++) {
        if (labels.type() == micv_shim::S32) {
            out[r] = labels.ptr<int32_t>(r)[0];
        } else {
            const float v = labels.ptr<float>(r)[0];
            micv_shim::require(v == std::nearbyint(v) && std::fabs(v) < 1e9f, "matching: labels must be integers");
            out[r] = (int32_t)v;
        }
    }
    return out;
}
inline Mat matrix(const float *m) {
    Mat c(kLabels, kLabels, micv_shim::F32);
    for (int r = 0; r < kLabels; r++)
        for (int x = 0; x < kLabels; x++) c.ptr<float>(r)[x] = m[r * kLabels + x];
    return c;
}
}  // namespace detail

// Leave-one-out; rows whose label or vote is outside 1..3 are left out of the matrix (the reference asserts).
inline void naiveConfusionMatrix(const Mat &features, const Mat &labels, Mat &confusion) {
    const std::vector<int32_t> lab = detail::labels_of(features, labels);
    float m[detail::kLabels * detail::kLabels];
    micv_shim::check(micv_knn_confusion_host(micv_shim::context(), features.ptr<float>(), features.rows, features.step,
                                             features.cols, lab.data(), nullptr, detail::kLabels, 0, detail::kK, 0, m,
                                             nullptr, nullptr));
    confusion = detail::matrix(m);
}

// Leave-one-person-out for persons 1..numPeople; appends numPeople matrices and then their average, like the reference.
inline void confusionMatrix(const Mat &features, const Mat &labels, const Mat &people, const size_t numPeople,
                            std::vector<Mat> &confusions) {
    const std::vector<int32_t> lab = detail::labels_of(features, labels);
    micv_shim::require(people.type() == micv_shim::S32 && people.rows == features.rows && people.cols == 1,
                       "matching::confusionMatrix: one CV_32SC1 person id per feature row expected");
    micv_shim::require(numPeople >= 1 && numPeople <= MICV_KNN_MAX_GROUPS, "matching::confusionMatrix: 1..32 people");
    std::vector<int32_t> grp(people.rows);
    for (int r = 0; r < people.rows; r++) grp[r] = people.ptr<int32_t>(r)[0];
    const int L2 = detail::kLabels * detail::kLabels;
    std::vector<float> m((numPeople + 1) * L2);
    micv_shim::check(micv_knn_confusion_host(micv_shim::context(), features.ptr<float>(), features.rows, features.step,
                                             features.cols, lab.data(), grp.data(), detail::kLabels, (int)numPeople,
                                             detail::kK, 0, m.data(), nullptr, nullptr));
    for (size_t g = 0; g <= numPeople; g++) confusions.push_back(detail::matrix(m.data() + g * L2));
}

// No gnuplot: prints the title and the numbers the plot labels ('%.2f', expected action = row, predicted = column) to
// stdout and, when fileName is given, writes the heat image (white -> green, 32 x 32 pixels per cell) as a binary PPM
// at fileName with its extension replaced by ".ppm".
inline void plotConfusionMatrix(const Mat &confusion, const std::string &title, const std::string &fileName = "") {
    micv_shim::require(confusion.type() == micv_shim::F32, "matching::plotConfusionMatrix: CV_32FC1 expected");
    std::cout << title << "\n";
    for (int y = 0; y < confusion.rows; y++) {
        std::cout << "action " << y + 1 << ":";
        for (int x = 0; x < confusion.cols; x++) {
            char b[32];
            std::snprintf(b, sizeof b, " %.2f", (double)confusion.ptr<float>(y)[x]);
            std::cout << b;
        }
        std::cout << "\n";
    }
    if (fileName.empty()) return;
    const size_t dot = fileName.find_last_of('.'), slash = fileName.find_last_of('/');
    const std::string path =
        (dot != std::string::npos && (slash == std::string::npos || dot > slash) ? fileName.substr(0, dot) : fileName) +
        ".ppm";
    const int cell = 32, W = confusion.cols * cell, H = confusion.rows * cell;
    std::vector<unsigned char> px((size_t)W * H * 3);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            float v = confusion.ptr<float>(y / cell)[x / cell];
            v = std::isfinite(v) ? std::min(std::max(v, 0.f), 1.f) : 0.f;  // palette (0 'white', 1 'green')
            unsigned char *p = &px[((size_t)y * W + x) * 3];
            p[0] = p[2] = (unsigned char)std::lrint(255.0 * (1.0 - v));
            p[1] = 255;
        }
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << W << " " << H << "\n255\n";
    f.write(reinterpret_cast<const char *>(px.data()), (std::streamsize)px.size());
    micv_shim::require((bool)f, "matching::plotConfusionMatrix: cannot write the image");
}
}  // namespace matching

namespace sol {
using micv_shim::Mat;
// The functions of ps1_cpp/src/Solution.h:19-75 with Config::EdgeDetect / Config::HoughLines / Config::Hough spelled
// out (gaussianSize, gaussianSigma, lowerThreshold, upperThreshold; rhoBinSize, thetaBinSize; numPeaks, threshold).
//
// sol::generateEdge, Solution.h:19, Solution.cpp:21-47 (Sobel aperture 3): CV_8UC1, or CV_32FC1 as problems 4-8 pass it
// (main.cpp:98, :107) -- ONE function that looks at the type at run time.
inline void generateEdge(const Mat &input, const int gaussianSize, const double gaussianSigma,
                         const double lowerThreshold, const double upperThreshold, Mat &output) {
    micv_shim::require(input.type() == micv_shim::U8 || input.type() == micv_shim::F32,
                       "sol::generateEdge: CV_8UC1 or CV_32FC1 expected");
    Mat out(input.rows, input.cols, micv_shim::U8);
    if (input.type() == micv_shim::U8)
        micv_shim::check(micv_generate_edge_host(micv_shim::context(), input.ptr<uint8_t>(), input.rows, input.cols,
                                                 input.step, gaussianSize, gaussianSigma, lowerThreshold,
                                                 upperThreshold, out.ptr<uint8_t>(), out.step));
    else
        micv_shim::check(micv_generate_edge_f32_host(micv_shim::context(), input.ptr<float>(), input.rows, input.cols,
                                                     input.step, gaussianSize, gaussianSigma, lowerThreshold,
                                                     upperThreshold, out.ptr<uint8_t>(), out.step));
    output = out;
}
// sol::generateEdge on several CV_8UC1 images of one size (ROIs with steps of their own included) in ONE
// micv_generate_edge_batch_host call: outputs[i] holds the bytes sol::generateEdge gives on inputs[i].  Not in the
// reference; the library's batch form of its first ps1 call.
inline void generateEdgeBatch(const std::vector<Mat> &inputs, const int gaussianSize, const double gaussianSigma,
                              const double lowerThreshold, const double upperThreshold, std::vector<Mat> &outputs) {
    micv_shim::require(!inputs.empty(), "sol::generateEdgeBatch: no image");
    std::vector<Mat> outs;
    std::vector<const uint8_t *> srcs;
    std::vector<uint8_t *> dsts;
    std::vector<size_t> steps, osteps;
    for (const Mat &m : inputs) {
        micv_shim::require(m.type() == micv_shim::U8 && m.rows == inputs[0].rows && m.cols == inputs[0].cols,
                           "sol::generateEdgeBatch: CV_8UC1 images of one size expected");
        outs.emplace_back(m.rows, m.cols, micv_shim::U8);
        srcs.push_back(m.ptr<uint8_t>());
        steps.push_back(m.step);
        dsts.push_back(outs.back().ptr<uint8_t>());
        osteps.push_back(outs.back().step);
    }
    micv_shim::check(micv_generate_edge_batch_host(micv_shim::context(), srcs.data(), steps.data(), (int)inputs.size(), inputs[0].rows,
                                                   inputs[0].cols, gaussianSize, gaussianSigma, lowerThreshold, upperThreshold, dsts.data(),
                                                   osteps.data()));
    outputs = outs;
}
// sol::gaussianBlur, Solution.h:21, Solution.cpp:49-61: the output has the input's type (CV_8UC1 or CV_32FC1)
inline void gaussianBlur(const Mat &input, const int gaussianSize, const double gaussianSigma, Mat &output) {
    micv_shim::require(input.type() == micv_shim::U8 || input.type() == micv_shim::F32,
                       "sol::gaussianBlur: CV_8UC1 or CV_32FC1 expected");
    Mat out(input.rows, input.cols, input.type());
    if (input.type() == micv_shim::U8)
        micv_shim::check(micv_gaussian_blur_u8_host(micv_shim::context(), input.ptr<uint8_t>(), input.rows, input.cols,
                                                    input.step, gaussianSize, gaussianSigma, out.ptr<uint8_t>(), out.step));
    else
        micv_shim::check(micv_gaussian_blur_f32_host(micv_shim::context(), input.ptr<float>(), input.rows, input.cols,
                                                     input.step, gaussianSize, gaussianSigma, out.ptr<float>(), out.step));
    output = out;
}
// Solution.h:26-30, :39-41, Solution.cpp:63-79
inline void houghLinesAccumulate(const Mat &edgeMask, const unsigned int rhoBinSize, const unsigned int thetaBinSize,
                                 Mat &accumulator) {
    cuda::houghLinesAccumulate(edgeMask, rhoBinSize, thetaBinSize, accumulator);
}
inline void houghCirclesAccumulate(const Mat &edgeMask, const size_t radius, Mat &accumulator) {
    cuda::houghCirclesAccumulate(edgeMask, radius, accumulator);
}
inline void findLocalMaxima(const Mat &accumulator, const unsigned int numPeaks, const int threshold,
                            std::vector<std::pair<unsigned int, unsigned int>> &localMaxima) {
    cuda::findLocalMaxima(accumulator, numPeaks, threshold, localMaxima);
}
// The radius loops of main.cpp:173-180, :263-270, :299-307 as one call (micv_hough_circles_range_peaks_host): entry i of
// localMaxima holds what houghCirclesAccumulate(edgeMask, minRadius + i) + findLocalMaxima(numPeaks, threshold) give.
inline void houghCirclesSearch(const Mat &edgeMask, const size_t minRadius, const size_t maxRadius,
                               const unsigned int numPeaks, const int threshold,
                               std::vector<std::vector<std::pair<unsigned int, unsigned int>>> &localMaxima) {
    micv_shim::require(edgeMask.type() == micv_shim::U8, "sol::houghCirclesSearch: CV_8UC1 expected");
    localMaxima.clear();
    if (minRadius > maxRadius) return;
    micv_shim::require(maxRadius <= 0xFFFFFFFFull, "sol::houghCirclesSearch: radius out of range");
    const size_t n = maxRadius - minRadius + 1;
    std::vector<uint32_t> peaks(n * numPeaks * 2 + 2);
    std::vector<int64_t> counts(n);
    micv_shim::check(micv_hough_circles_range_peaks_host(micv_shim::context(), edgeMask.ptr<uint8_t>(), edgeMask.rows,
                                                         edgeMask.cols, edgeMask.step, (unsigned)minRadius,
                                                         (unsigned)maxRadius, numPeaks, threshold, peaks.data(),
                                                         counts.data(), nullptr));
    localMaxima.resize(n);
    for (size_t i = 0; i < n; i++)
        for (int64_t k = 0; k < counts[i]; k++)
            localMaxima[i].emplace_back(peaks[(i * numPeaks + k) * 2], peaks[(i * numPeaks + k) * 2 + 1]);
}
// sol::rowColToRhoTheta, Solution.h:56-58, Solution.cpp:81-89
inline std::pair<int, int> rowColToRhoTheta(const std::pair<unsigned int, unsigned int> &coordinates,
                                            const Mat &inputImage, const unsigned int rhoBinSize,
                                            const unsigned int thetaBinSize) {
    const size_t diagDist = (size_t)std::ceil(std::sqrt((double)(inputImage.rows * inputImage.rows + inputImage.cols * inputImage.cols)));
    const int rho = (int)((size_t)coordinates.first * rhoBinSize - diagDist);
    const int theta = (int)(coordinates.second * thetaBinSize + (unsigned)-90);
    return std::make_pair(rho, theta);
}
namespace detail {
inline void require_bgr(const Mat &image, const char *what) {
    micv_shim::require(image.depth() == micv_shim::U8 && image.channels() == 3, what);
}
inline void color_bytes(const micv_shim::Scalar &color, uint8_t *c) {  // saturate_cast<uchar> of the first three entries
    for (int i = 0; i < 3; i++) {
        const double v = color.val[i];
        const long r = v >= -2147483648.0 && v < 2147483648.0 ? std::lrint(v) : -1;
        c[i] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
}
}  // namespace detail
// sol::drawLinesParametric, Solution.h:62-64, Solution.cpp:117-123, on an 8-bit three-channel image (GRAY2RGB first, as
// the driver does).  (rho, theta) pairs of rowColToRhoTheta are (row - diag, col - 90) at bin size 1, which is how they
// are handed to micv_draw_lines_parametric_host; theta outside [-90, 89] or rho < -diag name no accumulator cell and
// are not drawn.
inline void drawLinesParametric(Mat &image, const std::vector<std::pair<int, int>> &rhoTheta,
                                const micv_shim::Scalar color) {
    detail::require_bgr(image, "sol::drawLinesParametric: CV_8UC3 expected");
    const long long diag = (long long)std::ceil(std::sqrt((double)(image.rows * image.rows + image.cols * image.cols)));
    std::vector<uint32_t> peaks;
    for (const auto &val : rhoTheta) {
        if (val.second < -90 || val.second > 89 || (long long)val.first + diag < 0) continue;
        peaks.push_back((uint32_t)((long long)val.first + diag));
        peaks.push_back((uint32_t)(val.second + 90));
    }
    uint8_t c[3];
    detail::color_bytes(color, c);
    for (size_t at = 0; at < peaks.size() / 2; at += 4096) {  // the entry takes up to 4096 lines
        const int64_t n = (int64_t)std::min<size_t>(4096, peaks.size() / 2 - at);
        micv_shim::check(micv_draw_lines_parametric_host(micv_shim::context(), image.ptr<uint8_t>(), image.rows, image.cols,
                                                         image.step, peaks.data() + 2 * at, n, 1, 1, c));
    }
}
// sol::drawLineParametric, Solution.h:59, Solution.cpp:91-115 (integer-valued rho and theta, as the driver passes them)
inline void drawLineParametric(Mat &image, const float rho, const float theta, const micv_shim::Scalar color) {
    micv_shim::require(rho == std::nearbyint(rho) && theta == std::nearbyint(theta) && std::fabs(rho) < 1e9f,
                       "sol::drawLineParametric: integer-valued rho and theta expected");
    drawLinesParametric(image, {std::make_pair((int)rho, (int)theta)}, color);
}
// sol::drawCircles, Solution.h:67-70, Solution.cpp:125-132
inline void drawCircles(Mat &image, const std::vector<std::pair<unsigned int, unsigned int>> &center,
                        const size_t radius, const micv_shim::Scalar color) {
    detail::require_bgr(image, "sol::drawCircles: CV_8UC3 expected");
    micv_shim::require(radius <= 0xFFFFFFFFull, "sol::drawCircles: radius out of range");
    uint8_t c[3];
    detail::color_bytes(color, c);
    std::vector<uint32_t> peaks;
    for (const auto &p : center) {
        peaks.push_back(p.first);
        peaks.push_back(p.second);
    }
    for (size_t at = 0; at < center.size(); at += 4096) {
        const int64_t n = (int64_t)std::min<size_t>(4096, center.size() - at);
        micv_shim::check(micv_draw_circles_host(micv_shim::context(), image.ptr<uint8_t>(), image.rows, image.cols, image.step,
                                                peaks.data() + 2 * at, &n, 1, (unsigned)n, (unsigned)radius, c));
    }
}
// drawCircles for the lists of houghCirclesSearch: entry i with radius minRadius + i, all in one call
inline void drawCircles(Mat &image, const std::vector<std::vector<std::pair<unsigned int, unsigned int>>> &centers,
                        const size_t minRadius, const micv_shim::Scalar color) {
    detail::require_bgr(image, "sol::drawCircles: CV_8UC3 expected");
    size_t k = 0;
    for (const auto &l : centers) k = std::max(k, l.size());
    micv_shim::require(k <= 4096 && minRadius + centers.size() <= 0xFFFFFFFFull, "sol::drawCircles: too many circles");
    if (k == 0) return;
    std::vector<uint32_t> peaks(centers.size() * k * 2, 0);
    std::vector<int64_t> counts(centers.size());
    for (size_t i = 0; i < centers.size(); i++) {
        counts[i] = (int64_t)centers[i].size();
        for (size_t j = 0; j < centers[i].size(); j++) {
            peaks[(i * k + j) * 2] = centers[i][j].first;
            peaks[(i * k + j) * 2 + 1] = centers[i][j].second;
        }
    }
    uint8_t c[3];
    detail::color_bytes(color, c);
    micv_shim::check(micv_draw_circles_host(micv_shim::context(), image.ptr<uint8_t>(), image.rows, image.cols, image.step,
                                            peaks.data(), counts.data(), (unsigned)centers.size(), (unsigned)k,
                                            (unsigned)minRadius, c));
}
// sol::findParallelLines, Solution.h:72-75, Solution.cpp:134-173.  The kept pairs come in INPUT order (the reference's
// order is that of an unordered_multimap's buckets; every use draws them in one colour).
inline void findParallelLines(const std::vector<std::pair<uint32_t, uint32_t>> &rhoTheta, const size_t deltaTheta,
                              const size_t deltaRho, std::vector<std::pair<uint32_t, uint32_t>> &parallelRhoThetas) {
    parallelRhoThetas.clear();
    micv_shim::require(rhoTheta.size() <= 4096, "sol::findParallelLines: at most 4096 lines");
    micv_shim::require(deltaTheta >= 1 && deltaRho >= 1 && deltaTheta <= 0xFFFFFFFFull && deltaRho <= 0xFFFFFFFFull,
                       "sol::findParallelLines: deltaTheta and deltaRho must be positive");
    std::vector<uint32_t> in, out(rhoTheta.size() * 2 + 2);
    for (const auto &p : rhoTheta) {
        in.push_back(p.first);
        in.push_back(p.second);
    }
    int64_t n = 0;
    micv_shim::check(micv_parallel_lines_host(micv_shim::context(), in.data(), (int64_t)rhoTheta.size(), (unsigned)deltaRho,
                                              (unsigned)deltaTheta, out.data(), &n));
    for (int64_t i = 0; i < n; i++) parallelRhoThetas.emplace_back(out[2 * i], out[2 * i + 1]);
}
// cv::erode(src, dst, cv::getStructuringElement(cv::MORPH_ELLIPSE, cv::Size(ksize, ksize))), main.cpp:246-248
inline void erodeEllipse(const Mat &input, const int ksize, Mat &output) {
    micv_shim::require(input.type() == micv_shim::U8 || input.type() == micv_shim::F32, "sol::erodeEllipse: CV_8UC1 or CV_32FC1 expected");
    Mat out(input.rows, input.cols, input.type());
    if (input.type() == micv_shim::U8)
        micv_shim::check(micv_erode_ellipse_u8_host(micv_shim::context(), input.ptr<uint8_t>(), input.rows, input.cols, input.step,
                                                    ksize, out.ptr<uint8_t>(), out.step));
    else
        micv_shim::check(micv_erode_ellipse_f32_host(micv_shim::context(), input.ptr<float>(), input.rows, input.cols, input.step,
                                                     ksize, out.ptr<float>(), out.step));
    output = out;
}
// cv::cvtColor(src, dst, CV_GRAY2RGB) to 8 bit (main.cpp:88): CV_8UC1 or CV_32FC1 -> CV_8UC3
inline void gray2rgb(const Mat &input, Mat &output) {
    micv_shim::require(input.type() == micv_shim::U8 || input.type() == micv_shim::F32, "sol::gray2rgb: CV_8UC1 or CV_32FC1 expected");
    Mat out(input.rows, input.cols, micv_shim::U8C3);
    micv_shim::check(micv_gray_to_rgb8_host(micv_shim::context(), input.data, input.type() == micv_shim::U8 ? MICV_DEPTH_8U : MICV_DEPTH_32F,
                                            input.rows, input.cols, input.step, out.ptr<uint8_t>(), out.step));
    output = out;
}
// The matching step of Solution::siftHelper, ps4_cpp/src/Solution.cpp:172-184:
// BFMatcher::knnMatch(d1, d2, raw, 2) + `m[0].distance < ratio * m[1].distance`.
// goodMatches receives (queryIdx, trainIdx) pairs, distances the matching m[0].distance.
inline void matchDescriptors(const Mat &d1, const Mat &d2, const double ratio,
                             std::vector<std::pair<int, int>> &goodMatches, std::vector<float> &distances) {
    micv_shim::require(d1.type() == micv_shim::F32 && d2.type() == micv_shim::F32 && d1.cols == d2.cols &&
                           d2.rows >= 2,
                       "sol::matchDescriptors: CV_32FC1 descriptor matrices of one width expected");
    std::vector<int32_t> idx2(static_cast<size_t>(d1.rows) * 2), m(static_cast<size_t>(d1.rows) * 2);
    std::vector<float> dist2(static_cast<size_t>(d1.rows) * 2), dd(static_cast<size_t>(d1.rows));
    micv_shim::check(micv_bf_knn2_host(micv_shim::context(), d1.ptr<float>(), d1.rows, d1.step, d2.ptr<float>(),
                                       d2.rows, d2.step, d1.cols, idx2.data(), dist2.data()));
    int64_t n = 0;
    micv_shim::check(micv_bf_ratio_filter_host(micv_shim::context(), idx2.data(), dist2.data(), d1.rows, ratio,
                                               m.data(), dd.data(), d1.rows, &n));
    goodMatches.clear();
    distances.clear();
    for (int64_t i = 0; i < n; i++) {
        goodMatches.emplace_back(m[2 * i], m[2 * i + 1]);
        distances.push_back(dd[i]);
    }
}
}  // namespace sol
