// micv_display.hpp -- the OpenCV calls that end the reference's runProblem* functions, and ps2's driver functions, over
// libmicv.so's "display" entry points (include/mi_cv.h):
//   micv_cv::normalize        cv::normalize(x, x, 0, 255, cv::NORM_MINMAX, CV_8U)      ps2 main.cpp:94 ..., ps5 Solution.cpp:74
//   micv_cv::applyColorMap    cv::applyColorMap(x, x, cv::COLORMAP_JET)                ps5 Solution.cpp:76-77
//   micv_cv::randn            cv::randn(noise, mean, sigma) on CV_32FC1 from theRNG()  ps2 main.cpp:147,151
//   ps2::disparitySSDPair, ps2::disparityNCorrPair, ps2::addNoise                      ps2 main.cpp:21-78, 140-153
//   ps2::pairAndDisplay       one pair-and-display block of a runProblem* as ONE library call
// Same argument order, defaults and constant values as OpenCV's; argument combinations other than the ones named here
// throw std::invalid_argument saying what is supported.  The arithmetic is the library's ("display":
// it restates OpenCV 3.4, parity unpinned).  Header-only; works on micv::Mat and, with -DMICV_SHIM_WITH_OPENCV, on
// cv::Mat.
#pragma once

#include <cstdint>

#include "micv_shim.hpp"

namespace micv_cv {
using micv_shim::Mat;

enum { NORM_INF = 1, NORM_L1 = 2, NORM_L2 = 4, NORM_MINMAX = 32 };  // cv::NormTypes
enum { COLORMAP_AUTUMN = 0, COLORMAP_BONE = 1, COLORMAP_JET = 2 };  // cv::ColormapTypes

inline int display_depth(const Mat &m, const char *what) {
    micv_shim::require(!m.empty() && m.channels() == 1 &&
                           (m.depth() == micv_shim::F32 || m.depth() == micv_shim::U8 || m.depth() == micv_shim::S8), what);
    return m.depth() == micv_shim::F32 ? MICV_DEPTH_32F : (m.depth() == micv_shim::U8 ? MICV_DEPTH_8U : MICV_DEPTH_8S);
}

// cv::normalize(src, dst, alpha, beta, norm_type, dtype): alpha = 0, beta = 255, NORM_MINMAX, dtype CV_8U (= CV_8UC1) on a
// single-channel CV_32F, CV_8U or CV_8S image; dst may be src.
inline void normalize(const Mat &src, Mat &dst, double alpha = 1, double beta = 0, int norm_type = NORM_L2, int dtype = -1) {
    const int depth = display_depth(src, "normalize: single-channel CV_32F, CV_8U or CV_8S expected");
    micv_shim::require(alpha == 0 && beta == 255 && norm_type == NORM_MINMAX && dtype == micv_shim::U8,
                       "normalize: only (alpha 0, beta 255, NORM_MINMAX, CV_8U) is supported");
    Mat out;
    out.create(src.rows, src.cols, micv_shim::U8);
    micv_shim::check(micv_normalize_minmax_host(micv_shim::context(), src.data, depth, src.rows, src.cols, src.step, out.data,
                                                out.step, nullptr, 0, nullptr, 0, nullptr));
    dst = out;
}

// cv::applyColorMap(src, dst, COLORMAP_JET): CV_8UC1 -> CV_8UC3 (B, G, R); dst may be src.
inline void applyColorMap(const Mat &src, Mat &dst, int colormap) {
    micv_shim::require(!src.empty() && src.channels() == 1 && src.depth() == micv_shim::U8, "applyColorMap: CV_8UC1 expected");
    micv_shim::require(colormap == COLORMAP_JET, "applyColorMap: only COLORMAP_JET is supported");
    Mat out;
    out.create(src.rows, src.cols, micv_shim::U8 + 16);  // CV_8UC3
    micv_shim::check(micv_apply_colormap_jet_host(micv_shim::context(), src.data, src.rows, src.cols, src.step, out.data, out.step));
    dst = out;
}

// cv::theRNG(): one generator per thread, state 0xffffffff at first.
struct RNG {
    uint64_t state = 0xffffffffull;
};
inline RNG &theRNG() {
    static thread_local RNG rng;
    return rng;
}

// cv::randn(dst, mean, stddev) on an allocated CV_32FC1 image, from theRNG().
inline void randn(Mat &dst, double mean, double stddev) {
    micv_shim::require(!dst.empty() && dst.type() == micv_shim::F32, "randn: an allocated CV_32FC1 image expected");
    micv_shim::check(micv_cv_randn_f32_host(&theRNG().state, (float)mean, (float)stddev, dst.rows, dst.cols, dst.ptr<float>(), dst.step));
}
}  // namespace micv_cv

namespace ps2 {
using micv_shim::Mat;

struct DisparityConfig {  // Config::DisparitySSD (ps2_cpp/include/Config.h:40-42)
    size_t _windowRadius = 0;
    size_t _disparityRange = 0;
};

// The flags of the shim's cuda:: and serial:: functions (micv_shim.hpp): the CUDA kernels as written, or the CPU functions.
inline int stereo_flags(bool ncc, bool useGpuDisparity) {
    if (useGpuDisparity) return ncc ? (MICV_STEREO_COLS_2R | cuda::kStereoRolling) : (MICV_STEREO_COLS_2R | MICV_STEREO_MIN_SSD_5E6 | cuda::kStereoRolling);
    return ncc ? 0 : MICV_STEREO_SERIAL;
}
inline void check_pair(const Mat &left, const Mat &right, const char *what) {
    micv_shim::require(left.type() == micv_shim::F32 && right.type() == micv_shim::F32 && left.rows == right.rows &&
                           left.cols == right.cols && left.step == right.step, what);
}
inline void pair(bool ncc, const Mat &left, const Mat &right, const bool useGpuDisparity, const DisparityConfig &config,
                 Mat &leftDisparity, Mat &rightDisparity) {
    if (left.type() == micv_shim::U8 || right.type() == micv_shim::U8) {
        // 8-bit Mats (SSD only; micv_shim::disparity refuses NCC with a message): the two searches of main.cpp:21-48 as
        // two u8 calls -- the left image as reference over [-range, 0], the right one over [0, range]
        const int range = (int)config._disparityRange, flags = stereo_flags(ncc, useGpuDisparity);
        Mat l, r;
        micv_shim::disparity(ncc, left, right, config._windowRadius, -range, 0, flags, l);
        micv_shim::disparity(ncc, right, left, config._windowRadius, 0, range, flags, r);
        leftDisparity = l;
        rightDisparity = r;
        return;
    }
    check_pair(left, right, "disparity pair: CV_32FC1 images of equal size expected");
    Mat l, r;
    l.create(left.rows, left.cols, micv_shim::S8);
    r.create(left.rows, left.cols, micv_shim::S8);
    micv_shim::check(micv_disparity_pair_host(micv_shim::context(), left.ptr<float>(), right.ptr<float>(), left.rows, left.cols,
                                              left.step, (int)config._windowRadius, (int)config._disparityRange,
                                              ncc ? MICV_DISPARITY_NCC : MICV_DISPARITY_SSD, stereo_flags(ncc, useGpuDisparity),
                                              l.ptr<int8_t>(), r.ptr<int8_t>(), l.step));
    leftDisparity = l;
    rightDisparity = r;
}

// main.cpp:21-48
inline void disparitySSDPair(const Mat &left, const Mat &right, const bool useGpuDisparity, const DisparityConfig &config,
                             Mat &leftDisparity, Mat &rightDisparity) {
    pair(false, left, right, useGpuDisparity, config, leftDisparity, rightDisparity);
}
// main.cpp:51-78
inline void disparityNCorrPair(const Mat &left, const Mat &right, const bool useGpuDisparity, const DisparityConfig &config,
                               Mat &leftDisparity, Mat &rightDisparity) {
    pair(true, left, right, useGpuDisparity, config, leftDisparity, rightDisparity);
}

// disparityNCorr on the 8-bit Mats main.cpp loads, without its convertTo(CV_32FC1) (main.cpp:227-229, 304-306): CV_8UC1,
// ROI views included, each with its own step; the disparities are those of cuda:: / serial::disparityNCorr on the converted
// pair.  (Functions of their own: cuda:: / serial::disparityNCorr and disparityNCorrPair keep refusing 8-bit Mats.)
inline void disparityNCorr8(const Mat &left, const Mat &right, const size_t windowRad, const int minDisparity,
                            const int maxDisparity, const bool useGpuDisparity, Mat &disparity) {
    micv_shim::require(left.type() == micv_shim::U8 && right.type() == micv_shim::U8 && left.rows == right.rows &&
                           left.cols == right.cols, "disparityNCorr8: CV_8UC1 pair of equal size expected");
    Mat d;
    d.create(left.rows, left.cols, micv_shim::S8);
    micv_shim::check(micv_disparity_ncorr_u8_host(micv_shim::context(), left.ptr<uint8_t>(), left.step, right.ptr<uint8_t>(),
                                                  right.step, left.rows, left.cols, static_cast<int>(windowRad), minDisparity,
                                                  maxDisparity, stereo_flags(true, useGpuDisparity), d.ptr<int8_t>(), d.step));
    disparity = d;
}
// main.cpp:51-78: the left image as reference over [-range, 0], the right one over [0, range]
inline void disparityNCorrPair8(const Mat &left, const Mat &right, const bool useGpuDisparity, const DisparityConfig &config,
                                Mat &leftDisparity, Mat &rightDisparity) {
    const int range = (int)config._disparityRange;
    Mat l, r;
    disparityNCorr8(left, right, config._windowRadius, -range, 0, useGpuDisparity, l);
    disparityNCorr8(right, left, config._windowRadius, 0, range, useGpuDisparity, r);
    leftDisparity = l;
    rightDisparity = r;
}

// The two cv::randn calls of addNoise, in its order: what pairAndDisplay takes as noise.
inline void drawNoise(const Mat &first, const Mat &second, const float mean, const float sigma, Mat &firstNoise, Mat &secondNoise) {
    firstNoise.create(first.rows, first.cols, micv_shim::F32);
    micv_cv::randn(firstNoise, mean, sigma);
    secondNoise.create(second.rows, second.cols, micv_shim::F32);
    micv_cv::randn(secondNoise, mean, sigma);
}

// main.cpp:140-153: firstNoisy = first + noise, secondNoisy = second + noise'.
inline void addNoise(const Mat &first, const Mat &second, const float mean, const float sigma, Mat &firstNoisy, Mat &secondNoisy) {
    micv_shim::require(first.type() == micv_shim::F32 && second.type() == micv_shim::F32, "addNoise: CV_32FC1 expected");
    Mat n1, n2, a, b;
    drawNoise(first, second, mean, sigma, n1, n2);
    a.create(first.rows, first.cols, micv_shim::F32);
    b.create(second.rows, second.cols, micv_shim::F32);
    micv_shim::check(micv_gain_noise_f32_host(micv_shim::context(), first.ptr<float>(), first.step, 1.f, n1.ptr<float>(), n1.step,
                                              first.rows, first.cols, a.ptr<float>(), a.step));
    micv_shim::check(micv_gain_noise_f32_host(micv_shim::context(), second.ptr<float>(), second.step, 1.f, n2.ptr<float>(), n2.step,
                                              second.rows, second.cols, b.ptr<float>(), b.step));
    firstNoisy = a;
    secondNoisy = b;
}

// What one pair-and-display block of a runProblem* leaves: the two CV_8SC1 maps and the images the driver writes.
struct PairDisplay {
    Mat leftDisparity, rightDisparity;  // CV_8SC1
    Mat left, leftInverted, right;      // CV_8UC1: cv::normalize(.., 0, 255, NORM_MINMAX, CV_8UC1); ones * 255 - left
};

// The block as ONE call: left * gain + noise, right * gain + noise' (noise images empty: none), the pair, the three
// display images (inverted = false: leftInverted is not made, as in runProblem1).  Uploads the grey images (and the
// noise), downloads the maps and the 8-bit images.
inline PairDisplay pairAndDisplay(bool ncc, const Mat &left, const Mat &right, const bool useGpuDisparity,
                                  const DisparityConfig &config, float gain = 1.f, const Mat &noiseLeft = Mat(),
                                  const Mat &noiseRight = Mat(), bool inverted = true) {
    check_pair(left, right, "pairAndDisplay: CV_32FC1 images of equal size expected");
    const bool noisy = !noiseLeft.empty() || !noiseRight.empty();
    if (noisy) {
        check_pair(noiseLeft, noiseRight, "pairAndDisplay: CV_32FC1 noise images of equal size expected");
        micv_shim::require(noiseLeft.rows == left.rows && noiseLeft.cols == left.cols, "pairAndDisplay: noise of the images' size expected");
    }
    PairDisplay o;
    o.leftDisparity.create(left.rows, left.cols, micv_shim::S8);
    o.rightDisparity.create(left.rows, left.cols, micv_shim::S8);
    o.left.create(left.rows, left.cols, micv_shim::U8);
    if (inverted) o.leftInverted.create(left.rows, left.cols, micv_shim::U8);
    o.right.create(left.rows, left.cols, micv_shim::U8);
    micv_shim::check(micv_disparity_pair_display_host(
        micv_shim::context(), left.ptr<float>(), right.ptr<float>(), left.rows, left.cols, left.step, gain,
        noisy ? noiseLeft.ptr<float>() : nullptr, noisy ? noiseRight.ptr<float>() : nullptr, noisy ? noiseLeft.step : 0,
        (int)config._windowRadius, (int)config._disparityRange, ncc ? MICV_DISPARITY_NCC : MICV_DISPARITY_SSD,
        stereo_flags(ncc, useGpuDisparity), o.leftDisparity.ptr<int8_t>(), o.rightDisparity.ptr<int8_t>(), o.leftDisparity.step,
        o.left.data, inverted ? o.leftInverted.data : nullptr, o.right.data, o.left.step));
    return o;
}
}  // namespace ps2
