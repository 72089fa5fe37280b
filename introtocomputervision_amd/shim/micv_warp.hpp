// micv_warp.hpp -- the three OpenCV calls at the end of Solution::runProblem3 (ProblemSets/ps4_cpp/src/Solution.cpp:
// 315-325 for the similarity, :344-354 for the affine case) over libmicv.so's "ps4: registration" entry points:
//   micv_cv::invertAffineTransform   cv::invertAffineTransform(transform, transform)              :315, :344
//   micv_cv::warpAffine              cv::warpAffine(simB, reverseWarp, transform, size)          :322, :351
//   micv_cv::addWeighted             blended = simA * 0.5 + reverseWarp * 0.5                     :325, :354
//   sol::registerAndBlend            the five lines as one call (one launch on the device)
// Same argument order, defaults and flag values as OpenCV's; CV_8UC1 and CV_32FC1 images, CV_32F 2x3 transforms,
// INTER_NEAREST / INTER_LINEAR with or without WARP_INVERSE_MAP, BORDER_CONSTANT 0.  The arithmetic is the library's
// (include/mi_cv.h, DESIGN.md section 2: it restates OpenCV 3.4.1, parity unpinned).  Header-only; works on micv::Mat
// and, with -DMICV_SHIM_WITH_OPENCV, on cv::Mat.
#pragma once

#include "micv_shim.hpp"

namespace micv_cv {
using micv_shim::Mat;
using micv_shim::Size;

enum { INTER_NEAREST = 0, INTER_LINEAR = 1, WARP_INVERSE_MAP = 16 };  // cv::InterpolationFlags

inline int depth_of(const Mat &m, const char *what) {
    micv_shim::require(!m.empty() && m.channels() == 1 && (m.depth() == micv_shim::U8 || m.depth() == micv_shim::F32), what);
    return m.depth() == micv_shim::U8 ? MICV_DEPTH_8U : MICV_DEPTH_32F;
}
inline void transform_of(const Mat &M, float *six, const char *what) {
    micv_shim::require(M.rows == 2 && M.cols == 3 && M.type() == micv_shim::F32, what);
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 3; c++) six[3 * r + c] = M.ptr<float>(r)[c];
}

// iM may be M itself, as the reference calls it.
inline void invertAffineTransform(const Mat &M, Mat &iM) {
    float m[6], inv[6];
    transform_of(M, m, "invertAffineTransform: 2 x 3 CV_32F expected");
    micv_shim::check(micv_invert_affine_host(micv_shim::context(), m, 1, inv));
    iM.create(2, 3, micv_shim::F32);
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 3; c++) iM.ptr<float>(r)[c] = inv[3 * r + c];
}

inline void warpAffine(const Mat &src, Mat &dst, const Mat &M, Size dsize, int flags = INTER_LINEAR) {
    const int depth = depth_of(src, "warpAffine: CV_8UC1 or CV_32FC1 expected");
    float m[6];
    transform_of(M, m, "warpAffine: 2 x 3 CV_32F expected");
    const int interp = flags & 7;
    micv_shim::require((interp == INTER_NEAREST || interp == INTER_LINEAR) && !(flags & ~(7 | WARP_INVERSE_MAP)),
                       "warpAffine: INTER_NEAREST or INTER_LINEAR, optionally WARP_INVERSE_MAP");
    micv_shim::require(dsize.width > 0 && dsize.height > 0, "warpAffine: empty dsize");
    Mat out;  // a fresh Mat, so dst may be src (OpenCV copies in that case too)
    out.create(dsize.height, dsize.width, src.type());
    micv_shim::check(micv_warp_affine_host(micv_shim::context(), src.data, depth, src.rows, src.cols, src.step, m,
                                           (interp == INTER_NEAREST ? MICV_WARP_NEAREST : 0) |
                                               ((flags & WARP_INVERSE_MAP) ? MICV_WARP_INVERSE_MAP : 0),
                                           out.data, out.rows, out.cols, out.step));
    dst = out;
}

inline void addWeighted(const Mat &src1, double alpha, const Mat &src2, double beta, double gamma, Mat &dst) {
    const int depth = depth_of(src1, "addWeighted: CV_8UC1 or CV_32FC1 expected");
    micv_shim::require(src2.type() == src1.type() && src2.rows == src1.rows && src2.cols == src1.cols,
                       "addWeighted: sizes or types differ");
    Mat out;
    out.create(src1.rows, src1.cols, src1.type());
    micv_shim::check(micv_add_weighted_host(micv_shim::context(), src1.data, src1.step, alpha, src2.data, src2.step, beta, gamma,
                                            depth, src1.rows, src1.cols, out.data, out.step));
    dst = out;
}
}  // namespace micv_cv

namespace sol {
// Solution.cpp:315-325: `transform` is what ransacHelper returned (simA's points onto simB's) and comes back inverted,
// as the reference leaves it; reverseWarp = simB warped back onto simA, blended = simA * 0.5 + reverseWarp * 0.5.
inline void registerAndBlend(const micv_shim::Mat &simA, const micv_shim::Mat &simB, micv_shim::Mat &transform,
                             micv_shim::Mat &reverseWarp, micv_shim::Mat &blended) {
    const int depth = micv_cv::depth_of(simA, "registerAndBlend: CV_8UC1 or CV_32FC1 expected");
    micv_shim::require(simB.type() == simA.type() && simB.rows == simA.rows && simB.cols == simA.cols,
                       "registerAndBlend: sizes or types differ");
    float m[6];
    micv_cv::transform_of(transform, m, "registerAndBlend: 2 x 3 CV_32F expected");
    micv_shim::Mat w, o;
    w.create(simA.rows, simA.cols, simA.type());
    o.create(simA.rows, simA.cols, simA.type());
    micv_shim::check(micv_register_blend_host(micv_shim::context(), simA.data, simA.step, simB.data, simB.step, depth, simA.rows,
                                              simA.cols, m, w.data, w.step, o.data, o.step));
    micv_cv::invertAffineTransform(transform, transform);
    reverseWarp = w;
    blended = o;
}
}  // namespace sol
