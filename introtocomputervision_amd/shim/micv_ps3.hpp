// micv_ps3.hpp -- what the ps3 driver does after the geometry (ProblemSets/ps3_cpp/src/Solution.cpp), without OpenCV, twice:
//   drawEpipolarLines (:122-158), runProblem2 (:323-368), runExtraCredit (:370-481)
//                    the reference's functions as written: the end points on this thread in float, cv::line restated as
//                    line_wide below.  With line_wide these host loops are the statement of the contract of the
//                    "ps3: driver" block of include/mi_cv.h (parity with OpenCV's rasteriser unpinned);
//   ...Device        the same pictures from the library: drawEpipolarLinesDevice hands the end points to
//                    micv_draw_epipolar_lines_host, runProblem2Device and runExtraCreditDevice paint both pictures with ONE
//                    call of micv_ps3_epipolar_display_host, which computes the end points on the device as well.
// The pictures are returned instead of written as PNG; the callers write them through micv_viz::imwrite.
#pragma once

#include <climits>
#include <cmath>
#include <utility>
#include <vector>

#include "micv_geom.hpp"
#include "micv_shim.hpp"

namespace micv_ps3 {

using micv_shim::Mat;
using micv_shim::Scalar;

// cvRound as csrc/draw.hpp states it: half to even; INT_MIN for NaN, +-inf and every value outside int.
inline int cvRound(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return static_cast<int>(std::nearbyint(v));
}

// byte k of a painted pixel: saturate(nearbyint(color[k])), NaN gives 0 (the rule of micv_draw_rectangle_*)
inline unsigned char colourByte(double c) {
    const double v = std::nearbyint(c);
    return !(v > 0) ? 0 : (v > 255 ? 255 : static_cast<unsigned char>(v));
}

// cv::line(img, p1, p2, color), thickness 1, LINE_8, for ANY two int points: micv_viz::line's walk (the ends swapped when
// p1.x > p2.x, major = max(dx, |dy|) with the tie going to x, major + 1 steps, err = major - 2 minor) with its integers as
// wide as they need to be.  micv_viz::line keeps dx, dy and err in int, which overflow from 2^30 on; here the differences
// are long long (below 2^32) and the position of step i comes from the walk's closed form,
//   major coordinate  start +- i,      minor coordinate  start +- (2 minor i + major - 1) div (2 major),
// in __int128 (2 minor i reaches 2^65).  Only the steps whose major coordinate is in the image are visited, at most
// max(rows, cols) of them, so an end point at INT_MIN costs nothing.
inline void line_wide(Mat &img, long long x1, long long y1, long long x2, long long y2, const Scalar &color) {
    if (x1 > x2) {
        std::swap(x1, x2);
        std::swap(y1, y2);
    }
    const long long dx = x2 - x1, dys = y2 - y1, sy = dys < 0 ? -1 : 1, dy = dys < 0 ? -dys : dys;
    const bool steep = dy > dx;
    const long long major = steep ? dy : dx, minor = steep ? dx : dy;
    const long long a = steep ? y1 : x1, s = steep ? sy : 1, len = steep ? img.rows : img.cols;
    long long lo = s > 0 ? -a : a - (len - 1), hi = s > 0 ? len - 1 - a : a;
    if (lo < 0) lo = 0;
    if (hi > major) hi = major;
    const int cn = img.channels() < 4 ? img.channels() : 4;
    for (long long i = lo; i <= hi; i++) {
        const long long m = major == 0 ? 0 : static_cast<long long>((static_cast<__int128>(2 * minor) * i + major - 1) / (2 * major));
        const long long x = steep ? x1 + m : x1 + i, y = steep ? y1 + sy * i : y1 + sy * m;
        if (x < 0 || x >= img.cols || y < 0 || y >= img.rows) continue;
        unsigned char *d = img.ptr<unsigned char>(static_cast<int>(y)) + static_cast<size_t>(x) * img.channels();
        for (int k = 0; k < cn; k++) d[k] = colourByte(color.val[k]);
    }
}

// cv::line(img, Point2f(x1, y1), Point2f(x2, y2), color) for n segments {x1, y1, x2, y2}: the statement of
// micv_draw_segments_*.
inline void drawSegments(Mat &img, const float *segments, int n, const Scalar &color) {
    micv_shim::require(img.depth() == micv_shim::U8, "drawSegments: an 8-bit image expected");
    for (int k = 0; k < n; k++) {
        const float *s = segments + 4 * static_cast<size_t>(k);
        line_wide(img, cvRound(s[0]), cvRound(s[1]), cvRound(s[2]), cvRound(s[3]), color);
    }
}

inline void cross3(const float *a, const float *b, float *c) {  // cv::Mat::cross of CV_32F vectors
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// P_iL and P_iR of the line l on a rows x cols image (:127-145), as include/mi_cv.h ("ps3: geometry") states them:
// the products and differences in float, the scale by the float reciprocal of the third coordinate.
inline void endPoints(const float *l, int rows, int cols, float *out) {
    const float rm1 = static_cast<float>(rows - 1), cm1 = static_cast<float>(cols - 1);
    const float ul[3] = {0, 0, 1}, bl[3] = {0, rm1, 1}, ur[3] = {cm1, 0, 1}, br[3] = {cm1, rm1, 1};
    float IL[3], IR[3], PL[3], PR[3];
    cross3(ul, bl, IL);
    cross3(ur, br, IR);
    cross3(l, IL, PL);
    cross3(l, IR, PR);
    const float rl = static_cast<float>(1.0 / static_cast<double>(PL[2])), rr = static_cast<float>(1.0 / static_cast<double>(PR[2]));
    for (int c = 0; c < 3; c++) {
        out[c] = PL[c] * rl;
        out[3 + c] = PR[c] * rr;
    }
}

inline std::vector<float> endPointsOf(const Mat &img, const Mat &epiLines) {
    micv_shim::require(epiLines.type() == micv_shim::F32 && epiLines.rows == 3, "drawEpipolarLines: 3 x n CV_32F lines expected");
    std::vector<float> e(6 * static_cast<size_t>(epiLines.cols));
    for (int col = 0; col < epiLines.cols; col++) {
        const float l[3] = {epiLines.at<float>(0, col), epiLines.at<float>(1, col), epiLines.at<float>(2, col)};
        endPoints(l, img.rows, img.cols, &e[6 * static_cast<size_t>(col)]);
    }
    return e;
}

// drawEpipolarLines (:122-158) as written.  A vertical line has NaN / inf end points: both x become INT_MIN and nothing
// is drawn.
inline void drawEpipolarLines(Mat &img, const Mat &epiLines, const Scalar color) {
    micv_shim::require(img.depth() == micv_shim::U8, "drawEpipolarLines: an 8-bit image expected");
    const std::vector<float> e = endPointsOf(img, epiLines);
    for (int col = 0; col < epiLines.cols; col++) {
        const float *p = &e[6 * static_cast<size_t>(col)];
        line_wide(img, cvRound(p[0]), cvRound(p[1]), cvRound(p[3]), cvRound(p[4]), color);
    }
}

// The same picture from micv_draw_epipolar_lines_host: one launch for all lines.
inline void drawEpipolarLinesDevice(Mat &img, const Mat &epiLines, const Scalar color) {
    micv_shim::require(img.depth() == micv_shim::U8, "drawEpipolarLines: an 8-bit image expected");
    const std::vector<float> e = endPointsOf(img, epiLines);
    micv_shim::check(micv_draw_epipolar_lines_host(micv_shim::context(), img.data, img.rows, img.cols, img.channels(), img.step, e.data(),
                                                   epiLines.cols, color.val));
}

// linesA = (ptsB^T F)^T and linesB = F ptsA (:341-353), 3 x n each: a double chain per element, one rounding
// (include/mi_cv.h, "ps3: geometry": epipolar end points).
inline std::pair<Mat, Mat> epipolarLines(const Mat &fMat, const Mat &ptsA, const Mat &ptsB) {
    const std::vector<float> F = micv_geom::flat(fMat, 9, "epipolarLines: 3 x 3 CV_32F expected");
    micv_shim::require(ptsA.type() == micv_shim::F32 && ptsB.type() == micv_shim::F32 && ptsA.rows == 2 && ptsB.rows == 2 &&
                           ptsA.cols == ptsB.cols,
                       "epipolarLines: two 2 x n CV_32F point sets expected");
    Mat linesA(3, ptsA.cols, micv_shim::F32), linesB(3, ptsA.cols, micv_shim::F32);
    for (int i = 0; i < ptsA.cols; i++)
        for (int c = 0; c < 3; c++) {
            double x = ptsB.at<float>(0, i), y = ptsB.at<float>(1, i);
            double s = x * static_cast<double>(F[c]);
            s = s + y * static_cast<double>(F[3 + c]);
            s = s + 1.0 * static_cast<double>(F[6 + c]);
            linesA.at<float>(c, i) = static_cast<float>(s);
            x = ptsA.at<float>(0, i), y = ptsA.at<float>(1, i);
            s = static_cast<double>(F[3 * c]) * x;
            s = s + static_cast<double>(F[3 * c + 1]) * y;
            s = s + static_cast<double>(F[3 * c + 2]) * 1.0;
            linesB.at<float>(c, i) = static_cast<float>(s);
        }
    return std::make_pair(linesA, linesB);
}

inline const Scalar kLineColor(0, 255, 0, 0);  // CV_RGB(0, 0xFF, 0), :360-361, :472-473

struct Problem2 {
    Mat fMatEst, fMat, picA, picB;  // part a, part b, ps3-2-c-1, ps3-2-c-2
};
struct ExtraCredit {
    micv_geom::Normalized n;  // T_a, T_b, F_Hat, F
    Mat picA, picB;           // ps3-2-e-1, ps3-2-e-2
};

inline Mat estimate(const Mat &ptsA, const Mat &ptsB) {
    const std::vector<float> f = micv_geom::flat(fundamental::solveLeastSquares(ptsA, ptsB), 9, "fundamental::solveLeastSquares: 9 x 1");
    return micv_geom::mat3(f.data());  // fMatEst.reshape(0, 3)
}

// part c / part e on this thread (:341-363)
inline void display(const Mat &F, const Mat &ptsA, const Mat &ptsB, const Mat &imgA, const Mat &imgB, Mat &picA, Mat &picB) {
    const std::pair<Mat, Mat> lines = epipolarLines(F, ptsA, ptsB);
    picA = imgA.clone();
    picB = imgB.clone();
    drawEpipolarLines(picA, lines.first, kLineColor);
    drawEpipolarLines(picB, lines.second, kLineColor);
}

// part c / part e in one library call: one launch over (image, line)
inline void displayDevice(const Mat &F, const Mat &ptsA, const Mat &ptsB, const Mat &imgA, const Mat &imgB, Mat &picA, Mat &picB) {
    const std::vector<float> f = micv_geom::flat(F, 9, "display: 3 x 3 CV_32F expected"),
                             a = micv_geom::rows_of(ptsA, 2, "display: 2 x n CV_32F expected"),
                             b = micv_geom::rows_of(ptsB, 2, "display: 2 x n CV_32F expected");
    micv_shim::require(ptsA.cols == ptsB.cols && imgA.type() == imgB.type() && imgA.depth() == micv_shim::U8,
                       "display: point sets of one size and 8-bit pictures of one type expected");
    picA = Mat(imgA.rows, imgA.cols, imgA.type());
    picB = Mat(imgB.rows, imgB.cols, imgB.type());
    micv_shim::check(micv_ps3_epipolar_display_host(micv_shim::context(), f.data(), a.data(), b.data(), ptsA.cols, imgA.data, imgA.step,
                                                    imgA.rows, imgA.cols, imgB.data, imgB.step, imgB.rows, imgB.cols, imgA.channels(), 0,
                                                    kLineColor.val, picA.data, picA.step, picB.data, picB.step, nullptr));
}

inline Problem2 runProblem2(const Mat &ptsA, const Mat &ptsB, const Mat &imgA, const Mat &imgB) {
    Problem2 r;
    r.fMatEst = estimate(ptsA, ptsB);
    r.fMat = fundamental::rankReduce(r.fMatEst);
    display(r.fMat, ptsA, ptsB, imgA, imgB, r.picA, r.picB);
    return r;
}
inline Problem2 runProblem2Device(const Mat &ptsA, const Mat &ptsB, const Mat &imgA, const Mat &imgB) {
    Problem2 r;
    r.fMatEst = estimate(ptsA, ptsB);
    r.fMat = fundamental::rankReduce(r.fMatEst);
    displayDevice(r.fMat, ptsA, ptsB, imgA, imgB, r.picA, r.picB);
    return r;
}

inline ExtraCredit runExtraCredit(const Mat &ptsA, const Mat &ptsB, const Mat &imgA, const Mat &imgB) {
    ExtraCredit r;
    r.n = micv_geom::normalizedFundamental(ptsA, ptsB);
    display(r.n.F, ptsA, ptsB, imgA, imgB, r.picA, r.picB);
    return r;
}
inline ExtraCredit runExtraCreditDevice(const Mat &ptsA, const Mat &ptsB, const Mat &imgA, const Mat &imgB) {
    ExtraCredit r;
    r.n = micv_geom::normalizedFundamental(ptsA, ptsB);
    displayDevice(r.n.F, ptsA, ptsB, imgA, imgB, r.picA, r.picB);
    return r;
}

}  // namespace micv_ps3
