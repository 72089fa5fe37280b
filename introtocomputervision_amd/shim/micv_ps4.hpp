// micv_ps4.hpp -- what the ps4 driver (ProblemSets/ps4_cpp/src/Solution.cpp) writes out between harris::, sift::, the
// matcher and ransac::, without OpenCV, twice:
//   * as host loops (drawDots, hconcat, drawKeypoints, drawMatchLines, consensusMask): the STATEMENT OF THE CONTRACT of
//     the "ps4: driver" block of include/mi_cv.h.  They need nothing but this header's includes and no library call, so
//     they can be compiled and run on their own (tests/test_ps4_driver_shim.py does, under the address sanitizer);
//   * as harrisHelper / siftHelper / ransacHelper over them, and harrisHelperDevice / siftHelperDevice /
//     ransacHelperDevice beside them, which hand the same work to the library's one-call forms and write the same files.
// Reference: drawDots :59-69, harrisHelper :71-132, siftHelper :134-211, ransacHelper :213-253.
// The reference delegates the pixel work to OpenCV 3.4.1, whose source is not available here; what is restated is a
// decision of this library, PARITY UNPINNED (DESIGN.md sections 2 and 3):
//   * cv::drawKeypoints(.., Scalar::all(-1), DRAW_RICH_KEYPOINTS): per keypoint a colour Scalar(rng(256), rng(256),
//     rng(256)) from cv::theRNG(), a circle of radius cvRound(size / 2) around (cvRound(x), cvRound(y)) and, unless
//     angle == -1, a stroke to centre + (cvRound(cos * radius), cvRound(sin * radius)).  OpenCV draws both anti-aliased
//     in 1/16-pixel fixed point; here they are 8-connected: cv::circle's thickness-1 midpoint walk and micv_viz::line.
//     The sine and cosine are the fixed polynomial of the library's descriptor window (sincos_deg below);
//   * cv::Scalar(rng.., rng.., rng..): the reference's toolchain evaluates the arguments right to left, so the FIRST draw
//     is the third entry (R) and the third draw the first (B);
//   * rng.uniform(0, 255) is next() % 255; rng(256) is next() % 256; cv::RNG is multiply-with-carry, a = 4164903690.
#pragma once

#include <cmath>
#include <cstdint>
#include <tuple>
#include <vector>

#include "micv_config.hpp"
#include "micv_viz.hpp"
#include "micv_warp.hpp"

namespace micv_ps4 {

using micv_shim::KeyPoint;
using micv_shim::Mat;
using micv_viz::Point;

// ---- cv::RNG -------------------------------------------------------------------------------------------------------
struct RNG {
    uint64_t state;
    explicit RNG(uint64_t seed = 0xffffffffull) : state(seed ? seed : 0xffffffffull) {}
    unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690u + (state >> 32);
        return (unsigned)state;
    }
};
struct Colour {
    unsigned char b, g, r;
};
// Scalar(rng % m, rng % m, rng % m), arguments evaluated right to left
inline Colour random_colour(RNG &rng, unsigned m) {
    Colour c;
    c.r = (unsigned char)(rng.next() % m);
    c.g = (unsigned char)(rng.next() % m);
    c.b = (unsigned char)(rng.next() % m);
    return c;
}

// ---- rounding ------------------------------------------------------------------------------------------------------
inline bool coord_ok(float v) { return std::fabs(v) < 1e9f; }  // false for NaN and inf: such a stroke draws nothing
inline long long round_even(float v) { return (long long)std::rint((double)v); }  // cvRound: half to even
// saturate_cast<uchar>(cvRound(v)) as the library converts a float image (micv_gray_to_rgb8_*)
inline unsigned char f32_to_u8(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return 0;
    const long long r = round_even(v);
    return (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// sin / cos of `deg` degrees: the polynomial of the library's descriptor window, operation for operation
inline void sincos_deg(float deg, float &s, float &c) {
    float t = deg / 360.f;
    t = t - std::floor(t);
    const float x = t * 4.f;
    int q = (int)x;
    const float f = x - (float)q;
    q &= 3;
    const float y = f * 1.57079632679489662f, y2 = y * y;
    float ps = -2.50521083854417188e-8f;
    ps = std::fmaf(ps, y2, 2.75573192239858907e-6f);
    ps = std::fmaf(ps, y2, -1.98412698412698413e-4f);
    ps = std::fmaf(ps, y2, 8.33333333333333333e-3f);
    ps = std::fmaf(ps, y2, -1.66666666666666667e-1f);
    ps = std::fmaf(ps, y2, 1.f);
    const float sy = ps * y;
    float pc = 2.08767569878680990e-9f;
    pc = std::fmaf(pc, y2, -2.75573192239858907e-7f);
    pc = std::fmaf(pc, y2, 2.48015873015873016e-5f);
    pc = std::fmaf(pc, y2, -1.38888888888888889e-3f);
    pc = std::fmaf(pc, y2, 4.16666666666666667e-2f);
    pc = std::fmaf(pc, y2, -0.5f);
    pc = std::fmaf(pc, y2, 1.f);
    switch (q) {
        case 0: s = sy; c = pc; break;
        case 1: s = pc; c = -sy; break;
        case 2: s = -sy; c = -pc; break;
        default: s = -pc; c = sy; break;
    }
}

// ---- pixels: a window [x0, x0 + cols) of a BGR canvas, coordinates relative to the window --------------------------
struct Window {
    Mat *img;
    int x0, cols;
};
inline void put(const Window &w, long long x, long long y, Colour c) {
    if (x < 0 || x >= w.cols || y < 0 || y >= w.img->rows) return;
    unsigned char *d = w.img->ptr<unsigned char>((int)y) + 3 * ((size_t)w.x0 + (size_t)x);
    d[0] = c.b;
    d[1] = c.g;
    d[2] = c.r;
}
// micv_viz::line's walk in 64-bit coordinates; only the steps that can lie inside the window are visited
inline void line(const Window &w, long long x1, long long y1, long long x2, long long y2, Colour c) {
    if (x1 > x2) {
        std::swap(x1, x2);
        std::swap(y1, y2);
    }
    const long long dx = x2 - x1, dys = y2 - y1, sy = dys < 0 ? -1 : 1, dy = dys < 0 ? -dys : dys;
    const bool steep = dy > dx;
    const long long major = steep ? dy : dx, minor = steep ? dx : dy;
    if (major > 200000) {  // a stroke far longer than any image: the closed form of the walk over the in-window steps
        long long lo = !steep ? -x1 : (sy > 0 ? -y1 : y1 - (w.img->rows - 1));
        long long hi = !steep ? w.cols - 1 - x1 : (sy > 0 ? w.img->rows - 1 - y1 : y1);
        lo = std::max(lo, 0ll);
        hi = std::min(hi, major);
        for (long long i = lo; i <= hi; i++) {
            const long long m = (2 * minor * i + major - 1) / (2 * major);
            put(w, steep ? x1 + m : x1 + i, steep ? y1 + sy * i : y1 + sy * m, c);
        }
        return;
    }
    long long err = major - 2 * minor, x = x1, y = y1;
    for (long long i = 0; i <= major; i++) {
        put(w, x, y, c);
        const bool both = err < 0;
        err += both ? 2 * major - 2 * minor : -2 * minor;
        if (steep) { y += sy; if (both) x += 1; }
        else { x += 1; if (both) y += sy; }
    }
}
// cv::circle, thickness 1: the midpoint walk (as sol::drawCircles / micv_draw_circles_*)
inline void circle(const Window &w, long long cx, long long cy, long long radius, Colour c) {
    long long err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        put(w, cx + dx, cy + dy, c); put(w, cx - dx, cy + dy, c); put(w, cx + dx, cy - dy, c); put(w, cx - dx, cy - dy, c);
        put(w, cx + dy, cy + dx, c); put(w, cx - dy, cy + dx, c); put(w, cx + dy, cy - dx, c); put(w, cx - dy, cy - dx, c);
        dy++;
        err += plus;
        plus += 2;
        const long long mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// ---- the host loops -------------------------------------------------------------------------------------------------

// cv::normalize(src, dst, 0, 255, NORM_MINMAX, CV_8U) as micv_normalize_minmax_* states it: NaNs do not take part in the
// range and give 0; no value at all gives zeros.
inline Mat normalize_u8(const Mat &src) {
    micv_shim::require(src.type() == micv_shim::F32, "normalize: CV_32FC1 expected");
    float lo = 0, hi = 0;
    bool any = false;
    for (int y = 0; y < src.rows; y++)
        for (int x = 0; x < src.cols; x++) {
            const float t = src.at<float>(y, x);
            if (t != t) continue;
            if (!any || t < lo) lo = t;
            if (!any || t > hi) hi = t;
            any = true;
        }
    float a = 0.f, b = 0.f;
    if (any) {
        const double dlo = lo, dhi = hi;
        const double scale = 255.0 * (dhi - dlo > DBL_EPSILON ? 1.0 / (dhi - dlo) : 0.0), shift = 0.0 - dlo * scale;
        a = (float)scale;
        b = (float)shift;
    }
    Mat dst(src.rows, src.cols, micv::CV_8UC1);
    for (int y = 0; y < src.rows; y++)
        for (int x = 0; x < src.cols; x++) {
            const float t = src.at<float>(y, x) * a + b;
            const float r = std::fmin(std::fmax(std::rint(t), 0.f), 255.f);
            dst.at<unsigned char>(y, x) = std::isfinite(t) ? (unsigned char)(int)r : (unsigned char)0;
        }
    return dst;
}

// drawDots (Solution.cpp:59-69): img CV_32FC1 or CV_8UC1, mask the CV_32FC1 corner map
inline void drawDots(const Mat &mask, const Mat &img, Mat &dottedImg) {
    micv_shim::require(mask.type() == micv_shim::F32 && (img.type() == micv_shim::F32 || img.type() == micv::CV_8UC1) &&
                           mask.rows == img.rows && mask.cols == img.cols,
                       "drawDots: a grey image and a CV_32FC1 map of its size expected");
    const Mat maskNorm = normalize_u8(mask);
    Mat out(img.rows, img.cols, micv::CV_8UC3);
    for (int y = 0; y < img.rows; y++)
        for (int x = 0; x < img.cols; x++) {
            const unsigned char v = img.type() == micv_shim::F32 ? f32_to_u8(img.at<float>(y, x)) : img.at<unsigned char>(y, x);
            unsigned char *d = out.ptr<unsigned char>(y) + 3 * x;
            if (maskNorm.at<unsigned char>(y, x)) { d[0] = 0; d[1] = 0; d[2] = 255; }
            else d[0] = d[1] = d[2] = v;
        }
    dottedImg = out;
}

// cv::hconcat of two 8-bit images of equal rows and channels
inline void hconcat(const Mat &a, const Mat &b, Mat &dst) {
    micv_shim::require(a.rows == b.rows && a.type() == b.type() && a.depth() == micv_shim::U8, "hconcat: two 8-bit images of equal rows expected");
    Mat out(a.rows, a.cols + b.cols, a.type());
    const size_t ab = (size_t)a.cols * a.elemSize(), bb = (size_t)b.cols * b.elemSize();
    for (int y = 0; y < a.rows; y++) {
        std::memcpy(out.ptr<unsigned char>(y), a.ptr<unsigned char>(y), ab);
        std::memcpy(out.ptr<unsigned char>(y) + ab, b.ptr<unsigned char>(y), bb);
    }
    dst = out;
}

inline Mat to_bgr(const Mat &img) {
    micv_shim::require(img.depth() == micv_shim::U8 && (img.channels() == 1 || img.channels() == 3), "8-bit image of 1 or 3 channels expected");
    return img.channels() == 3 ? img.clone() : micv_viz::gray2rgb(img);
}

// The glyphs of cv::drawKeypoints on the window [x0, x0 + cols) of a BGR canvas, clipped to it; rng goes on.
inline void drawKeypointGlyphs(Mat &canvas, int x0, int cols, const std::vector<KeyPoint> &keypoints, RNG &rng) {
    micv_shim::require(canvas.type() == micv::CV_8UC3 && x0 >= 0 && cols > 0 && x0 + cols <= canvas.cols, "drawKeypoints: a window of a BGR canvas expected");
    const Window w{&canvas, x0, cols};
    for (const KeyPoint &p : keypoints) {
        const Colour c = random_colour(rng, 256);  // (every keypoint draws its colour, whether it paints or not)
        const float half = p.size * 0.5f;
        if (!coord_ok(p.pt.x) || !coord_ok(p.pt.y) || !(half >= 0.f && half <= 32767.f)) continue;
        const long long cx = round_even(p.pt.x), cy = round_even(p.pt.y), radius = round_even(half);
        circle(w, cx, cy, radius, c);
        if (p.angle != -1.f && std::fabs(p.angle) < 1e9f) {
            float s, co;
            sincos_deg(p.angle, s, co);
            line(w, cx, cy, cx + round_even(co * (float)radius), cy + round_even(s * (float)radius), c);
        }
    }
}
// cv::drawKeypoints(image, keypoints, outImage, Scalar::all(-1), DRAW_RICH_KEYPOINTS)
inline void drawKeypoints(const Mat &image, const std::vector<KeyPoint> &keypoints, Mat &outImage, RNG &rng) {
    Mat out = to_bgr(image);
    drawKeypointGlyphs(out, 0, out.cols, keypoints, rng);
    outImage = out;
}

// The lines of siftHelper (:194-205) and, with a mask, of ransacHelper (:243-249) on a BGR canvas: match i is drawn iff
// mask is NULL or mask[i]; a match whose index names no keypoint is skipped together with its draws.
inline void drawMatchLines(Mat &canvas, const std::vector<KeyPoint> &kpA, const std::vector<KeyPoint> &kpB,
                           const std::vector<std::pair<int, int>> &matches, const std::vector<unsigned char> *mask, int xOffset,
                           uint64_t seed = 12345) {
    micv_shim::require(canvas.type() == micv::CV_8UC3 && (!mask || mask->size() >= matches.size()), "drawMatchLines: a BGR canvas expected");
    const Window w{&canvas, 0, canvas.cols};
    RNG rng(seed);
    for (size_t i = 0; i < matches.size(); i++) {
        const int q = matches[i].first, t = matches[i].second;
        if ((mask && !(*mask)[i]) || q < 0 || (size_t)q >= kpA.size() || t < 0 || (size_t)t >= kpB.size()) continue;
        const Colour c = random_colour(rng, 255);
        const float x1 = kpA[q].pt.x, y1 = kpA[q].pt.y, x2 = kpB[t].pt.x + (float)xOffset, y2 = kpB[t].pt.y;
        if (!coord_ok(x1) || !coord_ok(y1) || !coord_ok(x2) || !coord_ok(y2)) continue;
        line(w, round_even(x1), round_even(y1), round_even(x2), round_even(y2), c);
    }
}

// ransacHelper draws `for idx : consensusSet` with idx indexing the UNSHUFFLED point arrays (Solution.cpp:244-248), though
// the set holds positions in the shuffled index vector (RANSAC.cpp:122-134): the as-written picture marks those positions.
inline std::vector<unsigned char> consensusMask(size_t n, const std::vector<int> &consensusSet) {
    std::vector<unsigned char> mask(n, 0);
    for (int idx : consensusSet)
        if (idx >= 0 && (size_t)idx < n) mask[idx] = 1;
    return mask;
}

#ifndef MICV_PS4_HOST_LOOPS_ONLY
// ---- the driver's helpers -------------------------------------------------------------------------------------------

// FeaturesContainer (Solution.h): the image, its Harris settings, what the helpers leave behind and the file names
struct FeaturesContainer {
    Mat input;  // CV_8UC1
    micv_config::Harris config;
    bool useGpu = true;
    std::string outPrefix, gradImgPath, crImgPath, cornersImgPath, keypointsImgPath, matchesImgPath;
    Mat gradientX, gradientY, cornerResponse, corners;
    std::vector<std::pair<int, int>> cornerLocs;
    std::vector<KeyPoint> keypoints;
    std::vector<std::pair<int, int>> goodMatches;
    FeaturesContainer(const Mat &img, const micv_config::Harris &h, bool gpu, const std::string &prefix, const std::string &stem)
        : input(img), config(h), useGpu(gpu), outPrefix(prefix), gradImgPath("/" + stem + "-gradients.pgm"),
          crImgPath("/" + stem + "-response.pgm"), cornersImgPath("/" + stem + "-corners.ppm"),
          keypointsImgPath("/" + stem + "-keypoints.ppm"), matchesImgPath("/" + stem + "-matches.ppm") {}
};

inline std::vector<float> flat_keypoints(const std::vector<KeyPoint> &kp) {
    std::vector<float> out(kp.size() * 4 + 4);
    for (size_t i = 0; i < kp.size(); i++) {
        out[4 * i] = kp[i].pt.x; out[4 * i + 1] = kp[i].pt.y; out[4 * i + 2] = kp[i].size; out[4 * i + 3] = kp[i].angle;
    }
    return out;
}
inline std::vector<int32_t> flat_matches(const std::vector<std::pair<int, int>> &m) {
    std::vector<int32_t> out(m.size() * 2 + 2);
    for (size_t i = 0; i < m.size(); i++) {
        out[2 * i] = m[i].first; out[2 * i + 1] = m[i].second;
    }
    return out;
}

// harrisHelper (Solution.cpp:71-132) with the pictures made by the loops above
inline void harrisHelper(FeaturesContainer &conf) {
    const Mat input = micv_shim::to_f32(conf.input);
    harris::getGradients(input, conf.config.sobel_kernel_size, conf.gradientX, conf.gradientY);
    Mat gradCombined;
    hconcat(normalize_u8(conf.gradientX), normalize_u8(conf.gradientY), gradCombined);
    micv_viz::imwrite(conf.outPrefix + conf.gradImgPath, gradCombined);
    if (conf.useGpu) harris::gpu::getCornerResponse(conf.gradientX, conf.gradientY, conf.config.window_size, conf.config.gaussian_sigma, conf.config.alpha, conf.cornerResponse);
    else harris::cpu::getCornerResponse(conf.gradientX, conf.gradientY, conf.config.window_size, conf.config.gaussian_sigma, conf.config.alpha, conf.cornerResponse);
    micv_viz::imwrite(conf.outPrefix + conf.crImgPath, normalize_u8(conf.cornerResponse));
    conf.cornerLocs.clear();
    harris::gpu::refineCorners(conf.cornerResponse, conf.config.response_threshold, conf.config.min_distance, conf.corners, conf.cornerLocs);
    Mat dottedImg;
    drawDots(conf.corners, input, dottedImg);
    micv_viz::imwrite(conf.outPrefix + conf.cornersImgPath, dottedImg);
}

// harrisHelper as ONE library call (micv_ps4_harris_display_host): same container contents, same files
inline void harrisHelperDevice(FeaturesContainer &conf) {
    const Mat input = micv_shim::to_f32(conf.input);
    const int rows = input.rows, cols = input.cols;
    const size_t n = (size_t)rows * cols;
    std::vector<float> fields(4 * n);
    std::vector<int32_t> locs(2 * n);
    int64_t count = 0;
    Mat grad(rows, 2 * cols, micv::CV_8UC1), resp(rows, cols, micv::CV_8UC1), dots(rows, cols, micv::CV_8UC3);
    micv_shim::check(micv_ps4_harris_display_host(micv_shim::context(), input.ptr<float>(), rows, cols, input.step, conf.config.sobel_kernel_size,
                                                  (int)conf.config.window_size, conf.config.gaussian_sigma, conf.config.alpha,
                                                  conf.useGpu ? 0 : MICV_HARRIS_CPU, conf.config.response_threshold, conf.config.min_distance,
                                                  fields.data(), locs.data(), (int64_t)n, &count, grad.data, grad.step, resp.data, resp.step,
                                                  dots.data, dots.step));
    Mat *out[4] = {&conf.gradientX, &conf.gradientY, &conf.cornerResponse, &conf.corners};
    for (int k = 0; k < 4; k++) *out[k] = Mat(rows, cols, micv_shim::F32, fields.data() + k * n).clone();
    conf.cornerLocs.clear();
    for (int64_t i = 0; i < count; i++) conf.cornerLocs.emplace_back(locs[2 * i], locs[2 * i + 1]);
    micv_viz::imwrite(conf.outPrefix + conf.gradImgPath, grad);
    micv_viz::imwrite(conf.outPrefix + conf.crImgPath, resp);
    micv_viz::imwrite(conf.outPrefix + conf.cornersImgPath, dots);
}

// The computing part of harrisHelper on the 8-bit picture itself: gradientX, gradientY, cornerResponse, corners and
// cornerLocs from conf.input (CV_8UC1; an ROI with a foreign step is fine) with ONE micv_harris_corners_u8_host call --
// 1 B per pixel goes up, and there is no convertTo(CV_32F).  Same container contents as harrisHelper's three calls.
inline void harrisCorners8(FeaturesContainer &conf) {
    const Mat &input = conf.input;
    if (input.type() != micv::CV_8UC1) throw std::invalid_argument("harrisCorners8: CV_8UC1 expected");
    const int rows = input.rows, cols = input.cols;
    const size_t n = (size_t)rows * cols;
    Mat gx(rows, cols, micv_shim::F32), gy(rows, cols, micv_shim::F32), resp(rows, cols, micv_shim::F32), corners(rows, cols, micv_shim::F32);
    std::vector<int32_t> locs(2 * n);
    int64_t count = 0;
    micv_shim::check(micv_harris_corners_u8_host(micv_shim::context(), input.ptr<uint8_t>(), rows, cols, input.step, conf.config.sobel_kernel_size,
                                                 (int)conf.config.window_size, conf.config.gaussian_sigma, conf.config.alpha,
                                                 conf.useGpu ? 0 : MICV_HARRIS_CPU, conf.config.response_threshold, conf.config.min_distance,
                                                 gx.ptr<float>(), gy.ptr<float>(), gx.step, resp.ptr<float>(), resp.step, corners.ptr<float>(),
                                                 corners.step, locs.data(), (int64_t)n, &count, 0.f, nullptr));
    conf.gradientX = gx;
    conf.gradientY = gy;
    conf.cornerResponse = resp;
    conf.corners = corners;
    conf.cornerLocs.clear();
    for (int64_t i = 0; i < count; i++) conf.cornerLocs.emplace_back(locs[2 * i], locs[2 * i + 1]);
}

// The descriptor step of siftHelper (Solution.cpp:166-169) on the 8-bit picture itself: desc = keypoints.size() x 128 F32
// from img8 (CV_8UC1; an ROI with a foreign step is fine) with ONE micv_sift_descriptors_u8_host call -- 1 B per pixel goes
// up and no gradient Mat is needed.  Same bytes as sift::computeDescriptors on harris::getGradients(img8 as F32, 3).
inline void siftDescriptors8(const Mat &img8, const std::vector<KeyPoint> &keypoints, Mat &desc) {
    if (img8.type() != micv::CV_8UC1) throw std::invalid_argument("siftDescriptors8: CV_8UC1 expected");
    const std::vector<float> kp = flat_keypoints(keypoints);
    Mat out(static_cast<int>(keypoints.size()), 128, micv_shim::F32);
    if (!keypoints.empty())
        micv_shim::check(micv_sift_descriptors_u8_host(micv_shim::context(), img8.ptr<uint8_t>(), img8.rows, img8.cols, img8.step, kp.data(),
                                                       static_cast<int64_t>(keypoints.size()), out.ptr<float>(), out.step));
    desc = out;
}

// siftHelper's computing steps (Solution.cpp:141-144, :166-186), shared by the two forms below
inline void siftCompute(FeaturesContainer &img1, FeaturesContainer &img2) {
    constexpr size_t SIFT_WINDOW_SIZE = 10;
    sift::getKeypoints(img1.gradientX, img1.gradientY, img1.cornerLocs, SIFT_WINDOW_SIZE, img1.keypoints);
    sift::getKeypoints(img2.gradientX, img2.gradientY, img2.cornerLocs, SIFT_WINDOW_SIZE, img2.keypoints);
    Mat d1, d2;
    sift::computeDescriptors(img1.gradientX, img1.gradientY, img1.keypoints, d1);
    sift::computeDescriptors(img2.gradientX, img2.gradientY, img2.keypoints, d2);
    std::vector<float> distances;
    img1.goodMatches.clear();
    if (d1.rows > 0 && d2.rows >= 2) sol::matchDescriptors(d1, d2, 0.75, img1.goodMatches, distances);
    img2.goodMatches = img1.goodMatches;
}

// siftHelper (Solution.cpp:134-211); rngState is cv::theRNG()'s word (0 at the start of a process)
inline void siftHelper(FeaturesContainer &img1, FeaturesContainer &img2, uint64_t &rngState) {
    siftCompute(img1, img2);
    RNG rng(rngState);
    Mat drawn1, drawn2, keypointsCombined;
    drawKeypoints(img1.input, img1.keypoints, drawn1, rng);
    drawKeypoints(img2.input, img2.keypoints, drawn2, rng);
    rngState = rng.state;
    hconcat(drawn1, drawn2, keypointsCombined);
    micv_viz::imwrite(img1.outPrefix + img1.keypointsImgPath, keypointsCombined);
    Mat combinedSrc = keypointsCombined.clone();
    drawMatchLines(combinedSrc, img1.keypoints, img2.keypoints, img1.goodMatches, nullptr, drawn1.cols);
    micv_viz::imwrite(img1.outPrefix + img1.matchesImgPath, combinedSrc);
}

inline void match_panels(const FeaturesContainer &img1, const FeaturesContainer &img2, const std::vector<unsigned char> *mask, int flags,
                         uint64_t &rngState, Mat *keypointPanel, Mat &matchPanel) {
    micv_shim::require(img1.input.type() == micv::CV_8UC1 && img2.input.type() == micv::CV_8UC1 && img1.input.rows == img2.input.rows,
                       "ps4: two CV_8UC1 images of equal rows expected");
    const int rows = img1.input.rows, cols = img1.input.cols + img2.input.cols;
    const std::vector<float> ka = flat_keypoints(img1.keypoints), kb = flat_keypoints(img2.keypoints);
    const std::vector<int32_t> m = flat_matches(img1.goodMatches);
    if (keypointPanel) keypointPanel->create(rows, cols, micv::CV_8UC3);
    matchPanel.create(rows, cols, micv::CV_8UC3);
    micv_shim::check(micv_ps4_match_panels_host(micv_shim::context(), img1.input.data, img1.input.step, img1.input.cols, img2.input.data,
                                                img2.input.step, img2.input.cols, rows, ka.data(), (int64_t)img1.keypoints.size(), kb.data(),
                                                (int64_t)img2.keypoints.size(), m.data(), (int64_t)img1.goodMatches.size(),
                                                mask ? mask->data() : nullptr, flags, 12345, &rngState,
                                                keypointPanel ? keypointPanel->data : nullptr, matchPanel.data, matchPanel.step));
}

// siftHelper with both pictures from ONE library call (micv_ps4_match_panels_host): same files
inline void siftHelperDevice(FeaturesContainer &img1, FeaturesContainer &img2, uint64_t &rngState) {
    siftCompute(img1, img2);
    Mat keypointsCombined, combinedSrc;
    match_panels(img1, img2, nullptr, 0, rngState, &keypointsCombined, combinedSrc);
    micv_viz::imwrite(img1.outPrefix + img1.keypointsImgPath, keypointsCombined);
    micv_viz::imwrite(img1.outPrefix + img1.matchesImgPath, combinedSrc);
}

using RansacResult = std::tuple<Mat, std::vector<int>, double>;

// ransacHelper's solve (Solution.cpp:220-235)
inline RansacResult ransacSolve(const FeaturesContainer &img1, const FeaturesContainer &img2, ransac::TransformType whichRansac,
                                const micv_config::RANSAC &settings) {
    std::vector<micv_shim::Point2f> a, b;
    for (const auto &match : img1.goodMatches) {
        a.push_back(img1.keypoints[match.first].pt);
        b.push_back(img2.keypoints[match.second].pt);
    }
    return ransac::solve(a, b, whichRansac, settings.reprojection_threshold, settings.max_iterations, settings.consensus_ratio);
}
// ransacHelper's picture (Solution.cpp:239-250) from a solve's consensus set, by the loops above ...
inline void drawConsensus(const FeaturesContainer &img1, const FeaturesContainer &img2, const std::vector<int> &consensusSet,
                          const std::string &path) {
    Mat combinedSrc;
    hconcat(to_bgr(img1.input), to_bgr(img2.input), combinedSrc);
    const std::vector<unsigned char> mask = consensusMask(img1.goodMatches.size(), consensusSet);
    drawMatchLines(combinedSrc, img1.keypoints, img2.keypoints, img1.goodMatches, &mask, img1.input.cols);
    micv_viz::imwrite(path, combinedSrc);
}
// ... and by the library (MICV_PS4_NO_GLYPHS): same file
inline void drawConsensusDevice(const FeaturesContainer &img1, const FeaturesContainer &img2, const std::vector<int> &consensusSet,
                                const std::string &path) {
    const std::vector<unsigned char> mask = consensusMask(img1.goodMatches.size() + 1, consensusSet);
    Mat combinedSrc;
    uint64_t unused = 0;
    match_panels(img1, img2, &mask, MICV_PS4_NO_GLYPHS, unused, nullptr, combinedSrc);
    micv_viz::imwrite(path, combinedSrc);
}
inline RansacResult ransacHelper(FeaturesContainer &img1, FeaturesContainer &img2, ransac::TransformType whichRansac,
                                 const micv_config::RANSAC &settings, const std::string &path) {
    RansacResult r = ransacSolve(img1, img2, whichRansac, settings);
    drawConsensus(img1, img2, std::get<1>(r), path);
    return r;
}
inline RansacResult ransacHelperDevice(FeaturesContainer &img1, FeaturesContainer &img2, ransac::TransformType whichRansac,
                                       const micv_config::RANSAC &settings, const std::string &path) {
    RansacResult r = ransacSolve(img1, img2, whichRansac, settings);
    drawConsensusDevice(img1, img2, std::get<1>(r), path);
    return r;
}
#endif  // MICV_PS4_HOST_LOOPS_ONLY

}  // namespace micv_ps4
