// micv_ps0.hpp -- ps0 of the reference (ProblemSets/ps0_cpp/main.cpp) without OpenCV, twice:
//   swapRedBlue, pixelReplacement, doArithmeticOperations, translateImg, addGaussianNoise (:17-79) with the reference's
//   signatures, and extractChannel, meanStdDev, subtract for the library calls main makes between them, as HOST LOOPS on
//   this thread.  They are the statement of the contract of the "ps0" block of include/mi_cv.h (parity with OpenCV
//   unpinned: cvRound rounds halves to even and gives INT_MIN for NaN, +-inf and values outside int; saturation follows);
//   ...Device        the same bytes from the library's `_host` entry points;
//   run / runDevice  main.cpp:110-171: the nine pictures, by the host loops and by ONE call (micv_ps0_run_host, three
//                    launches).
// cv::randn is the library's host generator (micv_cv_randn_f32_host) on theRNG(), as cv::theRNG() carries its state.
#pragma once

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "micv_shim.hpp"

namespace micv_ps0 {

using micv_shim::Mat;

inline int cvRound(double v) {
    const double r = std::nearbyint(v);
    return (r >= -2147483648.0 && r < 2147483648.0) ? static_cast<int>(r) : INT_MIN;
}
inline int cvRound(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? static_cast<int>(std::nearbyint(v)) : INT_MIN; }
inline unsigned char sat(int v) { return static_cast<unsigned char>(v < 0 ? 0 : (v > 255 ? 255 : v)); }

inline void requireU8(const Mat &m, int cn, const char *what) { micv_shim::require(m.depth() == micv_shim::U8 && m.channels() == cn && !m.empty(), what); }

struct Stats {  // micv_ps0_stats
    double mean = 0, stddev = 0;
    uint64_t sum = 0, sqsum = 0;
    int32_t min = 0, max = 0;
};

// ---- the host loops ---------------------------------------------------------------------------------------------------
inline void swapRedBlue(const Mat &inputImage, Mat &outputImage) {
    requireU8(inputImage, 3, "swapRedBlue: CV_8UC3 expected");
    Mat out(inputImage.rows, inputImage.cols, inputImage.type());
    for (int y = 0; y < out.rows; y++)
        for (int x = 0; x < out.cols; x++)
            for (int k = 0; k < 3; k++) out.ptr<unsigned char>(y)[3 * x + k] = inputImage.ptr<unsigned char>(y)[3 * x + 2 - k];
    outputImage = out;
}

inline void extractChannel(const Mat &src, Mat &dst, int coi) {
    micv_shim::require(src.depth() == micv_shim::U8 && coi >= 0 && coi < src.channels(), "extractChannel: 8-bit image and a channel of it expected");
    Mat out(src.rows, src.cols, micv::CV_8UC1);
    for (int y = 0; y < out.rows; y++)
        for (int x = 0; x < out.cols; x++) out.ptr<unsigned char>(y)[x] = src.ptr<unsigned char>(y)[x * src.channels() + coi];
    dst = out;
}

inline bool squareFits(const Mat &a, const Mat &b, int size) {
    const int ax = a.cols / 2 - size / 2, ay = a.rows / 2 - size / 2, bx = b.cols / 2 - size / 2, by = b.rows / 2 - size / 2;
    return size >= 0 && ax >= 0 && ay >= 0 && bx >= 0 && by >= 0 && ax + size <= a.cols && ay + size <= a.rows && bx + size <= b.cols &&
           by + size <= b.rows;
}

inline void pixelReplacement(const Mat &img1, const Mat &img2, Mat &outputImage, int size = 100) {
    micv_shim::require(img1.type() == img2.type() && img1.depth() == micv_shim::U8 && squareFits(img1, img2, size),
                       "pixelReplacement: two 8-bit images of one type that hold the square expected");
    Mat out = img2.clone();
    const int cn = img1.channels(), ax = img1.cols / 2 - size / 2, ay = img1.rows / 2 - size / 2, bx = img2.cols / 2 - size / 2,
              by = img2.rows / 2 - size / 2;
    for (int y = 0; y < size; y++)
        std::memcpy(out.ptr<unsigned char>(by + y) + (size_t)bx * cn, img1.ptr<unsigned char>(ay + y) + (size_t)ax * cn, (size_t)size * cn);
    outputImage = out;
}

inline Stats meanStdDev(const Mat &img) {
    requireU8(img, 1, "meanStdDev: CV_8UC1 expected");
    Stats s;
    s.min = 255, s.max = 0;
    for (int y = 0; y < img.rows; y++)
        for (int x = 0; x < img.cols; x++) {
            const unsigned v = img.ptr<unsigned char>(y)[x];
            s.sum += v, s.sqsum += (uint64_t)v * v;
            s.min = (int)v < s.min ? (int)v : s.min, s.max = (int)v > s.max ? (int)v : s.max;
        }
    const double inv = 1.0 / (double)((long long)img.rows * img.cols);
    s.mean = (double)s.sum * inv;
    const double var = (double)s.sqsum * inv - s.mean * s.mean;
    s.stddev = std::sqrt(var > 0.0 ? var : 0.0);
    return s;
}

inline void doArithmeticOperations(const Mat &inputImage, const double mean, const double stdDev, Mat &outputImage) {
    requireU8(inputImage, 1, "doArithmeticOperations: CV_8UC1 expected");
    Mat out(inputImage.rows, inputImage.cols, inputImage.type());
    const float a = static_cast<float>(1.0 / stdDev);
    for (int y = 0; y < out.rows; y++)
        for (int x = 0; x < out.cols; x++) {
            const int t1 = sat(cvRound((double)inputImage.ptr<unsigned char>(y)[x] - mean));  // outputImage -= mean
            const int t2 = sat(cvRound((float)t1 * a));                                       // outputImage /= stdDev
            const int t3 = sat(cvRound((float)t2 * 10.f));                                    // outputImage *= 10
            out.ptr<unsigned char>(y)[x] = sat(cvRound((double)t3 + mean));                   // outputImage += mean
        }
    outputImage = out;
}

// cv::warpAffine with [1 0 x; 0 1 y], INTER_LINEAR, BORDER_CONSTANT 0: an integer shift, zero where the source ends.
inline void translateImg(const Mat &image, const int xOffset, const int yOffset, Mat &output) {
    requireU8(image, 1, "translateImg: CV_8UC1 expected");
    Mat out = Mat::zeros(image.rows, image.cols, image.type());
    for (int y = 0; y < out.rows; y++)
        for (int x = 0; x < out.cols; x++) {
            const long long sx = (long long)x - xOffset, sy = (long long)y - yOffset;
            if (sx >= 0 && sx < image.cols && sy >= 0 && sy < image.rows) out.ptr<unsigned char>(y)[x] = image.ptr<unsigned char>((int)sy)[sx];
        }
    output = out;
}

inline void subtract(const Mat &a, const Mat &b, Mat &dst) {  // a -= b
    micv_shim::require(a.type() == micv::CV_8UC1 && b.type() == a.type() && a.rows == b.rows && a.cols == b.cols, "subtract: two CV_8UC1 images of one size");
    Mat out(a.rows, a.cols, a.type());
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) out.ptr<unsigned char>(y)[x] = sat((int)a.ptr<unsigned char>(y)[x] - (int)b.ptr<unsigned char>(y)[x]);
    dst = out;
}

// addGaussianNoise's arithmetic on a drawn plane (rows x cols floats, dense): both operands as CV_8SC1
inline void addNoisePlane(const Mat &image, const float *noise, Mat &output) {
    requireU8(image, 1, "addGaussianNoise: CV_8UC1 expected");
    Mat out(image.rows, image.cols, image.type());
    for (int y = 0; y < out.rows; y++)
        for (int x = 0; x < out.cols; x++) {
            int n = cvRound(noise[(size_t)y * image.cols + x]);
            n = n < -128 ? -128 : (n > 127 ? 127 : n);
            const int p = image.ptr<unsigned char>(y)[x];
            int s = (p > 127 ? 127 : p) + n;  // image.convertTo(output, CV_8SC1)
            s = s < -128 ? -128 : (s > 127 ? 127 : s);
            out.ptr<unsigned char>(y)[x] = static_cast<unsigned char>(s < 0 ? 0 : s);
        }
    output = out;
}

inline uint64_t &theRNG() {
    static uint64_t state = 0xffffffffull;
    return state;
}
inline std::vector<float> randn(int rows, int cols, double mean, double sigma) {
    std::vector<float> z((size_t)rows * cols);
    micv_shim::check(micv_cv_randn_f32_host(&theRNG(), (float)mean, (float)sigma, rows, cols, z.data(), (size_t)cols * 4));
    return z;
}

inline void addGaussianNoise(const Mat &image, const double mean, const double sigma, Mat &output) {
    if (image.channels() != 1) return;  // :68-71
    addNoisePlane(image, randn(image.rows, image.cols, mean, sigma).data(), output);
}

// ---- the same from the library ----------------------------------------------------------------------------------------
inline void mixDevice(const Mat &src, const int *map, int dcn, Mat &dst) {
    Mat out(src.rows, src.cols, micv::make_type(micv::CV_8U, dcn));
    micv_shim::check(micv_mix_channels_u8_host(micv_shim::context(), src.data, src.rows, src.cols, src.channels(), src.step, map, out.data, dcn, out.step));
    dst = out;
}
inline void swapRedBlueDevice(const Mat &inputImage, Mat &outputImage) {
    requireU8(inputImage, 3, "swapRedBlue: CV_8UC3 expected");
    const int map[3] = {2, 1, 0};
    mixDevice(inputImage, map, 3, outputImage);
}
inline void extractChannelDevice(const Mat &src, Mat &dst, int coi) {
    micv_shim::require(src.depth() == micv_shim::U8, "extractChannel: 8-bit image expected");
    mixDevice(src, &coi, 1, dst);
}
inline void pixelReplacementDevice(const Mat &img1, const Mat &img2, Mat &outputImage, int size = 100) {
    micv_shim::require(img1.type() == img2.type() && img1.depth() == micv_shim::U8, "pixelReplacement: two 8-bit images of one type expected");
    Mat out(img2.rows, img2.cols, img2.type());
    micv_shim::check(micv_pixel_replacement_u8_host(micv_shim::context(), img1.data, img1.rows, img1.cols, img1.step, img2.data, img2.rows, img2.cols,
                                                    img2.step, img1.channels(), size, out.data, out.step));
    outputImage = out;
}
inline Stats meanStdDevDevice(const Mat &img) {
    requireU8(img, 1, "meanStdDev: CV_8UC1 expected");
    micv_ps0_stats r;
    micv_shim::check(micv_mean_stddev_u8_host(micv_shim::context(), img.data, img.rows, img.cols, img.step, &r));
    Stats s;
    s.mean = r.mean, s.stddev = r.stddev, s.sum = r.sum, s.sqsum = r.sqsum, s.min = r.min, s.max = r.max;
    return s;
}
inline void doArithmeticOperationsDevice(const Mat &inputImage, const double mean, const double stdDev, Mat &outputImage) {
    requireU8(inputImage, 1, "doArithmeticOperations: CV_8UC1 expected");
    Mat out(inputImage.rows, inputImage.cols, inputImage.type());
    micv_shim::check(micv_ps0_arithmetic_u8_host(micv_shim::context(), inputImage.data, inputImage.rows, inputImage.cols, inputImage.step, mean, stdDev,
                                                 out.data, out.step));
    outputImage = out;
}
inline void translateImgDevice(const Mat &image, const int xOffset, const int yOffset, Mat &output) {
    requireU8(image, 1, "translateImg: CV_8UC1 expected");
    Mat out(image.rows, image.cols, image.type());
    const float m[6] = {1, 0, (float)xOffset, 0, 1, (float)yOffset};
    micv_shim::check(micv_warp_affine_host(micv_shim::context(), image.data, MICV_DEPTH_8U, image.rows, image.cols, image.step, m, 0, out.data, out.rows,
                                           out.cols, out.step));
    output = out;
}
inline void subtractDevice(const Mat &a, const Mat &b, Mat &dst) {
    micv_shim::require(a.type() == micv::CV_8UC1 && b.type() == a.type() && a.rows == b.rows && a.cols == b.cols, "subtract: two CV_8UC1 images of one size");
    Mat out(a.rows, a.cols, a.type());
    micv_shim::check(micv_subtract_sat_u8_host(micv_shim::context(), a.data, a.step, b.data, b.step, a.rows, a.cols, out.data, out.step));
    dst = out;
}
inline void addGaussianNoiseDevice(const Mat &image, const double mean, const double sigma, Mat &output) {
    if (image.channels() != 1) return;
    const std::vector<float> z = randn(image.rows, image.cols, mean, sigma);
    Mat out(image.rows, image.cols, image.type());
    micv_shim::check(micv_add_noise_s8_u8_host(micv_shim::context(), image.data, image.step, z.data(), (size_t)image.cols * 4, image.rows, image.cols,
                                               out.data, out.step));
    output = out;
}

// ---- main.cpp:110-171 -------------------------------------------------------------------------------------------------
struct Pictures {  // ps0-2-a-1, 2-b-1, 2-c-1, 3-a-1, 4-b-1, 4-c-1, 4-d-1, 5-a-1, 5-b-1
    Mat swapped, green, red, replaced, arithmeticOps, translatedGreen, translationDiff, noisyGreen, noisyBlue;
    Stats stats;
};
constexpr int kNoiseSigma = 5;  // :163

inline Pictures run(const Mat &image1, const Mat &image2, int size = 100) {
    Pictures p;
    Mat redBG, blue;
    swapRedBlue(image1, p.swapped);
    extractChannel(image1, p.green, 1);
    extractChannel(image1, p.red, 2);
    extractChannel(image2, redBG, 2);
    pixelReplacement(p.red, redBG, p.replaced, size);
    p.stats = meanStdDev(p.green);
    doArithmeticOperations(p.green, p.stats.mean, p.stats.stddev, p.arithmeticOps);
    translateImg(p.green, -2, 0, p.translatedGreen);
    subtract(p.green, p.translatedGreen, p.translationDiff);
    addGaussianNoise(p.green, 0, kNoiseSigma, p.noisyGreen);
    extractChannel(image1, blue, 0);
    addGaussianNoise(blue, 0, kNoiseSigma, p.noisyBlue);
    return p;
}

inline Pictures runDevice(const Mat &image1, const Mat &image2, int size = 100) {
    requireU8(image1, 3, "run: CV_8UC3 expected");
    requireU8(image2, 3, "run: CV_8UC3 expected");
    Pictures p;
    const int r = image1.rows, c = image1.cols;
    p.swapped = Mat(r, c, micv::CV_8UC3);
    p.replaced = Mat(image2.rows, image2.cols, micv::CV_8UC1);
    Mat planes(7 * r, c, micv::CV_8UC1);
    micv_ps0_stats st;
    micv_shim::check(micv_ps0_run_host(micv_shim::context(), image1.data, r, c, image1.step, image2.data, image2.rows, image2.cols, image2.step, size,
                                       &theRNG(), 0.f, (float)kNoiseSigma, p.swapped.data, p.swapped.step, planes.data, planes.step,
                                       planes.step * (size_t)r, p.replaced.data, p.replaced.step, &st));
    Mat *out[7] = {&p.green, &p.red, &p.arithmeticOps, &p.translatedGreen, &p.translationDiff, &p.noisyGreen, &p.noisyBlue};
    for (int k = 0; k < 7; k++) *out[k] = Mat(r, c, micv::CV_8UC1, planes.ptr<unsigned char>(k * r), planes.step).clone();
    p.stats.mean = st.mean, p.stats.stddev = st.stddev, p.stats.sum = st.sum, p.stats.sqsum = st.sqsum, p.stats.min = st.min, p.stats.max = st.max;
    return p;
}

}  // namespace micv_ps0
