// draw.hpp -- device-side pieces shared by the overlay kernels (ps1.hip: sol::drawLinesParametric, sol::drawCircles;
// ps5.hip: drawVelocityVectors; ps4.hip: the keypoint glyphs and match lines).  The contract is micv_viz::line
// (shim/micv_viz.hpp), cv::LineIterator's walk.
#pragma once
#include "common.hpp"

namespace micv {

// saturate_cast<uchar>(cvRound(v)): cvRound is x86's cvtss2si -- half to even, and INT_MIN for NaN, +-inf and every
// value outside int, which then saturates to 0.
__device__ __forceinline__ uint8_t f32_to_u8(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return 0;
    const int r = (int)rintf(v);
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// One bounds-checked 3-channel pixel (micv_viz::put_pixel).
__device__ __forceinline__ void put_rgb(uint8_t *img, size_t stride, int rows, int cols, long long x, long long y, uint8_t c0,
                                        uint8_t c1, uint8_t c2) {
    if (x < 0 || x >= cols || y < 0 || y >= rows) return;
    uint8_t *d = img + (size_t)y * stride + 3 * (size_t)x;
    d[0] = c0;
    d[1] = c1;
    d[2] = c2;
}

// The minor coordinate's advance after i major steps of micv_viz::line's walk (err = major - 2 minor; a step moves the
// minor axis when err < 0, then err += 2 major - 2 minor, else err -= 2 minor):
// m(i) = (2 minor i + major - 1) div (2 major).  64-bit throughout: 2 minor i passes 2^31 on a long stroke.
__device__ __forceinline__ long long line_minor_after(long long minor, long long major, long long i) {
    return major == 0 ? 0 : (2 * minor * i + major - 1) / (2 * major);
}

}  // namespace micv
