// pixmap.hpp -- the one "source pixel to three bytes" kernel: cv::cvtColor(GRAY2RGB) to 8 bit (ps1.hip), prevImg.clone()
// with GRAY2RGB for a grey frame (ps5.hip) and the panel copy of cv::drawKeypoints (ps4.hip).  A thread is a pixel, a
// workgroup 64 x 4 of them; the per-pixel read is draw::read_bgr (draw.hpp).
#pragma once
#include "common.hpp"
#include "draw.hpp"

namespace micv {

template <typename T, int CN>
__global__ __launch_bounds__(256) void to_bgr8_kernel(const T *__restrict__ src, size_t sstride, int rows, int cols,
                                                       uint8_t *__restrict__ dst, size_t dstride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const T *row = reinterpret_cast<const T *>(reinterpret_cast<const char *>(src) + (size_t)y * sstride);
    draw::put(draw::Target{dst, dstride, rows, cols, 3}, x, y, draw::read_bgr<T, CN>(row, x));
}

// depth 8U with 1 or 3 channels, or 32F grey; the strides in bytes
inline int launch_to_bgr8(hipStream_t s, const void *src, int depth, int channels, size_t sstride, int rows, int cols, uint8_t *dst,
                          size_t dstride) {
    const dim3 grid(cdiv(cols, 64), cdiv(rows, 4));
    if (depth == MICV_DEPTH_32F)
        to_bgr8_kernel<float, 1><<<grid, 256, 0, s>>>(static_cast<const float *>(src), sstride, rows, cols, dst, dstride);
    else if (channels == 3)
        to_bgr8_kernel<uint8_t, 3><<<grid, 256, 0, s>>>(static_cast<const uint8_t *>(src), sstride, rows, cols, dst, dstride);
    else
        to_bgr8_kernel<uint8_t, 1><<<grid, 256, 0, s>>>(static_cast<const uint8_t *>(src), sstride, rows, cols, dst, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace micv
