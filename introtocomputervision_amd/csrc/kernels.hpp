// kernels.hpp -- host-side launchers shared between translation units of libmicv.
#pragma once
#include "common.hpp"

namespace micv {

// Separable correlation passes over `nfields` planar fields (field f at base + f*field_elems).
// Row pass: dst(y,x) = chain_k fmaf(src(y, reflect101(x+k-n/2)), taps[k], acc), acc0 = +0.
int launch_filter_rows(hipStream_t s, const float *src, int sstride, size_t sfield, float *dst,
                       int dstride, size_t dfield, int rows, int cols, int nfields, const Taps &t);
// Column pass, same chain top->bottom.
int launch_filter_cols(hipStream_t s, const float *src, int sstride, size_t sfield, float *dst,
                       int dstride, size_t dfield, int rows, int cols, int nfields, const Taps &t);

// Sobel pair through the two generic passes. tmp: 2*rows*cols floats.
int sobel_dev(hipStream_t s, const float *src, int rows, int cols, int sstride, int ksize,
              float scale, float *gx, float *gy, int gstride, float *tmp, bool force_generic = false);

// dst(y,x) = src(2y+1, 2x+1), dst dims (rows/2, cols/2).
int launch_pyr_down(hipStream_t s, const float *src, int rows, int cols, int sstride, float *dst,
                    int dstride);
// 2x replicate + [1,4,6,4,1]/16 separable blur, result times `scale` (1 or 2, exact).
// tmp: rows * 2*cols floats.
int launch_pyr_up(hipStream_t s, const float *src, int rows, int cols, int sstride, float *dst,
                  int dstride, float scale, float *tmp);
// Builds pyramid levels of `batch` images in one launch (level l = direct decimation of the
// input). dst[l] == nullptr skips a level; image b of level l lands at dst[l] + b*rows_l*cols_l.
int launch_pyr_build(hipStream_t s, const float *src, size_t img_elems, int sstride, int rows,
                     int cols, int levels, float *const *dst, int batch);
// Two image sets (prev / next) in one launch; dst_a[l] == nullptr skips level l in both.
int launch_pyr_build2(hipStream_t s, const float *src_a, const float *src_b, size_t img_elems,
                      int sstride, int rows, int cols, int levels, float *const *dst_a,
                      float *const *dst_b, int batch, const int *row_lo = nullptr,
                      const int *row_hi = nullptr);
// A frame sequence (frame f at src + f*frame_pitch bytes, 1 / 3 / 4 channels of MICV_DEPTH_8U, 3 / 4 of MICV_DEPTH_32F):
// the dense grey plane of every frame (gray + f*gray_elems, pitch cols) and levels 1 .. levels-1 of its pyramid
// (dst[l] + f*rows_l*cols_l; dst[0] is not read) in one launch.
int launch_seq_gray_pyr(hipStream_t s, const void *src, size_t frame_pitch, size_t sstride, int channels, int depth,
                        int frames, int rows, int cols, float *gray, size_t gray_elems, int levels, float *const *dst);
int launch_resize_linear(hipStream_t s, const float *src, int srows, int scols, int sstride,
                         float *dst, int drows, int dcols, int dstride);
// du = resize(2 * pyrUp(du_coarse), drows x dcols) for `batch` pairs and both fields, one launch.
int launch_flow_expand_resize(hipStream_t s, const float *src_u, const float *src_v, int fr, int fc,
                              size_t src_pair, float *dst_u, float *dst_v, int drows, int dcols,
                              size_t dst_pair, int batch);
int launch_warp(hipStream_t s, const float *src, int sstride, const float *du, const float *dv,
                int fstride, int rows, int cols, float *dst, int dstride, int batch = 1, size_t src_img = 0,
                size_t flow_img = 0, size_t dst_img = 0);
int launch_pyr_up_batch(hipStream_t s, const float *src_u, const float *src_v, int rows, int cols, size_t src_img,
                        float *dst_u, float *dst_v, size_t dst_img, float scale, int batch);

// canny.hip: the u8 Gaussian blur of sol::generateEdge / sol::gaussianBlur, and the Canny stages behind it on a blurred
// 8-bit plane (weak / strong: rows * cdiv(cols, 64) words of scratch each; synchronises `s` like micv_generate_edge_dev).
int launch_gauss_u8(hipStream_t s, const uint8_t *src, size_t stride, int rows, int cols, const Taps &t, uint8_t *dst,
                    size_t dstride);
int canny_from_u8(micv_ctx *ctx, hipStream_t s, const uint8_t *cin, size_t cstride, int rows, int cols, double low_thresh,
                  double high_thresh, unsigned long long *weak, unsigned long long *strong, uint8_t *edges, size_t estride);
// ps1.hip: the float front end of micv_generate_edge_f32_dev -- the float blur and saturate_cast<uchar>(cvRound(v)) into a
// byte plane (stride in bytes, a multiple of 4)
int launch_gauss_f32_to_u8(hipStream_t s, const float *src, size_t stride, int rows, int cols, const Taps &t, uint8_t *dst, size_t dstride);
// hough.hip: maxDist of Hough.cu:258-259
size_t hough_diag(int rows, int cols);

// sift.hip, for the byte entries of sift_u8.hip: the descriptor kernel on `batch` byte images of one size (image i at
// img + i * img_dist, pitch in bytes), lists of cap rows ([batch][cap][4]) with device counts ([batch], or null: cap
// rows each), descriptor blocks desc_dist bytes apart with rows dstride bytes apart.  cap >= 1; nothing is validated here.
int sift_u8_launch(hipStream_t s, const uint8_t *img, size_t img_dist, int batch, int rows, int cols, size_t pitch, const float *kps,
                   int64_t cap, const int64_t *count, float *desc, size_t desc_dist, size_t dstride);

// harris.hip, for the byte entries of harris_u8.hip.  The fused image -> R launch on `images` byte images of one size
// (image i at img + i * img_dist, pitch in bytes; R, and the gradient planes when gx is not null, at i * resp_dist /
// i * grad_dist bytes); tall: 64x32 tiles instead of 64x16.
struct HarrisU8Launch {
    const uint8_t *img;
    size_t img_dist, pitch;
    int rows, cols, images;
    Taps g;
    float alpha;
    float *resp;
    size_t resp_dist, rstride;
    float *gx, *gy;
    size_t grad_dist, gstride;
    bool tall;
};
int harris_image_u8_launch(hipStream_t s, const HarrisU8Launch &a, int r, bool cpu);
// Threshold + NMS of `images` responses in one launch: sparse maps (optional) and rows * cdiv(cols, 64) mask words per
// image, image i's at rowmask + i * mask_words.  Distances in bytes.
int harris_nms_batch_launch(micv_ctx *ctx, hipStream_t s, const float *resp, size_t resp_dist, int rows, int cols, size_t rstride,
                            double threshold, int min_distance, float *corners, size_t corners_dist, size_t cstride,
                            unsigned long long *rowmask, size_t mask_words, int images);
// One image's ordered list from its mask words, as micv_harris_refine_dev makes it; scratch: harris_list_scratch_bytes().
int harris_list_run(micv_ctx *ctx, hipStream_t s, const unsigned long long *rowmask, int rows, int cols, int32_t *locs_yx, int64_t cap,
                    int64_t *count, void *scratch);
size_t harris_list_scratch_bytes(int rows, int cols);

// sift::getKeypoints' row for corner (y, x) with gradient (gxv, gyv) there: cv::KeyPoint(x = corner.second,
// y = corner.first, size, angle), Descriptors.cpp:33-45.
__device__ __forceinline__ void sift_keypoint_store(float gxv, float gyv, int y, int x, float size, float *__restrict__ kp) {
    const float PI = 3.1415921636f;  // sic, Descriptors.cpp:5
    const float a = atan2f(gyv, gxv) * 180.f / PI;
    kp[0] = (float)x;
    kp[1] = (float)y;
    kp[2] = size;
    kp[3] = a;
}

}  // namespace micv
