// sift_u8.hip -- the descriptor step of Solution::siftHelper on byte images: micv_sift_descriptors_u8_{dev,host,batch_dev}
// (mi_cv.h).  The kernel is sift.hip's descriptor body on a byte source: the 3 x 3 Sobel pair of every sample is recomputed
// from the image, so device memory holds the bytes, the keypoint lists and the descriptors only, and
// the list lengths are read on the device.
#include "host_io.hpp"
#include "kernels.hpp"

namespace micv {

static int sift_u8_common(const char *fn, micv_ctx *ctx, const uint8_t *img, size_t img_dist, int batch, int rows, int cols, size_t stride,
                          const float *kp_xysa, int64_t cap, const int64_t *count, float *desc, size_t d_dist, size_t dstride,
                          micv_stream stream) {
    MICV_REQUIRE(ctx && img, "%s: null argument", fn);
    MICV_REQUIRE(batch >= 1 && batch <= 65535, "%s: batch %d", fn, batch);
    MICV_REQUIRE(cap >= 0 && (cap == 0 || (kp_xysa && desc)), "%s: bad keypoint list", fn);
    MICV_REQUIRE(rows > 0 && cols > 0 && stride >= (size_t)cols, "%s: bad size / stride", fn);
    MICV_REQUIRE(dstride % 4 == 0 && dstride >= 128 * 4 && dstride / 4 < ((size_t)1 << 30), "%s: descriptor rows are 128 floats", fn);
    MICV_REQUIRE(cap < ((int64_t)1 << 31) * 4, "%s: too many keypoints", fn);
    MICV_REQUIRE(rows <= 65535 && cols <= 65535, "%s: images up to 65 535 pixels on a side", fn);
    // one image's descriptor block: cap rows, the last one 128 floats long -- (cap - 1) * dstride + 512 <= d_dist, as a
    // quotient: the product of a cap near 2^33 and a stride near 2^32 would wrap
    MICV_REQUIRE(batch == 1 || cap == 0 || (d_dist % 4 == 0 && d_dist >= 512 && (size_t)(cap - 1) <= (d_dist - 512) / dstride),
                 "%s: the descriptor blocks of a batch overlap (image stride %zu)", fn, d_dist);
    MICV_HIP(hipSetDevice(ctx->device));
    if (cap == 0) return MICV_OK;
    return sift_u8_launch(static_cast<hipStream_t>(stream), img, img_dist, batch, rows, cols, stride, kp_xysa, cap, count, desc,
                          batch > 1 ? d_dist : 0, dstride);
}

}  // namespace micv

using namespace micv;

extern "C" {

int micv_sift_descriptors_u8_dev(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, const float *kp_xysa, int64_t cap,
                                 const int64_t *count, float *desc, size_t dstride, micv_stream stream) {
    return sift_u8_common("micv_sift_descriptors_u8", ctx, img, 0, 1, rows, cols, stride, kp_xysa, cap, count, desc, 0, dstride, stream);
}

int micv_sift_descriptors_u8_batch_dev(micv_ctx *ctx, const uint8_t *img, size_t image_stride, int batch, int rows, int cols, size_t stride,
                                       const float *kp_xysa, int64_t cap, const int64_t *count, float *desc, size_t dimage_stride,
                                       size_t dstride, micv_stream stream) {
    return sift_u8_common("micv_sift_descriptors_u8_batch", ctx, img, image_stride, batch, rows, cols, stride, kp_xysa, cap, count, desc,
                          dimage_stride, dstride, stream);
}

int micv_sift_descriptors_u8_host(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, const float *kp_xysa, int64_t n,
                                  float *desc, size_t dstride) {
    HostCall h(ctx, "micv_sift_descriptors_u8_host");
    if (!h.ok()) return h.finish();
    MICV_REQUIRE(img && rows > 0 && cols > 0 && n >= 0 && (n == 0 || (kp_xysa && desc)), "micv_sift_descriptors_u8_host: bad argument");
    MICV_REQUIRE(stride >= (size_t)cols && dstride % 4 == 0 && dstride >= 512, "micv_sift_descriptors_u8_host: bad stride");
    MICV_REQUIRE(n <= INT32_MAX, "micv_sift_descriptors_u8_host: too many keypoints");  // (the row count of the 2-D download)
    if (n == 0) return MICV_OK;
    // 1 B per pixel up (micv_sift_descriptors_host: 8)
    uint8_t *di = h.up<uint8_t>(img, stride, (size_t)cols, rows);
    float *dk = h.up<float>(kp_xysa, (size_t)n * 16), *dd = h.alloc<float>((size_t)n * 512);
    if (!h.ok()) return h.finish();
    MICV_TRY(micv_sift_descriptors_u8_dev(ctx, di, rows, cols, (size_t)cols, dk, n, nullptr, dd, 512, h.s));
    h.down(desc, dstride, dd, 512, (int)n);
    return h.finish();
}

}  // extern "C"
