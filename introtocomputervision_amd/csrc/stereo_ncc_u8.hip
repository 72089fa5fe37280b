// stereo_ncc_u8.hip -- disparityNCorr on byte images, radius 1..10 without ROLLING: the float search of stereo_float.hpp
// with a byte source (micv_disparity_ncorr_u8_{dev,batch_dev}; the dispatch is stereo.hip's stereo_u8_common).
//
// Two launches per piece of a batch, and nothing in device memory but the bytes and one f32 window-energy plane per pair:
//   stereo_energy_kernel      the window energy of `right`, summed in the contract's order from the bytes
//   stereo_ncc_u8_kernel      stereo_tile<R, ST_NCC, RPW, DCH> on StereoArgs8: Lv[], the prefetch registers and the LDS strip
//                             are filled from byte loads at y * pitch + x (clamp-to-edge, each image its own pitch), converted
//                             to f32 as they are staged; the search loop is the f32 kernel's, instruction for instruction
// The pair is blockIdx.z.  Rows per wave, the chunk of disparities, the prefetch and the register budget are the f32
// kernel's (stereo.hip: launch_stereo).  What differs: on bytes every operand is in the range of ncc_arith.hpp's short
// sqrt / division, so the instantiation has neither NccRange tracking nor the long-form search body.
#include "stereo_float.hpp"

namespace micv {

template <int R, int RPW, int ST_DCH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) void stereo_ncc_u8_kernel(StereoArgs8 a) {
    extern __shared__ float st_lds[];
    a.select(blockIdx.z);
    stereo_tile<R, ST_NCC, RPW, ST_DCH>(a, st_lds, blockIdx.x, blockIdx.y);
}

template <int R, int RPW>
static void launch(hipStream_t s, const StereoArgs8 &a, int batch) {
    constexpr int DCH = stereo_ncc_dch(R, RPW), OUTW = 64 - 2 * R;
    const unsigned gy = cdiv(a.rows, 4 * RPW);
    stereo_energy_kernel<R, RPW><<<dim3(cdiv(a.e_width, OUTW), gy, batch), 256, 0, s>>>(a, a.energy);
    stereo_ncc_u8_kernel<R, RPW, DCH><<<dim3(cdiv(a.cols, OUTW), gy, batch), 256,
                                        4 * (2 * RPW + 2 * R) * (64 + DCH) * sizeof(float), s>>>(a);
}

int stereo_ncc_u8_launch(hipStream_t s, const StereoArgs8 &a, int batch, int rad, bool rows10) {
    MICV_REQUIRE(rad >= 1 && rad <= 10 && batch >= 1 && batch <= 65535, "stereo_ncc_u8_launch: radius %d, %d pairs", rad, batch);
#define MICV_ST8_CASE(RR)                                           \
    case RR:                                                        \
        if (rows10) launch<RR, 10>(s, a, batch); else launch<RR, 8>(s, a, batch); \
        break;
    switch (rad) {
        MICV_ST8_CASE(1) MICV_ST8_CASE(2) MICV_ST8_CASE(3) MICV_ST8_CASE(4) MICV_ST8_CASE(5)
        MICV_ST8_CASE(6) MICV_ST8_CASE(7) MICV_ST8_CASE(8) MICV_ST8_CASE(9) MICV_ST8_CASE(10)
    }
#undef MICV_ST8_CASE
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace micv
