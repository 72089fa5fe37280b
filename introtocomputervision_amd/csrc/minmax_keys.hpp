// minmax_keys.hpp -- the order-preserving 32-bit keys the min-max reductions keep their extremes in (display.hip,
// ps5.hip): NaNs drop out, a zero word means "nothing seen", and an atomic max on the key (and on the complement of the
// minimum's key) is exact whatever the order of arrival.
#pragma once
#include "common.hpp"

namespace micv {

// float <-> unsigned, order-preserving (-inf < ... < -0 < +0 < ... < +inf); no non-NaN float maps to 0 or to ~0.
__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

}  // namespace micv
