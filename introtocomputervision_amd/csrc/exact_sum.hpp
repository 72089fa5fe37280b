// exact_sum.hpp -- order-independent exact sums of f32 terms (moments.hip).
//
// A finite f32 term is mant * 2^(s - 149) with mant < 2^24 and s = biased exponent - 1 (0 for subnormals), s in
// [0, 253].  It lands in bin s >> 4 (16 bins of 16 exponent steps) as the signed integer mant << (s & 15), below
// 2^39 in magnitude; bin k weighs 2^(16k - 149).  Bins are summed as int64 in any order -- integer addition is exact
// and associative -- so the total is the exact sum whatever the grid shape or the schedule.  With at most 2^24
// terms per bin no int64 overflows (2^24 * 2^39 = 2^63).  The final big integer is rounded once to double
// (round-to-nearest-even), which is what `float x = cv::sum(...)[0]` would give if its double accumulator were
// exact; the caller then rounds that double to f32.
//
// Non-finite terms do not enter the bins: they set a flag (kNaN, kPosInf, kNegInf), and the flags decide the result.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else  // plain C++ (tests/cpp/exact_sum_check.cpp runs the rounding on the host against math.fsum)
#include <cmath>
#define __host__
#define __device__
#endif

#include <cstdint>

namespace micv {

constexpr int kSumBins = 16;
constexpr unsigned kSumNaN = 1u, kSumPosInf = 2u, kSumNegInf = 4u;
constexpr uint64_t kMaxExactTerms = 1ull << 24;  // per sum; the callers' image-size limit

// Splits one f32 term; a zero or non-finite term gives value 0 (non-finite ones set `flags`).
__host__ __device__ inline void split_term(float t, int &bin, long long &val, unsigned &flags) {
    const uint32_t u = __builtin_bit_cast(uint32_t, t);
    const uint32_t e = (u >> 23) & 255u, m = u & 0x7FFFFFu;
    if (e == 255u) {
        flags |= m ? kSumNaN : ((u >> 31) ? kSumNegInf : kSumPosInf);
        bin = 0;
        val = 0;
        return;
    }
    const uint32_t mant = e ? (m | 0x800000u) : m;
    const int s = e ? (int)e - 1 : 0;
    bin = s >> 4;
    const long long v = (long long)mant << (s & 15);
    val = (u >> 31) ? -v : v;
}

// Rounds the exact value sum_k bins[k] * 2^(16k - 149) once to double (RNE); `bins` is clobbered.
__host__ __device__ inline double round_bins_to_double(long long *bins) {
    // carries: limbs 0..14 into [0, 2^16), limb 15 keeps the sign
    for (int k = 0; k < kSumBins - 1; k++) {
        const long long c = bins[k] >> 16;  // arithmetic shift: floor division
        bins[k] -= c * 65536;
        bins[k + 1] += c;
    }
    bool neg = bins[kSumBins - 1] < 0;
    if (neg) {  // two's complement of the whole number, limb by limb
        long long carry = 1;
        for (int k = 0; k < kSumBins - 1; k++) {
            long long v = (0xFFFF - bins[k]) + carry;
            carry = v >> 16;
            bins[k] = v & 0xFFFF;
        }
        bins[kSumBins - 1] = ~bins[kSumBins - 1] + carry;
    }
    // 16-bit limbs of the magnitude: 15 from the low bins, 4 from the top bin (< 2^63)
    uint32_t limb[kSumBins + 3];
    for (int k = 0; k < kSumBins - 1; k++) limb[k] = (uint32_t)bins[k];
    const uint64_t top = (uint64_t)bins[kSumBins - 1];
    for (int j = 0; j < 4; j++) limb[kSumBins - 1 + j] = (uint32_t)((top >> (16 * j)) & 0xFFFFu);
    int h = kSumBins + 2;
    while (h >= 0 && limb[h] == 0) h--;
    if (h < 0) return 0.0;
    int hb = 15;
    while (!((limb[h] >> hb) & 1u)) hb--;
    const int nbits = 16 * h + hb + 1;  // bit length of the magnitude
    const int lo = nbits > 64 ? nbits - 64 : 0;
    // the 64 (or fewer) leading bits, and a sticky bit for everything below them
    uint64_t w = 0;
    bool sticky = false;
    for (int k = 0; k <= h; k++) {
        const int b0 = 16 * k;  // bit position of limb k
        const uint64_t l = limb[k];
        if (b0 + 16 <= lo) {
            sticky |= l != 0;
        } else if (b0 < lo) {
            const int sh = lo - b0;
            sticky |= (l & ((1ull << sh) - 1)) != 0;
            w |= l >> sh;
        } else {
            w |= l << (b0 - lo);
        }
    }
    // 64 bits > 53 + 2: OR-ing the sticky into the lowest bit makes the one conversion round as the exact value would
    if (sticky) w |= 1ull;
    const double d = (double)w;  // RNE
    const double r = ldexp(d, lo - 149);  // exact: the result is a normal double
    return neg ? -r : r;
}

// The f32 result of a sum: flags first, then the bins rounded to double, then to f32.
__host__ __device__ inline float finish_sum(long long *bins, unsigned flags) {
    if ((flags & kSumNaN) || ((flags & kSumPosInf) && (flags & kSumNegInf)))
        return __builtin_bit_cast(float, 0x7FC00000u);
    if (flags & kSumPosInf) return __builtin_bit_cast(float, 0x7F800000u);
    if (flags & kSumNegInf) return __builtin_bit_cast(float, 0xFF800000u);
    return (float)round_bins_to_double(bins);
}

}  // namespace micv
