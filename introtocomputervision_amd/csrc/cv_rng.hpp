// cv_rng.hpp -- cv::RNG (multiply-with-carry words, the ziggurat gaussian of rand.cpp) and the library's double exp,
// shared by the host-side generators of pf.hip (ps6: displacement, resampling and particle tables) and display.hip
// (micv_cv_randn_f32_host: the noise images of ps2's addNoise).  One definition, so that the two draw the same
// sequence; tests/_pf_ref.py restates it.  -ffp-contract=off like everything else.
#pragma once

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace micv {

// 2^e for -1022 <= e <= 1023, exactly.
__host__ __device__ inline double pow2i(int e) { return __builtin_bit_cast(double, (uint64_t)(e + 1023) << 52); }

// The library's double exp (mi_cv.h): fdlibm's reduction and rational form, no contraction, so the host
// generator, the device similarities and tests/_pf_ref.py agree bit for bit.
__host__ __device__ inline double pf_exp(double x) {
    if (x != x) return x;
    if (x > 7.09782712893383973096e+02) return HUGE_VAL;
    if (x < -7.45133219101941108420e+02) return 0.0;
    const int k = (int)(x * 1.44269504088896338700e+00 + (x < 0 ? -0.5 : 0.5));
    const double hi = x - (double)k * 6.93147180369123816490e-01;
    const double lo = (double)k * 1.90821492927058770002e-10;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (1.66666666666666019037e-01 +
                              t * (-2.77777777770155933842e-03 +
                                   t * (6.61375632143793436117e-05 +
                                        t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))));
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    if (k > 1000) return (y * pow2i(1000)) * pow2i(k - 1000);
    if (k < -1000) return (y * pow2i(k + 1000)) * pow2i(-1000);
    return y * pow2i(k);
}

// cv::RNG (OpenCV 3.4 core/operations.hpp, rand.cpp) as mi_cv.h restates it.
struct CvRng {
    uint64_t state;
    explicit CvRng(uint64_t seed) : state(seed ? seed : 0xffffffffull) {}
    uint32_t next() {
        state = (uint64_t)(uint32_t)state * 4164903690u + (state >> 32);
        return (uint32_t)state;
    }
    float uniform(float a, float b) {
        const float u = (float)next() * 2.3283064365386962890625e-10f;
        return u * (b - a) + a;
    }
    double gaussian(double sigma);
};

struct Ziggurat {
    uint32_t kn[128];
    float wn[128], fn[128];
    Ziggurat() {
        const double m1 = 2147483648.0;
        double dn = 3.442619855899, tn = dn;
        const double vn = 9.91256303526217e-3;
        const double q = vn / pf_exp(-.5 * dn * dn);
        kn[0] = (uint32_t)((dn / q) * m1);
        kn[1] = 0;
        wn[0] = (float)(q / m1);
        wn[127] = (float)(dn / m1);
        fn[0] = 1.f;
        fn[127] = (float)pf_exp(-.5 * dn * dn);
        for (int i = 126; i >= 1; i--) {
            dn = std::sqrt(-2. * std::log(vn / dn + pf_exp(-.5 * dn * dn)));
            kn[i + 1] = (uint32_t)((dn / tn) * m1);
            tn = dn;
            fn[i] = (float)pf_exp(-.5 * dn * dn);
            wn[i] = (float)(dn / m1);
        }
    }
};

inline float logf_d(float v) { return (float)std::log((double)v); }

inline double CvRng::gaussian(double sigma) {
    static const Ziggurat z;
    const float r = 3.442620f, rng_flt = 2.3283064365386962890625e-10f;
    uint64_t temp = state;
    auto step = [&] { temp = (uint64_t)(uint32_t)temp * 4164903690u + (temp >> 32); };
    float x, y;
    for (;;) {
        const int hz = (int)(uint32_t)temp;
        step();
        const int iz = hz & 127;
        x = (float)hz * z.wn[iz];
        const uint32_t ahz = hz == INT_MIN ? 0x80000000u : (uint32_t)(hz < 0 ? -hz : hz);
        if (ahz < z.kn[iz]) break;
        if (iz == 0) {
            do {
                x = (float)(uint32_t)temp * rng_flt;
                step();
                y = (float)(uint32_t)temp * rng_flt;
                step();
                x = (float)((double)(-logf_d(x + FLT_MIN)) * 0.2904764);
                y = -logf_d(y + FLT_MIN);
            } while (y + y < x * x);
            x = hz > 0 ? r + x : -r - x;
            break;
        }
        y = (float)(uint32_t)temp * rng_flt;
        step();
        if ((double)(z.fn[iz] + y * (z.fn[iz - 1] - z.fn[iz])) < pf_exp(-.5 * (double)x * (double)x)) break;
    }
    state = temp;
    return (double)x * sigma;
}

}  // namespace micv
