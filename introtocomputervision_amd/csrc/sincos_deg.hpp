// sincos_deg.hpp -- the fixed sine / cosine polynomial of the SIFT descriptor window (sift.hip), shared with the keypoint
// glyphs of ps4.hip, so that the two turn an angle into the same direction.  tests/_ps4_feat_ref.py restates it.
#pragma once
#include "common.hpp"

namespace micv {

// sin / cos of `deg` degrees: quadrant by float arithmetic, Taylor polynomials as fmaf chains.
__device__ __forceinline__ void sincos_deg(float deg, float &s, float &c) {
    float t = deg / 360.f;
    t = t - floorf(t);
    const float x = t * 4.f;
    int q = (int)x;
    const float f = x - (float)q;
    q &= 3;
    const float y = f * 1.57079632679489662f, y2 = y * y;
    float ps = -2.50521083854417188e-8f;
    ps = fmaf(ps, y2, 2.75573192239858907e-6f);
    ps = fmaf(ps, y2, -1.98412698412698413e-4f);
    ps = fmaf(ps, y2, 8.33333333333333333e-3f);
    ps = fmaf(ps, y2, -1.66666666666666667e-1f);
    ps = fmaf(ps, y2, 1.f);
    const float sy = ps * y;
    float pc = 2.08767569878680990e-9f;
    pc = fmaf(pc, y2, -2.75573192239858907e-7f);
    pc = fmaf(pc, y2, 2.48015873015873016e-5f);
    pc = fmaf(pc, y2, -1.38888888888888889e-3f);
    pc = fmaf(pc, y2, 4.16666666666666667e-2f);
    pc = fmaf(pc, y2, -0.5f);
    pc = fmaf(pc, y2, 1.f);
    switch (q) {
        case 0: s = sy; c = pc; break;
        case 1: s = pc; c = -sy; break;
        case 2: s = -sy; c = -pc; break;
        default: s = -pc; c = sy; break;
    }
}

}  // namespace micv
