// epipolar.hpp -- the end points of one epipolar line (Solution.cpp:343-362 and :124-163), shared by epipolar_kernel
// (geom.hip, micv_epipolar_endpoints_dev) and the display kernel of ps3.hip, which draws the line it has just computed:
// the line of the point, its intersections with the left and the right image border, each scaled by the reciprocal of
// its third coordinate.  include/mi_cv.h, "ps3: geometry", states the order of operations.
#pragma once
#include "common.hpp"

namespace micv {

template <typename R>
__device__ inline void cross3(const R *a, const R *b, R *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// out[0..2] = P_iL, out[3..5] = P_iR of the point (x, y); side 0: l = (p^T F)^T, side 1: l = F p.
template <typename R>
__device__ inline void epipolar_endpoints(const float *__restrict__ F, double x, double y, int side, int rows, int cols, float *out) {
    const R rm1 = (R)(rows - 1), cm1 = (R)(cols - 1);
    const R ul[3] = {0, 0, 1}, bl[3] = {0, rm1, 1}, ur[3] = {cm1, 0, 1}, br[3] = {cm1, rm1, 1};
    R IL[3], IR[3], l[3], PL[3], PR[3];
    cross3<R>(ul, bl, IL);
    cross3<R>(ur, br, IR);
    for (int c = 0; c < 3; c++) {
        double s;
        if (side == 0) {  // (p^T F)^T
            s = x * (double)F[c];
            s = s + y * (double)F[3 + c];
            s = s + 1.0 * (double)F[6 + c];
        } else {  // F p
            s = (double)F[3 * c] * x;
            s = s + (double)F[3 * c + 1] * y;
            s = s + (double)F[3 * c + 2] * 1.0;
        }
        l[c] = (R)s;
    }
    cross3<R>(l, IL, PL);
    cross3<R>(l, IR, PR);
    const R rl = (R)(1.0 / (double)PL[2]), rr = (R)(1.0 / (double)PR[2]);
    for (int c = 0; c < 3; c++) {
        out[c] = (float)(PL[c] * rl);
        out[3 + c] = (float)(PR[c] * rr);
    }
}

}  // namespace micv
