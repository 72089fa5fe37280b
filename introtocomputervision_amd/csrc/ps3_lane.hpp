// ps3_lane.hpp -- one lane of the segment kernel (ps3.hip), in plain C++ so that the same text also compiles for the
// host: tools/probes/ps3_host_loops.cpp (`lanes`) runs every lane of every test case on the CPU under the address and
// undefined-behaviour sanitizers and the pictures must equal the host loop's (tests/test_ps3_driver_shim.py).
//
// The contract is micv_ps3::line_wide (shim/micv_ps3.hpp): micv_viz::line for any two int32 points, which is draw.hpp's
// clip with the WIDE form of the minor advance.
#pragma once
#include "draw.hpp"

namespace micv {

// Lane `lane` of `lanes` paints steps i0 + lane, i0 + lane + lanes, ... of the segment (fx1, fy1) -> (fx2, fy2).
MICV_HD inline void seg_lane(const draw::Target &t, uint32_t colour, float fx1, float fy1, float fx2, float fy2, int lane, int lanes) {
    const draw::LineWalk w = draw::line_walk(t.rows, t.cols, draw::cv_round_i32(fx1), draw::cv_round_i32(fy1), draw::cv_round_i32(fx2),
                                             draw::cv_round_i32(fy2));
    draw::walk_steps(w, lane, lanes, draw::wide_minor(w), [&](long long x, long long y) { draw::put(t, x, y, colour); });
}

}  // namespace micv
