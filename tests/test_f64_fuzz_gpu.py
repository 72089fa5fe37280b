"""A derandomized hypothesis fuzz of all three float pipelines against the float64 bounds (tests/_f64_ref.py): small
shapes, row pitches, image kinds, LK windows and dispatch forms, Harris arithmetics, NCC radii, ranges and COLS_2R.
Its own module, so that a missing hypothesis skips only this test (tests/test_f64_bounds_gpu.py holds the rest)."""
import pytest

import _f64_ref as F
from test_f64_bounds_gpu import check_ncc, lk_pair, run_harris, run_lk, run_ncc
from test_f64_ref import check_lk, harris_outside, report

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")
pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, given, settings  # noqa: E402
from hypothesis import strategies as st  # noqa: E402


@settings(max_examples=100, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck), print_blob=True)
@given(st.tuples(st.integers(1, 70), st.integers(1, 140)), st.sampled_from([0, 1, 3, 64]), st.integers(0, 2 ** 31 - 1),
       st.sampled_from(["smooth", "uniform", "flat", "normal", "u8"]), st.sampled_from([1, 3, 5, 7, 15, 21, 43]),
       st.sampled_from([0, 1, 2, 3]), st.integers(0, 11), st.integers(-20, 5), st.integers(0, 30),
       st.sampled_from([0, F.COLS_2R, F.ROLLING, F.ROLLING | F.COLS_2R]))
def test_fuzz_all_three(shape, pad, seed, kind, win, form, rad, dmin, span, flags):
    rows, cols = shape
    prev, nxt = lk_pair(seed, rows, cols, kind)
    u, v = run_lk(prev, nxt, win, form, pad)
    check_lk(u, v, F.lk_flow(prev, nxt, win), f"fuzz lk {shape} pad {pad} {kind} win {win} form {form}")
    gx, gy = nxt, prev  # any finite fields will do as gradients
    hw = min(win, 63)
    R = run_harris(gx, gy, hw, hw / 3.0, ["default", "generic", "cpu"][form % 3], pad=pad)
    ref = F.harris_response(gx, gy, hw, hw / 3.0, 0.04)
    report(harris_outside(R, ref), R, ref[0], ref[1], f"fuzz harris {shape} {kind} win {hw}")
    flags = flags & ~F.COLS_2R if rad == 0 else flags  # COLS_2R at radius 0 is refused (an empty window)
    got = run_ncc(prev, nxt, rad, dmin, dmin + span, flags, pad=pad)
    check_ncc(prev, nxt, rad, dmin, dmin + span, flags, got, f"fuzz ncc {shape} pad {pad} {kind} r {rad} flags {flags}")
