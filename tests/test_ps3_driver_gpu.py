"""The "ps3: driver" block on the device (csrc/ps3.hip) through introtocomputervision_amd/ps3.py, `_dev` and `_host`, against
tests/_ps3_driver_ref.py byte for byte, padding included: segments on every case of the restatement, the epipolar lines of
random fundamental matrices and of one with a vertical line, the one-launch display against the two-step form, and
runProblem2 / runExtraCredit on the reference's point files against geometry.* and the restated drawing."""
import ctypes as C

import numpy as np
import pytest

import _ps3_driver_ref as R
import _ps3_ref as G

pytestmark = pytest.mark.gpu

CASES = R.cases()
EXPECTED = {c[0]: R.apply_case(c) for c in CASES}  # computed once, never written to


def _mods():
    import torch
    from introtocomputervision_amd import geometry, ps3
    return torch, geometry, ps3


def dev_image(torch, ch, pad, rows=R.ROWS, cols=R.COLS):
    buf, _ = R.image(rows, cols, ch, pad)
    t = torch.from_numpy(buf).cuda()
    return t, t.as_strided((rows, cols, ch), (cols * ch + pad, ch, 1))


def test_every_case_on_the_device():
    torch, _, ps3 = _mods()
    for name, ch, pad, segments, colour in CASES:
        buf, view = dev_image(torch, ch, pad)
        ps3.drawSegments(view, torch.from_numpy(segments).cuda(), colour)
        assert np.array_equal(buf.cpu().numpy(), EXPECTED[name]), name


def test_every_case_from_host_memory():
    _, _, ps3 = _mods()
    for name, ch, pad, segments, colour in CASES:
        buf, view = R.image(R.ROWS, R.COLS, ch, pad)
        ps3.drawSegments(view, segments, colour)
        assert np.array_equal(buf, EXPECTED[name]), name


def test_a_grey_two_dimensional_image_and_the_largest_size():
    """[rows, cols] without a channel axis; and 32768 columns, the limit, with a far segment through it."""
    torch, _, ps3 = _mods()
    img = torch.zeros((3, 32768), dtype=torch.uint8, device="cuda")
    seg = np.asarray([[-R.FAR, -1, R.FAR, 3], [32767, -5, 32767, 5]], np.float32)
    ps3.drawSegments(img, torch.from_numpy(seg).cuda(), (200.0,))
    want = np.zeros((3, 32768, 1), np.uint8)
    R.draw_segments(want, seg, (200.0,))
    assert want.any(1).all() and np.array_equal(img.cpu().numpy(), want[:, :, 0])


def random_F(seed):
    rng = np.random.default_rng(seed)
    F = rng.normal(0, 1, (3, 3)).astype(np.float32)
    F[:2, :2] *= np.float32(1e-2)  # lines that cross a 48 x 64 picture at every slope, near-vertical ones included
    return F


def points(seed, n, rows=R.ROWS, cols=R.COLS):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)]).astype(np.float32)  # 2 x n


@pytest.mark.parametrize("ch,pad", [(1, 0), (3, 5), (4, 0)])
def test_draw_epipolar_lines_on_end_points_of_random_F(ch, pad):
    torch, g, ps3 = _mods()
    drawn = 0
    for seed in range(6):
        F, p = random_F(seed), points(100 + seed, 33)
        for side in (0, 1):
            e = g.fundamental.epipolarEndpoints(F, torch.from_numpy(p).cuda(), side, R.ROWS, R.COLS)
            buf, view = dev_image(torch, ch, pad)
            ps3.drawEpipolarLines(view, e, R.GREEN)
            want, wview = R.image(R.ROWS, R.COLS, ch, pad)
            before = want.copy()
            R.draw_epipolar_lines(wview, e.cpu().numpy(), R.GREEN)
            assert np.array_equal(buf.cpu().numpy(), want), (seed, side)
            hbuf, hview = R.image(R.ROWS, R.COLS, ch, pad)
            ps3.drawEpipolarLines(hview, e.cpu().numpy(), R.GREEN)
            assert np.array_equal(hbuf, want), (seed, side)
            drawn += int((want != before).sum())
    assert drawn > 2000


def test_a_vertical_epipolar_line_leaves_the_image_untouched():
    """F p = (a, 0, c) for every p: l_1 = 0, the line meets neither border, its end points are NaN / inf."""
    torch, g, ps3 = _mods()
    F = np.asarray([[0, 0, 1], [0, 0, 0], [0, 0, -20]], np.float32)
    p = points(7, 9)
    e = g.fundamental.epipolarEndpoints(F, torch.from_numpy(p).cuda(), 1, R.ROWS, R.COLS)
    en = e.cpu().numpy()
    assert not np.isfinite(en[:, [0, 1, 3, 4]]).all(1).any()
    assert all(R.cv_round(v) == R.INT_MIN for v in en[:, [0, 3]].ravel())
    buf, view = dev_image(torch, 3, 5)
    before = buf.cpu().numpy().copy()
    ps3.drawEpipolarLines(view, e, R.GREEN)
    assert np.array_equal(buf.cpu().numpy(), before)
    outA, outB = ps3.epipolarDisplay(F, torch.from_numpy(p).cuda(), torch.from_numpy(p).cuda(), view, view)
    assert np.array_equal(outB.cpu().numpy(), view.cpu().numpy())  # side 1 is the vertical one


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_epipolar_display_equals_end_points_then_lines(dev, f64):
    """Two pictures of different sizes, with padding; into copies, in place, with and without the end points."""
    torch, g, ps3 = _mods()
    F, pa, pb = random_F(11), points(12, 70, 40, 56), points(13, 70)
    bufA, viewA = R.image(R.ROWS, R.COLS, 3, 5)
    bufB, viewB = R.image(40, 56, 3, 2)
    eA = g.fundamental.epipolarEndpoints(F, pb, 0, R.ROWS, R.COLS, f64=f64)
    eB = g.fundamental.epipolarEndpoints(F, pa, 1, 40, 56, f64=f64)
    assert np.array_equal(eA, G.epipolar_endpoints(F, pb.T, 0, R.ROWS, R.COLS, f64=f64), equal_nan=True)
    wantA, wA = R.image(R.ROWS, R.COLS, 3, 5)
    wantB, wB = R.image(40, 56, 3, 2)
    R.draw_epipolar_lines(wA, eA, R.GREEN)
    R.draw_epipolar_lines(wB, eB, R.GREEN)
    assert not np.array_equal(wantA, bufA) and not np.array_equal(wantB, bufB)
    if dev:
        tA, tB = torch.from_numpy(bufA).cuda(), torch.from_numpy(bufB).cuda()
        vA = tA.as_strided((R.ROWS, R.COLS, 3), (R.COLS * 3 + 5, 3, 1))
        vB = tB.as_strided((40, 56, 3), (56 * 3 + 2, 3, 1))
        Fd, da, db = (torch.from_numpy(x).cuda() for x in (F, pa, pb))
        host = lambda t: t.cpu().numpy()
    else:
        tA, tB, vA, vB, Fd, da, db = bufA, bufB, viewA, viewB, F, pa, pb
        host = lambda t: t
    outA, outB, ends = ps3.epipolarDisplay(Fd, da, db, vA, vB, f64=f64, endpoints=True)
    assert np.array_equal(host(outA), wA) and np.array_equal(host(outB), wB)
    assert np.array_equal(host(ends).view(np.uint32), np.stack([eA, eB]).view(np.uint32))
    assert np.array_equal(host(tA), R.image(R.ROWS, R.COLS, 3, 5)[0])  # the pictures stay as they are
    outA, outB = ps3.epipolarDisplay(Fd, da, db, vA, vB, f64=f64)
    assert np.array_equal(host(outA), wA) and np.array_equal(host(outB), wB)
    ps3.epipolarDisplay(Fd, da, db, vA, vB, f64=f64, inplace=True)
    assert np.array_equal(host(tA), wantA) and np.array_equal(host(tB), wantB)  # padding included


def golden_pictures():
    rng = np.random.default_rng(323)
    return rng.integers(0, 256, (712, 1072, 3), dtype=np.uint8), rng.integers(0, 256, (700, 1060, 3), dtype=np.uint8)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_run_problem_2_and_extra_credit_on_the_golden_points(dev):
    torch, g, ps3 = _mods()
    pts = G.load_all()
    pa, pb = np.ascontiguousarray(pts["a"].T), np.ascontiguousarray(pts["b"].T)  # 2 x n
    picA, picB = golden_pictures()
    up = (lambda x: torch.from_numpy(x).cuda()) if dev else (lambda x: x)
    host = (lambda t: t.cpu().numpy()) if dev else (lambda t: t)

    def drawn(F):
        wA, wB = picA.copy(), picB.copy()
        eA = g.fundamental.epipolarEndpoints(host(F), pb, 0, 712, 1072)
        eB = g.fundamental.epipolarEndpoints(host(F), pa, 1, 700, 1060)
        R.draw_epipolar_lines(wA, eA, R.GREEN)
        R.draw_epipolar_lines(wB, eB, R.GREEN)
        assert ((wA != picA).any(2).sum() > 5000) and ((wB != picB).any(2).sum() > 5000)
        return wA, wB

    est, F, outA, outB = ps3.runProblem2(up(pa), up(pb), up(picA), up(picB))
    assert np.array_equal(host(est), g.fundamental.solveLeastSquares(pa, pb).reshape(3, 3))
    assert np.array_equal(host(F), g.fundamental.rankReduce(host(est)))
    wA, wB = drawn(F)
    assert np.array_equal(host(outA), wA) and np.array_equal(host(outB), wB)

    Ta, Tb, Fh, F2, outA, outB = ps3.runExtraCredit(up(pa), up(pb), up(picA), up(picB))
    for got, want in zip((Ta, Tb, Fh, F2), g.fundamental.normalized(pa, pb)):
        assert np.array_equal(host(got), want)
    wA, wB = drawn(F2)
    assert np.array_equal(host(outA), wA) and np.array_equal(host(outB), wB)


def test_bad_arguments_are_refused_before_anything_runs():
    torch, _, ps3 = _mods()
    from introtocomputervision_amd._capi import EINVAL, lib
    from introtocomputervision_amd.lk import _ctx_for
    img = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    seg = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
    ctx = _ctx_for(img, None).handle
    col = (C.c_double * 4)(0, 255, 0, 0)
    assert lib.micv_draw_segments_dev(ctx, img.data_ptr(), 8, 8, 2, 24, seg.data_ptr(), 2, col, None) == EINVAL
    assert lib.micv_draw_segments_dev(ctx, img.data_ptr(), 8, 8, 3, 23, seg.data_ptr(), 2, col, None) == EINVAL
    assert lib.micv_draw_segments_dev(ctx, img.data_ptr(), 8, 32769, 3, 32769 * 3, seg.data_ptr(), 2, col, None) == EINVAL
    assert lib.micv_draw_segments_dev(ctx, img.data_ptr(), 8, 8, 3, 24, None, 2, col, None) == EINVAL
    assert lib.micv_draw_epipolar_lines_dev(ctx, img.data_ptr(), 8, 8, 3, 24, seg.data_ptr(), -1, col, None) == EINVAL
    torch.cuda.synchronize()
    assert not img.any()
    assert ps3.drawSegments(img, torch.zeros((0, 4), dtype=torch.float32, device="cuda")) is img  # n = 0: a no-op
