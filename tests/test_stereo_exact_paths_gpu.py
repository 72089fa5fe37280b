"""disparitySSD's exact-sum dispatch (csrc/stereo_exact.hip) path by path.  Every case runs the call twice -- on a
context that takes the exact-sum kernels when the pre-pass finds an 8-bit-valued pair (the default) and on one that never
does (MICV_OPT_STEREO_EXACT = -1) -- and compares both byte for byte with an independent answer: the exact integer
reference (tests/_stereo_ref.py) on 8-bit-valued pairs, the order-exact float32 reference (tests/_stereo_f32_ref.py)
otherwise (NaN and infinite pixels included); neither shares code with the C oracle.

  - every search-kernel instantiation stereo_exact_covers() can select, under 8 and 10 rows per float strip, on 8-bit pairs
    and on the same pairs with one pixel 0.5 (the float tiles that ride in the exact-sum launch), through a covering table
    that rotates disparity spans (1..4 chunks of 64, each chunk edge), rows, columns, row pitch and MIN_SSD_5E6;
  - ties across lanes and across 64-disparity chunks (periodic, constant, two-level pairs) and serial:: edge positions;
  - the largest window costs the 8-bit range allows, and MIN_SSD_5E6 splitting an image into -1 and valid disparities;
  - one bad pixel (not an integer in 0..255) anywhere the pre-pass must find it, then a clean call on the same context;
  - the reference's stereo geometry and 1080p, at size;
  - SERIAL with a CUDA-path flag: refused before anything runs, the output left as it was."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _stereo_f32_ref as fref
import _stereo_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COLS_2R, MIN_SSD_5E6, SERIAL = 1, 2, 4


def dev(a, pad=0):
    """Device copy of a 2-D float array; pad > 0 gives it a row pitch of cols + pad elements."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if pad == 0:
        return torch.from_numpy(a).cuda()
    wide = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=torch.float32, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return wide[:, :a.shape[1]]


@pytest.fixture(scope="module")
def ctxs():
    """(exact-sum kernels allowed = the default, float kernels only)."""
    from introtocomputervision_amd._capi import Context, OPT_STEREO_EXACT
    exact, flt = Context(0), Context(0)
    exact.set_option(OPT_STEREO_EXACT, 0)
    flt.set_option(OPT_STEREO_EXACT, -1)
    yield exact, flt
    exact.close()
    flt.close()


def set_rpw(ctxs, rpw):
    from introtocomputervision_amd._capi import OPT_STEREO_ROWS
    for c in ctxs:
        c.set_option(OPT_STEREO_ROWS, rpw)


def is_u8(img):
    return bool(np.all(np.isfinite(img)) and np.all(img == np.round(img)) and img.min() >= 0 and img.max() <= 255)


def expected(left, right, rad, lo, hi, flags):
    """The exact integer reference on 8-bit-valued pairs, the order-exact float32 reference otherwise."""
    if is_u8(left) and is_u8(right):
        return ref.ssd_serial(left, right, rad, lo, hi) if flags & SERIAL else ref.ssd_cuda(left, right, rad, lo, hi, flags)
    if flags & SERIAL:
        return fref.ssd_serial_f32(left, right, rad, lo, hi)
    return fref.ssd_f32(left, right, rad, lo, hi, flags)


def run_both(ctxs, left, right, rad, lo, hi, flags, pad=0):
    from introtocomputervision_amd import stereo
    dl, dr = dev(left, pad), dev(right, pad)
    return [stereo.disparitySSD(dl, dr, rad, lo, hi, flags, ctx=c).cpu().numpy() for c in ctxs]


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.int8, what
    bad = got != exp
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {len(idx)} of {exp.size} pixels differ, first {idx[:4].tolist()}: "
                             f"got {got[bad][:4].tolist()}, want {exp[bad][:4].tolist()}")


def check(ctxs, left, right, rad, lo, hi, flags, pad=0, exp=None, what=""):
    if exp is None:
        exp = expected(left, right, rad, lo, hi, flags)
    got_exact, got_float = run_both(ctxs, left, right, rad, lo, hi, flags, pad)
    what = f"{what} {left.shape} r={rad} [{lo}, {hi}] flags={flags} pad={pad}"
    same(got_exact, exp, "default context " + what)
    same(got_float, exp, "float-only context " + what)
    return exp


def u8_pair(rng, rows, cols, kind):
    if kind == "noise":  # a shifted copy with every third row replaced: a clear minimum on most rows
        left = rng.integers(0, 256, (rows, cols))
        right = np.roll(left, int(rng.integers(-20, 21)), axis=1)
        right[::3] = rng.integers(0, 256, right[::3].shape)
    else:  # three grey levels: equal costs everywhere
        left = rng.integers(0, 3, (rows, cols)) * 127
        right = rng.integers(0, 3, (rows, cols)) * 127
    return left.astype(np.float32), right.astype(np.float32)


# ---- 1. every instantiation the dispatch can select ------------------------------------------------------------------
# stereo_exact_kernel<R, WC, MODE, RPW>: full window r 1..7, COLS_2R r 2..7, serial:: r 1..5 (tools/audit_asm_loads.py's
# REQUIRED_SCALAR lists the same set).  The other dimensions rotate through the table.
FORMS = [(r, "full", "ssd") for r in range(1, 8)] + [(r, "2R", "ssd") for r in range(2, 8)] + \
        [(r, "full", "serial") for r in range(1, 6)]
SPANS = (0, 63, 64, 65, 127, 128, 191, 192, 255)  # 1..4 chunks of 64 disparities, each chunk edge
ROWS = (1, 7, 8, 9, 33, 41)                          # around SX_Y = 8 and the float tiles' 4 x RPW rows


def cols_for(r, k):
    """Around the float tile width 64 - 2r, the exact-sum tile's XMAX = 128, and the window itself."""
    return (1, 2 * r, 2 * r + 1, 63 - 2 * r, 64 - 2 * r, 127, 128, 129, 257)[k % 9]


COVER = []
for _rpw in (8, 10):
    for _img in ("u8", "frac"):
        for _form in FORMS:
            COVER.append(pytest.param(len(COVER), *_form, _rpw, _img,
                                      id=f"r{_form[0]}-{_form[1]}-{_form[2]}-rpw{_rpw}-{_img}"))


@pytest.mark.parametrize("i,rad,window,mode,rpw,img", COVER)
def test_every_exact_sum_form(ctxs, i, rad, window, mode, rpw, img):
    set_rpw(ctxs, rpw)
    rng = np.random.default_rng(9000 + i)
    span = SPANS[(i * 5) % 9]
    rows = ROWS[(i * 7 + rpw) % 6]
    cols = cols_for(rad, i * 4 + (img == "frac"))
    pad = 3 * (i % 2)
    lo = int(rng.integers(-128, 128 - span))  # wholly negative, wholly positive or across 0, by draw
    flags = SERIAL if mode == "serial" else (COLS_2R if window == "2R" else 0) | (MIN_SSD_5E6 if i % 3 == 1 else 0)
    left, right = u8_pair(rng, rows, cols, ("noise", "levels")[(i // 3) % 2])
    if flags & MIN_SSD_5E6:  # a dark half against a bright one: both -1 and found disparities in the output
        right[:, cols // 2:] = 255 - right[:, cols // 2:]
    if img == "frac":
        (left if i % 2 else right)[int(rng.integers(0, rows)), int(rng.integers(0, cols))] = 0.5
    check(ctxs, left, right, rad, lo, lo + span, flags, pad=pad, what=img)


# ---- 2. ties across lanes and chunks ---------------------------------------------------------------------------------
TIE_FORMS = [(1, 0, 8), (3, COLS_2R, 10), (4, 0, 10), (6, COLS_2R, 8), (7, 0, 8), (7, COLS_2R, 10), (2, SERIAL, 8),
             (5, SERIAL, 10)]


def tie_pairs(rng, rows, cols):
    out = []
    for period in (64, 32, 1):
        base = rng.integers(0, 256, (rows, period))
        left = np.tile(base, (1, cols // period + 1))[:, :cols]
        out.append((f"period {period}", left, np.roll(left, int(rng.integers(0, period)), axis=1)))
        stripes = np.tile(rng.integers(0, 256, (1, period)), (rows, cols // period + 1))[:, :cols]  # vertical stripes
        out.append((f"stripes {period}", stripes, np.roll(stripes, 5, axis=1)))
    out.append(("constant", np.full((rows, cols), 77), np.full((rows, cols), 77)))
    out.append(("constant apart", np.full((rows, cols), 0), np.full((rows, cols), 255)))
    out.append(("two levels", rng.integers(0, 2, (rows, cols)) * 255, rng.integers(0, 2, (rows, cols)) * 255))
    return [(n, l.astype(np.float32), r.astype(np.float32)) for n, l, r in out]


@pytest.mark.parametrize("rad,flags,rpw", TIE_FORMS, ids=[f"r{r}-f{f}-rpw{p}" for r, f, p in TIE_FORMS])
def test_ties_go_to_the_lowest_disparity_across_chunks(ctxs, rad, flags, rpw):
    """SSD(d) = SSD(d + 64) exactly on pairs periodic in x with period 64 (32, 1): the lowest d must win across every
    chunk boundary, where the exact-sum kernels compare in a separate step after the arg max."""
    set_rpw(ctxs, rpw)
    rng = np.random.default_rng(rad * 31 + flags)
    for lo, hi in ((-128, 127), (-100, 91), (0, 127)):
        for name, left, right in tie_pairs(rng, 19, 203):
            check(ctxs, left, right, rad, lo, hi, flags, what=name)


@pytest.mark.parametrize("rad", [1, 3, 5])
def test_serial_best_at_the_padded_image_edge(ctxs, rad):
    """serial:: searches positions -r .. cols - 1 + r only: ramps that put the unique best position exactly on either edge
    of the padded image, and ranges that reach past it (the invalid positions' keys must lose) or lie wholly outside it
    (no position searched: 0)."""
    set_rpw(ctxs, 8)
    rows, cols = 13, 90
    ramp = np.tile(np.arange(cols, dtype=np.float32), (rows, 1))
    cases = [(np.full((rows, cols), 255, np.float32), ramp),  # best: right edge, p = cols - 1 + r
             (np.zeros((rows, cols), np.float32), ramp),       # best: left edge, p = -r
             (ramp, ramp[:, ::-1].copy())]
    for left, right in cases:
        for lo, hi in ((-128, 127), (-128, -60), (60, 127), (cols + rad - 1, 127), (-128, -(cols + rad))):
            check(ctxs, left, right, rad, lo, hi, SERIAL, what="serial edge")
    exp = check(ctxs, cases[0][0], cases[0][1], rad, -128, 127, SERIAL)
    assert (exp[:, cols - 30:] == (cols - 1 + rad) - np.arange(cols - 30, cols)).all()  # the edge position itself


# ---- 3. the largest costs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rad,flags", [(7, 0), (7, COLS_2R), (5, SERIAL)], ids=["r7-full", "r7-2R", "r5-serial"])
def test_largest_costs(ctxs, rad, flags):
    """All-255 against all-0, a 0 / 255 checkerboard against its inverse, row stripes against their inverse: window sums
    up to 225 * 255^2 = 14 630 625 < 2^24 at r = 7, where the key (2C - B) * 64 - idx is at its extremes."""
    set_rpw(ctxs, 10)
    rows, cols = 37, 150
    yy, xx = np.mgrid[0:rows, 0:cols]
    cb = ((yy + xx) % 2 * 255).astype(np.float32)
    st = (yy % 2 * 255).astype(np.float32)
    pairs = [("255 vs 0", np.full((rows, cols), 255, np.float32), np.zeros((rows, cols), np.float32)),
             ("checkerboard", cb, 255 - cb), ("row stripes", st, 255 - st)]
    for name, left, right in pairs:
        for lo, hi in ((-128, 127), (0, 0), (-64, 63)):
            exp = check(ctxs, left, right, rad, lo, hi, flags, what=name)
            check(ctxs, right, left, rad, lo, hi, flags, what=name + " swapped")
            if name == "row stripes" and not flags & SERIAL:
                assert (exp == lo).all()  # every cost is the maximum: the lowest disparity everywhere
    if flags & SERIAL:
        return
    # MIN_SSD_5E6: a bright band of 10 rows in an otherwise equal pair -- windows that overlap it by 6 rows or more cost
    # at least 6 * 14 * 255^2 > 5e6 (-1), the others 0 (found)
    left = np.zeros((rows, cols), np.float32)
    right = left.copy()
    right[12:22] = 255
    for lo, hi in ((-128, 127), (-5, 5)):
        exp = check(ctxs, left, right, rad, lo, hi, flags | MIN_SSD_5E6, what="5e6 band")
        assert (exp == -1).any() and (exp == lo).any()


# ---- 4. bad pixels the pre-pass must find ----------------------------------------------------------------------------
BAD_VALUES = [0.5, 255.5, -1.0, 256.0, 1e-45, np.inf, -np.inf, np.nan, -0.0]
BAD_FORMS = [(1, 0, -40, 10, 8), (5, 0, -70, 0, 8), (7, COLS_2R, -128, 127, 10)]


@pytest.mark.parametrize("rad,flags,lo,hi,rpw", BAD_FORMS, ids=["r1", "r5", "r7-2R-4chunks-rpw10"])
def test_one_bad_pixel_anywhere(ctxs, rad, flags, lo, hi, rpw):
    """One pixel that is not an integer in 0..255 -- a fraction, 255.5, a negative, 256, a denormal, +-inf, NaN -- in
    either image: at each corner, in the last row of a partial 8-row strip, in the last column, and in a right-image
    column reached only through clamping.  The call must equal the float32 reference (the float kernels did it); the next call on
    the same context with a clean pair must equal the exact reference.  -0.0 is a legal 0: same bytes on either path."""
    set_rpw(ctxs, rpw)
    rows, cols = 21, 70  # strips 0..7, 8..15 and the partial 16..20
    rng = np.random.default_rng(rad)
    spots = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows - 1, cols // 2), (rows // 2, cols - 1)]
    places = [(side, y, x, lo, hi) for side in (0, 1) for y, x in spots]
    # right column 0 when every fetch x + d + window column lies left of the image: reached only by clamping
    places.append((1, rows // 2, 0, -128, -(cols + rad)))
    n = 0
    for bad in BAD_VALUES:
        for side, y, x, plo, phi in places:
            left, right = u8_pair(rng, rows, cols, "noise")
            (left if side == 0 else right)[y, x] = bad
            exp = expected(left, right, rad, plo, phi, flags)
            check(ctxs, left, right, rad, plo, phi, flags, exp=exp, what=f"bad {bad} at {'LR'[side]}{(y, x)}")
            l2, r2 = u8_pair(rng, rows, cols, "noise")
            check(ctxs, l2, r2, rad, plo, phi, flags, what="clean after bad")
            n += 1
    assert n == len(BAD_VALUES) * len(places)


# ---- 5. at size ------------------------------------------------------------------------------------------------------
def _refs(jobs):
    """The exact references of several calls, computed side by side (numpy releases the GIL in the array loops)."""
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
        return list(ex.map(lambda j: expected(*j), jobs))


def _quantised_pair(seed, rows, cols):
    from introtocomputervision_amd import synth
    left, right, _ = synth.stereo_pair(seed, rows, cols)
    q = lambda a: np.clip(np.round(a), 0, 255).astype(np.float32)  # noqa: E731
    return q(left), q(right)


def test_reference_geometry_at_size(ctxs):
    """The reference's own stereo case: 640 x 511, r = 7, 95 disparities, left-reference [-95, 0] and right-reference
    [0, 95], with the as-written CUDA flags COLS_2R | MIN_SSD_5E6 and with none; serial:: at r = 6 / 7 (float kernels)."""
    set_rpw(ctxs, 0)
    rows, cols = 640, 511
    rng = np.random.default_rng(640)
    pairs = [_quantised_pair(0x5EED0002, rows, cols)]
    noise = rng.integers(0, 256, (rows, cols)).astype(np.float32)
    pairs.append((noise, np.roll(noise, -11, axis=1)))
    jobs = []
    for left, right in pairs:
        for flags in (COLS_2R | MIN_SSD_5E6, 0):
            jobs.append((left, right, 7, -95, 0, flags))
            jobs.append((right, left, 7, 0, 95, flags))
    left, right = pairs[0]
    jobs += [(left, right, 6, -95, 0, SERIAL), (right, left, 7, 0, 95, SERIAL)]
    for job, exp in zip(jobs, _refs(jobs)):
        check(ctxs, *job, exp=exp, what="reference geometry")


def test_1080p_at_size(ctxs):
    """1080 x 1920 with the rows per strip chosen automatically (10 here): r 1..7 over [-127, 0], the whole int8 range
    once, COLS_2R, MIN_SSD_5E6 and serial:: once each -- against the exact reference."""
    set_rpw(ctxs, 0)
    left, right = _quantised_pair(0x5EED0002, 1080, 1920)
    jobs = [(left, right, r, -127, 0, 0) for r in range(1, 8)]
    jobs += [(left, right, 3, -128, 127, 0), (left, right, 6, -127, 0, COLS_2R), (left, right, 4, -127, 0, MIN_SSD_5E6),
             (left, right, 5, -127, 0, SERIAL)]
    with ThreadPoolExecutor(max_workers=1) as gpu_side:  # the GPU calls run while the references are computed
        got = gpu_side.submit(lambda: [run_both(ctxs, *j) for j in jobs])
        exps = _refs(jobs)
        got = got.result()
    for job, exp, (ge, gf) in zip(jobs, exps, got):
        what = f"1080p r={job[2]} [{job[3]}, {job[4]}] flags={job[5]}"
        same(ge, exp, "default context " + what)
        same(gf, exp, "float-only context " + what)


# ---- SERIAL with a CUDA-path flag ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [SERIAL | COLS_2R, SERIAL | MIN_SSD_5E6, SERIAL | COLS_2R | MIN_SSD_5E6])
def test_serial_with_cuda_flags_is_refused(ctxs, flags):
    """serial::disparitySSD has a (2r+1)^2 window and no threshold: SERIAL with COLS_2R or MIN_SSD_5E6 is MICV_EINVAL, on
    either context, device and host entry, every radius -- and the output buffer is left exactly as it was.  (The exact-
    sum path used to enqueue its pre-pass and then return MICV_EUNSUPPORTED with no message, disp never written.)"""
    from introtocomputervision_amd import _capi
    rows, cols = 19, 50
    rng = np.random.default_rng(flags)
    left, right = u8_pair(rng, rows, cols, "noise")
    dl, dr = dev(left), dev(right)
    hl, hr = np.ascontiguousarray(left), np.ascontiguousarray(right)
    for rad in range(1, 8):
        for c in ctxs:
            ddisp = torch.full((rows, cols), 77, dtype=torch.int8, device="cuda")
            rc = _capi.lib.micv_disparity_ssd_dev(c.handle, dl.data_ptr(), dr.data_ptr(), rows, cols, cols * 4, rad, -20, 0,
                                                  flags, ddisp.data_ptr(), cols, None)
            msg = _capi.last_error()
            torch.cuda.synchronize()
            assert rc == _capi.EINVAL and "serial::disparitySSD" in msg, (rad, rc, msg)
            assert (ddisp.cpu().numpy() == 77).all()
            hdisp = np.full((rows, cols), 77, np.int8)
            rc = _capi.lib.micv_disparity_ssd_host(c.handle, hl.ctypes.data, hr.ctypes.data, rows, cols, cols * 4, rad, -20,
                                                   0, flags, hdisp.ctypes.data, cols)
            msg = _capi.last_error()
            assert rc == _capi.EINVAL and "serial::disparitySSD" in msg, (rad, rc, msg)
            assert (hdisp == 77).all()
            with pytest.raises(_capi.MicvError, match="serial::disparitySSD"):
                from introtocomputervision_amd import stereo
                stereo.disparitySSD(dl, dr, rad, -20, 0, flags, ctx=c)
    # the context still works: the same call without the CUDA-path flags
    for c in ctxs:
        from introtocomputervision_amd import stereo
        same(stereo.disparitySSD(dl, dr, 3, -20, 0, SERIAL, ctx=c).cpu().numpy(), ref.ssd_serial(left, right, 3, -20, 0),
             "serial after refusal")
