"""disparitySSD on 8-bit images: micv_disparity_ssd_u8_dev / _host / _batch_dev (stereo.disparitySSD8, disparitySSD8Batch).

The contract (include/mi_cv.h): the bytes of micv_disparity_ssd_dev on the images converted to float32, from byte images of
any alignment and pitch, a batch of pairs in one launch pair, nothing written outside rows x cols of a pair.  The expected
bytes come from the exact integer reference (tests/_stereo_ref.py, numpy only); for the forms it does not cover (ROLLING at
a radius the exact-sum kernels do not take, radius 0) from the library's f32 entry on the converted pair -- whose own
tests are test_stereo_exact_paths_gpu.py and test_stereo_float_paths_gpu.py."""
import numpy as np
import pytest

import _stereo_ref as ref
from _host_pitch import strided_host

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COLS_2R, MIN_SSD_5E6, SERIAL, ROLLING = 1, 2, 4, 8
SENTINEL = 0xA5
SENTINEL_I8 = np.uint8(SENTINEL).view(np.int8)


def view8(a, off=0, pad=0, tail=0):
    """`a` (uint8, [..., rows, cols]) as a device view into a larger byte block filled with the sentinel: first byte at
    `off`, row pitch cols + pad, and for a batch `tail` more bytes between pairs.  -> (block, view)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    rows, cols = a.shape[-2:]
    pitch = cols + pad
    if a.ndim == 2:
        size, shape, strides = (off + rows * pitch, (rows, cols), (pitch, 1))
    else:
        pair = rows * pitch + tail
        size, shape, strides = (off + a.shape[0] * pair, (a.shape[0], rows, cols), (pair, pitch, 1))
    block = torch.full((size + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(block, shape, strides, off)
    view.copy_(torch.from_numpy(a).cuda())
    return block, view


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def f32_entry(ctx, left, right, rad, lo, hi, flags):
    """The library's f32 entry on the converted pair."""
    from introtocomputervision_amd import stereo
    dl, dr = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in (left, right))
    return stereo.disparitySSD(dl, dr, rad, lo, hi, flags, ctx=ctx).cpu().numpy()


def expected(left, right, rad, lo, hi, flags):
    if flags & SERIAL:
        return ref.ssd_serial(left, right, rad, lo, hi)
    return ref.ssd_cuda(left, right, rad, lo, hi, flags & (COLS_2R | MIN_SSD_5E6))


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.int8, what
    bad = got != exp
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{what}: {len(idx)} of {exp.size} pixels differ, first {idx[:4].tolist()}: "
                             f"got {got[bad][:4].tolist()}, want {exp[bad][:4].tolist()}")


def run8(ctx, left, right, rad, lo, hi, flags):
    from introtocomputervision_amd import stereo
    return stereo.disparitySSD8(dev8(left), dev8(right), rad, lo, hi, flags, ctx=ctx).cpu().numpy()


def pair8(rng, rows, cols, shift=None):
    """A shifted copy with every third row replaced: a clear minimum on most rows."""
    left = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    right = np.roll(left, int(rng.integers(-20, 21)) if shift is None else shift, axis=1)
    right[::3] = rng.integers(0, 256, right[::3].shape, dtype=np.uint8)
    return left, right


# ---- 1. every form on bytes ------------------------------------------------------------------------------------------
FORMS = [(r, f | t) for r in range(1, 8) for f in (0, COLS_2R) if not (f and r < 2) for t in (0, MIN_SSD_5E6)] + \
        [(r, SERIAL) for r in range(1, 6)]
SPANS = (0, 63, 64, 65, 127, 128, 255)  # 1..4 chunks of 64 disparities and each chunk edge
ROWS = (1, 7, 8, 9, 17)
COLS = (1, 5, 63, 64, 65, 129, 200)     # a wave takes at most 128 columns: 129 and 200 have two column strips


@pytest.mark.parametrize("i,rad,flags", [pytest.param(i, r, f, id=f"r{r}-f{f}") for i, (r, f) in enumerate(FORMS)])
def test_every_form_on_bytes(ctx, i, rad, flags):
    rng = np.random.default_rng(8000 + i)
    for k in range(3):  # three rotations of the table per form
        span, rows, cols = SPANS[(i * 3 + k * 5) % 7], ROWS[(i + k * 2) % 5], COLS[(i * 2 + k * 3) % 7]
        lo = int(rng.integers(-128, 128 - span))
        left, right = pair8(rng, rows, cols)
        if flags & MIN_SSD_5E6:  # a half against its inverse: -1 and found disparities
            right[:, cols // 2:] = 255 - right[:, cols // 2:]
        same(run8(ctx, left, right, rad, lo, lo + span, flags), expected(left, right, rad, lo, lo + span, flags),
             f"{rows}x{cols} r={rad} [{lo}, {lo + span}] flags={flags}")


# ---- 2. alignment ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loff,roff", [(1, 2), (2, 3), (3, 1)])
def test_any_alignment_and_pitch(ctx, loff, roff):
    """Views into larger byte blocks at 1, 2, 3 bytes past an aligned address, odd row pitches that differ between the
    images, and a padded output: the aligned call's bytes, the padding untouched."""
    from introtocomputervision_amd import _capi
    rng = np.random.default_rng(loff * 10 + roff)
    for rows, cols, rad, flags, lo, hi in ((17, 200, 5, COLS_2R | MIN_SSD_5E6, -70, 0), (9, 129, 7, 0, -128, 127),
                                           (8, 5, 2, SERIAL, -3, 3), (7, 300, 1, 0, -10, 90)):
        left, right = pair8(rng, rows, cols)
        exp = run8(ctx, left, right, rad, lo, hi, flags)
        same(exp, expected(left, right, rad, lo, hi, flags), "aligned call")
        lpitch = (cols + 2 * loff) | 1
        (_, lv), (_, rv) = view8(left, loff, pad=lpitch - cols), view8(right, roff, pad=lpitch + 2 * roff - cols)
        assert lv.data_ptr() % 4 == loff and rv.data_ptr() % 4 == roff and lv.stride(0) % 2 == 1 and rv.stride(0) % 2 == 1
        assert lv.stride(0) != rv.stride(0)
        dpitch = cols + 3
        disp = torch.full((rows, dpitch), SENTINEL_I8, dtype=torch.int8, device="cuda")
        _capi.check(_capi.lib.micv_disparity_ssd_u8_dev(ctx.handle, lv.data_ptr(), lv.stride(0), rv.data_ptr(), rv.stride(0),
                                                        rows, cols, rad, lo, hi, flags, disp.data_ptr(), dpitch, None))
        got = disp.cpu().numpy()
        same(np.ascontiguousarray(got[:, :cols]), exp, f"offsets {loff}, {roff} {rows}x{cols} r={rad}")
        assert (got[:, cols:] == SENTINEL_I8).all()


# ---- 3. ROLLING on bytes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rad", [1, 5, 7])
@pytest.mark.parametrize("flags", [ROLLING, ROLLING | COLS_2R | MIN_SSD_5E6])
def test_rolling_on_bytes_is_the_fresh_sums(ctx, rad, flags):
    rng = np.random.default_rng(rad * 100 + flags)
    rows, cols = 45, 129  # more than one of ROLLING's 40-row strips
    left, right = pair8(rng, rows, cols)
    right[:, cols // 2:] = 255 - right[:, cols // 2:]
    got = run8(ctx, left, right, rad, -100, 27, flags)
    same(got, ref.ssd_cuda(left, right, rad, -100, 27, flags & ~ROLLING), "the reference without ROLLING")
    same(got, f32_entry(ctx, left, right, rad, -100, 27, flags), "the f32 entry with ROLLING")


# ---- 4. forms that leave the exact path ------------------------------------------------------------------------------
LEAVE = [(0, 0), (8, 0), (10, COLS_2R | MIN_SSD_5E6), (12, 0), (6, SERIAL), (7, SERIAL), (1, COLS_2R), (9, ROLLING)]


@pytest.mark.parametrize("rad,flags", LEAVE, ids=[f"r{r}-f{f}" for r, f in LEAVE])
def test_forms_the_exact_sum_kernels_do_not_take(ctx, rad, flags):
    rng = np.random.default_rng(rad * 16 + flags)
    rows, cols = 17, 129
    left, right = pair8(rng, rows, cols)
    (_, lv), (_, rv) = view8(left, 1, pad=3), view8(right, 2, pad=6)
    from introtocomputervision_amd import stereo
    got = stereo.disparitySSD8(lv, rv, rad, -40, 30, flags, ctx=ctx).cpu().numpy()
    same(got, f32_entry(ctx, left, right, rad, -40, 30, flags), "the f32 entry")
    if flags & SERIAL:
        same(got, ref.ssd_serial(left, right, rad, -40, 30), "serial:: is integer sums at any radius")
    elif rad == 1:  # (from radius 8 on a window's sum can pass 2^24: the float contract is the only definition there)
        same(got, ref.ssd_cuda(left, right, rad, -40, 30, flags), "reference")


def test_float_only_context(ctx):
    """MICV_OPT_STEREO_EXACT = -1: the converted pair through the float kernels, a batch included."""
    from introtocomputervision_amd import stereo
    from introtocomputervision_amd._capi import Context, OPT_STEREO_EXACT
    flt = Context(0)
    try:
        flt.set_option(OPT_STEREO_EXACT, -1)
        rng = np.random.default_rng(41)
        pairs = [pair8(rng, 17, 129) for _ in range(2)]
        for rad, flags in ((5, 0), (7, COLS_2R | MIN_SSD_5E6), (3, SERIAL)):
            exps = [expected(l, r, rad, -40, 30, flags) for l, r in pairs]
            for (l, r), exp in zip(pairs, exps):
                same(run8(flt, l, r, rad, -40, 30, flags), exp, "single")
            got = stereo.disparitySSD8Batch(dev8(np.stack([p[0] for p in pairs])), dev8(np.stack([p[1] for p in pairs])),
                                            rad, -40, 30, flags, ctx=flt).cpu().numpy()
            for g, exp in zip(got, exps):
                same(g, exp, "batch element")
    finally:
        flt.close()


# ---- 5. the threshold matters ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rad,flags", [(6, MIN_SSD_5E6), (7, MIN_SSD_5E6), (6, COLS_2R | MIN_SSD_5E6), (7, COLS_2R | MIN_SSD_5E6)])
def test_threshold_splits_the_image(ctx, rad, flags):
    """min_disparity >= 0, so -1 can only be the 5e6 threshold: independent 0 / 255 noise on the left half (window costs
    around half the taps x 255^2 > 5e6), a shifted copy on the right half (cost 0)."""
    rng = np.random.default_rng(rad + flags)
    rows, cols = 17, 200
    left = (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)
    right = np.roll(left, 2, axis=1)
    right[:, :cols // 2] = (rng.integers(0, 2, (rows, cols // 2)) * 255).astype(np.uint8)
    exp = ref.ssd_cuda(left, right, rad, 0, 3, flags)
    assert (exp == -1).any() and (exp != -1).any()
    same(run8(ctx, left, right, rad, 0, 3, flags), exp, "threshold")


# ---- 6. extremes and ties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, COLS_2R, COLS_2R | MIN_SSD_5E6])
def test_extremes_and_ties(ctx, flags):
    rows, cols = 17, 200
    rng = np.random.default_rng(6)
    white = np.full((rows, cols), 255, np.uint8)
    base = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
    periodic = np.tile(base, (1, cols // 32 + 1))[:, :cols]
    cases = [("all 255", white, white), ("255 against 0", white, np.zeros_like(white)),
             ("constant", np.full((rows, cols), 77, np.uint8), np.full((rows, cols), 77, np.uint8)),
             ("period 32", periodic, np.roll(periodic, 5, axis=1))]
    for name, left, right in cases:
        for lo, hi in ((-128, 127), (-100, 27)):
            exp = expected(left, right, 7, lo, hi, flags)
            if name in ("all 255", "constant"):
                assert (exp == lo).all()  # equal costs in every chunk: the lowest disparity
            same(run8(ctx, left, right, 7, lo, hi, flags), exp, name)


# ---- 7. batch --------------------------------------------------------------------------------------------------------
def batch_case(ctx, batch, rows, cols, rad, lo, hi, flags, what):
    """Different random data in every pair, pair strides larger than the image with sentinel gaps in inputs and output:
    every element equals the single u8 call and the reference, the gaps are untouched."""
    from introtocomputervision_amd import _capi
    rng = np.random.default_rng(batch * 1000 + rows * 10 + rad)
    pairs = [pair8(rng, rows, cols) for _ in range(batch)]
    (_, lv), (_, rv) = view8(np.stack([p[0] for p in pairs]), 1, pad=3, tail=7), view8(np.stack([p[1] for p in pairs]), 3, pad=0, tail=1)
    dpitch, dpair = cols + 5, rows * (cols + 5) + 11
    disp = torch.full((batch * dpair,), SENTINEL_I8, dtype=torch.int8, device="cuda")
    _capi.check(_capi.lib.micv_disparity_ssd_u8_batch_dev(
        ctx.handle, lv.data_ptr(), lv.stride(0), lv.stride(1), rv.data_ptr(), rv.stride(0), rv.stride(1), batch, rows, cols,
        rad, lo, hi, flags, disp.data_ptr(), dpair, dpitch, None))
    got = disp.cpu().numpy()
    written = np.zeros(got.shape, bool)
    for i, (left, right) in enumerate(pairs):
        m = got[i * dpair:i * dpair + rows * dpitch].reshape(rows, dpitch)
        written[i * dpair:i * dpair + rows * dpitch].reshape(rows, dpitch)[:, :cols] = True
        g = np.ascontiguousarray(m[:, :cols])
        same(g, expected(left, right, rad, lo, hi, flags), f"{what}: element {i} against the reference")
        same(g, run8(ctx, left, right, rad, lo, hi, flags), f"{what}: element {i} against the single call")
    assert (got[~written] == SENTINEL_I8).all(), f"{what}: bytes outside the maps were written"


@pytest.mark.parametrize("batch", [1, 2, 3, 5])
def test_batch(ctx, batch):
    batch_case(ctx, batch, 9, 129, 5, -70, 10, COLS_2R | MIN_SSD_5E6, "9 rows")
    batch_case(ctx, batch, 17, 70, 7, -128, 127, 0, "17 rows")
    batch_case(ctx, batch, 9, 65, 3, -20, 20, SERIAL, "serial")


def test_batch_in_pieces():
    """A bound of 1 MiB on the packed planes: five pairs of 17 x 1000 (about 0.3 MiB of planes each) go three and two.
    The context's arena shows that no launch held all five."""
    from introtocomputervision_amd._capi import Context, OPT_STEREO_BATCH_MB
    small = Context(0)
    try:
        small.set_option(OPT_STEREO_BATCH_MB, 1)
        batch_case(small, 5, 17, 1000, 7, -20, 20, COLS_2R | MIN_SSD_5E6, "pieces")
        assert 0 < small.scratch_bytes() <= 1 << 20
    finally:
        small.close()


def test_last_piece_is_laid_out_as_the_full_ones():
    """1040 pairs of 17 x 20 under a bound of 4 MiB: two full pieces of some 470 pairs (1400 strips: 16 columns per wave fill
    the device in one round) and a last one of about 100, which on its own would be tiled with 8 columns per wave and
    another plan width.  Every piece must fit the one reservation made for the full piece -- the library refuses a launch
    whose planes would not -- and the arena must stay within the bound; every element is compared as in test_batch."""
    from introtocomputervision_amd._capi import Context, OPT_STEREO_BATCH_MB
    small = Context(0)
    try:
        small.set_option(OPT_STEREO_BATCH_MB, 4)
        batch_case(small, 1040, 17, 20, 2, -3, 3, MIN_SSD_5E6, "last piece")
        assert 0 < small.scratch_bytes() <= 4 << 20
    finally:
        small.close()


# ---- 8. concurrency without the flag word ----------------------------------------------------------------------------
def test_f32_calls_of_another_stream_do_not_reach_a_u8_call():
    """One context, two streams: f32 calls on a pair that is NOT 8-bit-valued (their pre-pass stores the call's epoch in the
    context's flag word) issued around a u8 call.  The u8 search reads a word nobody writes, so it cannot take the other
    call's verdict for its own.

    This is NOT a test of overlapping calls, and they are not safe: two streams of one context still share its scratch arena
    (mi_cv.h: one context per stream), u8 and f32 calls alike, so the events below keep the calls from overlapping on the
    device.  What the test shows is only that a flag word left at an f32 call's epoch does not reach the u8 search."""
    from introtocomputervision_amd import stereo
    from introtocomputervision_amd._capi import Context
    c = Context(0)
    try:
        rng = np.random.default_rng(8)
        left, right = pair8(rng, 17, 200)
        exp = ref.ssd_cuda(left, right, 5, -70, 0, 0)
        fl = torch.from_numpy(left.astype(np.float32) + 0.5).cuda()
        fr = torch.from_numpy(right.astype(np.float32)).cuda()
        dl, dr = dev8(left), dev8(right)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        got, other = [], []
        for _ in range(3):
            with torch.cuda.stream(sb):
                other.append(stereo.disparitySSD(fl, fr, 5, -70, 0, 0, ctx=c))
            sa.wait_stream(sb)
            with torch.cuda.stream(sa):
                got.append(stereo.disparitySSD8(dl, dr, 5, -70, 0, 0, ctx=c))
            sb.wait_stream(sa)
        torch.cuda.synchronize()
        for g in got:
            same(g.cpu().numpy(), exp, "u8 call between f32 calls")
        for o in other[1:]:
            assert torch.equal(o, other[0])
    finally:
        c.close()


# ---- 9. at the reference's size --------------------------------------------------------------------------------------
def test_reference_size_batch_of_three(ctx):
    """511 x 640, radius 7, [-95, 0], the as-written CUDA flags, three pairs: element 0 against the integer reference, all
    three against the f32 entry on the converted pairs; once more with the batch cut into single pairs."""
    from introtocomputervision_amd import stereo
    from introtocomputervision_amd._capi import Context, OPT_STEREO_BATCH_MB
    rows, cols, flags = 511, 640, COLS_2R | MIN_SSD_5E6
    rng = np.random.default_rng(511)
    pairs = [pair8(rng, rows, cols, shift=-11 * (i + 1)) for i in range(3)]
    pairs[1][1][:, :200] = 255 - pairs[1][1][:, :200]  # a region over the threshold
    dl, dr = dev8(np.stack([p[0] for p in pairs])), dev8(np.stack([p[1] for p in pairs]))
    got = stereo.disparitySSD8Batch(dl, dr, 7, -95, 0, flags, ctx=ctx).cpu().numpy()
    same(got[0], ref.ssd_cuda(pairs[0][0], pairs[0][1], 7, -95, 0, flags), "element 0 against the reference")
    for i, (left, right) in enumerate(pairs):
        same(got[i], f32_entry(ctx, left, right, 7, -95, 0, flags), f"element {i} against the f32 entry")
    assert (got[1] == -1).any()
    small = Context(0)
    try:
        small.set_option(OPT_STEREO_BATCH_MB, 1)
        again = stereo.disparitySSD8Batch(dl, dr, 7, -95, 0, flags, ctx=small).cpu().numpy()
    finally:
        small.close()
    assert np.array_equal(again, got)


# ---- 10. _host -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rad,flags", [(5, COLS_2R | MIN_SSD_5E6), (7, 0), (3, SERIAL), (9, 0)])
def test_host_entry(ctx, rad, flags):
    from introtocomputervision_amd import _capi, stereo
    rng = np.random.default_rng(rad)
    rows, cols = 17, 129
    left, right = pair8(rng, rows, cols)
    exp = run8(ctx, left, right, rad, -40, 30, flags)
    (_, lv), (_, rv) = strided_host(left, 3), strided_host(right, 10)
    for _ in range(2):  # the second call of a shape finds its device blocks in the context's cache
        same(stereo.disparitySSD8(lv, rv, rad, -40, 30, flags, ctx=ctx), exp, "host arrays")
    dblock, dv = strided_host(np.zeros((rows, cols), np.int8), 6)
    dv[...] = SENTINEL_I8
    _capi.check(_capi.lib.micv_disparity_ssd_u8_host(ctx.handle, lv.ctypes.data, lv.strides[0], rv.ctypes.data, rv.strides[0],
                                                     rows, cols, rad, -40, 30, flags, dv.ctypes.data, dv.strides[0]))
    same(np.ascontiguousarray(dv), exp, "pitched output")
    assert (dblock[:, cols:] == SENTINEL).all()


# ---- 11. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from introtocomputervision_amd import _capi
    lib = _capi.lib
    rows, cols = 9, 40
    rng = np.random.default_rng(11)
    left, right = pair8(rng, rows, cols)
    dl, dr = dev8(left), dev8(right)
    disp = torch.full((2, rows, cols), 77, dtype=torch.int8, device="cuda")
    hdisp = np.full((rows, cols), 77, np.int8)
    L, R, D = dl.data_ptr(), dr.data_ptr(), disp.data_ptr()

    def calls(l=L, r=R, ls=cols, rs=cols, rad=3, lo=-10, hi=0, flags=0, d=D, ds=cols):
        host = {L: left.ctypes.data, R: right.ctypes.data, D: hdisp.ctypes.data}
        yield lib.micv_disparity_ssd_u8_dev(ctx.handle, l, ls, r, rs, rows, cols, rad, lo, hi, flags, d, ds, None)
        yield lib.micv_disparity_ssd_u8_batch_dev(ctx.handle, l, rows * cols, ls, r, rows * cols, rs, 1, rows, cols, rad, lo, hi,
                                                  flags, d, rows * cols, ds, None)
        yield lib.micv_disparity_ssd_u8_host(ctx.handle, host.get(l, l), ls, host.get(r, r), rs, rows, cols, rad, lo, hi, flags,
                                             host.get(d, d), ds)

    cases = [(dict(l=None), "null"), (dict(r=None), "null"), (dict(d=None), "null"), (dict(ls=cols - 1), "stride"),
             (dict(rs=cols - 1), "stride"), (dict(ds=cols - 1), "stride"), (dict(flags=SERIAL | COLS_2R), "serial::disparitySSD"),
             (dict(flags=SERIAL | ROLLING), "SERIAL and ROLLING"), (dict(lo=-129), "int8"), (dict(hi=128), "int8"),
             (dict(lo=1, hi=0), "int8"), (dict(rad=32), "radius"), (dict(flags=16), "flags")]
    for kw, word in cases:
        for rc in calls(**kw):
            msg = _capi.last_error()
            assert rc == _capi.EINVAL and word in msg, (kw, rc, msg)
    # a batch whose disparity maps overlap
    rc = lib.micv_disparity_ssd_u8_batch_dev(ctx.handle, L, 0, cols, R, 0, cols, 2, rows, cols, 3, -10, 0, 0, D, rows * cols - 1,
                                             cols, None)
    assert rc == _capi.EINVAL and "overlap" in _capi.last_error()
    torch.cuda.synchronize()
    assert (disp.cpu().numpy() == 77).all() and (hdisp == 77).all()
    # the same arguments without the fault
    for rc in calls():
        assert rc == _capi.OK, _capi.last_error()
    torch.cuda.synchronize()
    exp = ref.ssd_cuda(left, right, 3, -10, 0, 0)
    same(disp[0].cpu().numpy(), exp, "after the refusals")
    same(hdisp, exp, "after the refusals, host")
