"""Every path of the ps7 motion-history kernels (mhi.hip: the fused blur / subtract / threshold ballot kernel, the
bit-plane 7 x 7 open, threshold, update, energy, and mhiHelper's loop) byte for byte against tests/_mhi_ref.py, which
shares no code with the kernels or the oracle.  The shapes (tests/_mhi_cases.py) sit at the kernels' own edges: the
16-row blur tile, the 52-row wave and 208-row workgroup of the open with their 6-row aprons, the 64-column word with
its 6-column aprons and the fast-path edge of the second word, and images smaller than the structuring element and
than the blur's half-width.  No tolerance anywhere.

Which case shows which mistake (tests/test_mhi_ref.py proves each on the CPU): a `>` for the `>=` of the ballot
kernel, a reversed, absolute or wrapped subtract and a missing dilation fail test_frame_difference[53x70] at
53x70-step-b1x1-t1, a threshold cast to int at 53x70-step-b1x1-t1.7, `-val` as a byte at 53x70-step-b1x1-t255, swapped
blur sizes at 53x70-noise-b5x1-t40, a rectangle or a wider ellipse row (a half-width changed in morph_rows), a close
for the open at 53x70-noise-b3x3-t1.7, a zero-padded erosion at test_frame_difference[6x7] (6x7-step-b1x1-t0), half-away
rounding and an unfused blur at test_planted_rounding_rows, `mask != 0`, a saturated tau and a missing floor at
test_update."""
import numpy as np
import pytest

import _mhi_cases as C
import _mhi_ref as M

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _mhi():
    from introtocomputervision_amd import mhi
    return mhi


def _lib():
    from introtocomputervision_amd import _capi
    return _capi.lib, _capi.check


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ctx():
    from introtocomputervision_amd import _capi
    c = _capi.Context(0)
    yield c
    c.close()


def dev_block(nbytes):
    import torch
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


def dev_view(block, off, stride, a):
    """Copies a into the block as a [rows, cols] view that starts `off` bytes in with `stride` bytes per row."""
    import torch
    v = torch.as_strided(block, a.shape, (stride, 1), off)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def outside_intact(block, off, stride, rows, cols):
    """Every byte of the block that is not in the [rows, cols] view still holds the sentinel."""
    b = np.array(host(block))
    for y in range(rows):
        b[off + y * stride: off + y * stride + cols] = SENTINEL
    return bool((b == SENTINEL).all())


def strided_host(a, pad, lead=0):
    """The helper of tests/test_warp_gpu.py with a leading offset: a sentinel block and a [rows, cols] view into it."""
    block = np.full(lead + a.shape[0] * (a.shape[1] + pad), SENTINEL, np.uint8)
    view = np.lib.stride_tricks.as_strided(block[lead:], a.shape, (a.shape[1] + pad, 1))
    view[...] = a
    return block, view


def host_outside_intact(block, view):
    b = block.copy()
    np.lib.stride_tricks.as_strided(b[view.ctypes.data - block.ctypes.data:], view.shape, view.strides)[...] = SENTINEL
    return bool((b == SENTINEL).all())


# ------------------------------------------------------------------------------------------- frameDifference

@pytest.mark.parametrize("rows,cols", C.SHAPES, ids=[f"{r}x{c}" for r, c in C.SHAPES])
def test_frame_difference(rows, cols):
    mhi = _mhi()
    bad = []
    for c in C.cases_of(rows, cols):
        f1, f2 = C.frames(c)
        want = C.expected(c)
        got = host(mhi.frameDifference(dev(f1), dev(f2), c.thresh, c.ksize, c.sigma))
        if not np.array_equal(got, want):
            bad.append((c.name, "dev", int((got != want).sum())))
        got = mhi.frameDifference(np.array(f1), np.array(f2), c.thresh, c.ksize, c.sigma)
        if not np.array_equal(got, want):
            bad.append((c.name, "host", int((got != want).sum())))
    assert not bad, bad


def test_planted_rounding_rows():
    """One-row images in which one pixel's blur is an exact .5 tie, or lies within a float ulp of one (so that an
    unfused chain rounds the other way), and that pixel decides a mask bit the open keeps."""
    mhi = _mhi()
    for tup, x in M.TIE_TUPLES + M.FMA_TUPLES:
        f1, f2, thr = M.tie_pair(tup, x)
        want = M.frame_difference(f1, f2, thr, M.TIE_BLUR, M.TIE_SIGMA)
        assert np.array_equal(host(mhi.frameDifference(dev(f1), dev(f2), thr, M.TIE_BLUR, M.TIE_SIGMA)), want), tup
        assert np.array_equal(mhi.frameDifference(f1, f2, thr, M.TIE_BLUR, M.TIE_SIGMA), want), tup


PITCH_CASES = ("53x70-noise-b3x3-t1.7", "57x71-step-b1x1-t1", "58x128-noise-b31x31-t1.7", "6x7-step-b1x1-t0")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_pitched_and_unaligned_destination(ctx, off):
    """micv_mhi_frame_difference_dev with `diff` 0 .. 3 bytes into a sentinel block and dstride > cols: an odd pitch
    (the alignment changes from row to row, so one image takes the dword store and the byte store) and a pitch that is
    a multiple of 4 (every row as aligned as the first); then the same with pitched, unaligned sources."""
    import torch
    lib, check = _lib()
    for name in PITCH_CASES:
        c = C.case(name)
        f1, f2 = C.frames(c)
        want = C.expected(c)
        d1, d2 = dev(f1), dev(f2)
        for dstride in (c.cols + 7 + (c.cols % 2), (c.cols + 8) // 4 * 4):  # odd; a multiple of 4
            assert dstride > c.cols
            block = dev_block(off + c.rows * dstride + 16)
            check(lib.micv_mhi_frame_difference_dev(ctx.handle, d1.data_ptr(), d2.data_ptr(), c.rows, c.cols, c.cols,
                                                    float(c.thresh), c.ksize[0], c.ksize[1], c.sigma,
                                                    block.data_ptr() + off, dstride, _stream()))
            got = host(torch.as_strided(block, (c.rows, c.cols), (dstride, 1), off))
            assert np.array_equal(got, want), (name, dstride, int((got != want).sum()))
            assert outside_intact(block, off, dstride, c.rows, c.cols), (name, dstride)
        # pitched sources that start off + 1 bytes into their blocks
        stride = c.cols + 9
        b1, b2 = dev_block(off + 1 + c.rows * stride), dev_block(off + 1 + c.rows * stride)
        v1, v2 = dev_view(b1, off + 1, stride, f1), dev_view(b2, off + 1, stride, f2)
        out = dev_block(c.rows * c.cols)
        check(lib.micv_mhi_frame_difference_dev(ctx.handle, v1.data_ptr(), v2.data_ptr(), c.rows, c.cols, stride,
                                                float(c.thresh), c.ksize[0], c.ksize[1], c.sigma, out.data_ptr(),
                                                c.cols, _stream()))
        assert np.array_equal(host(out).reshape(c.rows, c.cols), want), name
        assert outside_intact(b1, off + 1, stride, c.rows, c.cols) and outside_intact(b2, off + 1, stride, c.rows, c.cols)
        # the Python flavour on views of a larger tensor
        assert np.array_equal(host(_mhi().frameDifference(v1, v2, c.thresh, c.ksize, c.sigma)), want), name


# ------------------------------------------------------------------------------------------- threshold, energy, update

def test_threshold_and_energy_on_every_byte_value(ctx):
    mhi = _mhi()
    import torch
    v = np.arange(768).astype(np.uint8).reshape(6, 128)
    block = dev_block(3 + 6 * 141)
    pv = dev_view(block, 3, 141, v)
    for t in C.THRESHOLDS:
        want = M.threshold(v, t)
        assert np.array_equal(host(mhi.thresholdDifference(dev(v), t)), want), t
        assert np.array_equal(host(mhi.thresholdDifference(pv, t)), want), t
        assert np.array_equal(mhi.thresholdDifference(v, t), want), t
    want = M.energy(v)
    assert want.sum() == 765
    assert np.array_equal(host(mhi.energyFromHistory(dev(v))), want)
    assert np.array_equal(host(mhi.energyFromHistory(pv)), want)
    assert np.array_equal(mhi.energyFromHistory(v), want)
    assert all(np.array_equal(e, want) for e in mhi.energyFromHistory([v, v]))
    assert outside_intact(block, 3, 141, 6, 128)
    # pitched destinations through the C entry points
    lib, check = _lib()
    for fn, extra, exp in ((lib.micv_mhi_threshold_dev, (1.7,), M.threshold(v, 1.7)), (lib.micv_mhi_energy_dev, (), want)):
        out = dev_block(1 + 6 * 131)
        check(fn(ctx.handle, pv.data_ptr(), 6, 128, 141, *extra, out.data_ptr() + 1, 131, _stream()))
        assert np.array_equal(host(torch.as_strided(out, (6, 128), (131, 1), 1)), exp)
        assert outside_intact(out, 1, 131, 6, 128)


@pytest.mark.parametrize("tau", C.TAUS)
def test_update(tau):
    mhi = _mhi()
    hist, mask = C.update_inputs()
    rows, cols = hist.shape
    want = M.update(hist, mask, tau)
    h = dev(hist)
    assert mhi.calcMotionHistory(h, dev(mask), tau) is h
    assert np.array_equal(host(h), want)
    hb, mb = dev_block(2 + rows * (cols + 5)), dev_block(1 + rows * (cols + 11))
    hv, mv = dev_view(hb, 2, cols + 5, hist), dev_view(mb, 1, cols + 11, mask)
    mhi.calcMotionHistory(hv, mv, tau)
    assert np.array_equal(host(hv), want)
    assert outside_intact(hb, 2, cols + 5, rows, cols) and np.array_equal(host(mv), mask)
    hh = np.array(hist)
    mhi.calcMotionHistory(hh, np.array(mask), tau)
    assert np.array_equal(hh, want)
    # decays to the floor and stays there
    z = np.zeros_like(mask)
    for _ in range(3):
        want = M.update(want, z, tau)
        mhi.calcMotionHistory(h, dev(z), tau)
    assert np.array_equal(host(h), want) and (want == 0).any()


# ------------------------------------------------------------------------------------------- historySequence

def test_history_sequence():
    """More frames than tau, `save` unordered with a repeat; dense frames, and frames sliced in rows and columns out
    of a larger tensor / array, so that the frame pitch and the row stride both exceed the dense ones."""
    import torch
    mhi = _mhi()
    h = C.HISTORY
    frames, want = C.history_frames(), C.history_expected()
    args = (h["thresh"], h["ksize"], h["sigma"], h["tau"], list(h["save"]))
    assert np.array_equal(host(mhi.historySequence(dev(frames), *args)), want)
    F, rows, cols = frames.shape
    big = torch.full((F, rows + 5, cols + 9), SENTINEL, dtype=torch.uint8, device="cuda")
    view = big[:, 2:2 + rows, 4:4 + cols]
    view.copy_(dev(frames))
    assert view.stride(0) > rows * view.stride(1) > rows * cols
    assert np.array_equal(host(mhi.historySequence(view, *args)), want)
    assert np.array_equal(mhi.historySequence(np.array(frames), *args), want)
    hbig = np.full((F, rows + 3, cols + 6), SENTINEL, np.uint8)
    hview = hbig[:, 1:1 + rows, 5:5 + cols]
    hview[...] = frames
    assert np.array_equal(mhi.historySequence(hview, *args), want)
    # tau above 255 is stored as a byte here too
    want300 = M.history_seq(frames, h["thresh"], h["ksize"], h["sigma"], 300, [3, 8])
    assert want300.max() == 44
    assert np.array_equal(host(mhi.historySequence(dev(frames), h["thresh"], h["ksize"], h["sigma"], 300, [3, 8])), want300)


# ------------------------------------------------------------------------------------------- host entries, strided

def test_host_entries_with_strided_buffers(ctx):
    lib, check = _lib()
    c = C.case("53x70-noise-b3x3-t1.7")
    f1, f2 = C.frames(c)
    rows, cols = c.rows, c.cols
    (_, s1), (_, s2) = strided_host(f1, 13, 3), strided_host(f2, 13, 3)
    dblock, dv = strided_host(np.zeros_like(f1), 5, 1)
    dblock[...] = SENTINEL
    check(lib.micv_mhi_frame_difference_host(ctx.handle, s1.ctypes.data, s2.ctypes.data, rows, cols, s1.strides[0],
                                             float(c.thresh), c.ksize[0], c.ksize[1], c.sigma, dv.ctypes.data,
                                             dv.strides[0]))
    assert np.array_equal(dv, C.expected(c)) and host_outside_intact(dblock, dv)
    for fn, extra, want in ((lib.micv_mhi_threshold_host, (40.0,), M.threshold(f1, 40)),
                            (lib.micv_mhi_energy_host, (), M.energy(C.step_pair(rows, cols)[0]))):
        src = f1 if extra else C.step_pair(rows, cols)[0]  # (the step pair's first frame holds zeros)
        _, sv = strided_host(src, 7, 2)
        dblock, dv = strided_host(np.zeros_like(f1), 3, 0)
        dblock[...] = SENTINEL
        check(fn(ctx.handle, sv.ctypes.data, rows, cols, sv.strides[0], *extra, dv.ctypes.data, dv.strides[0]))
        assert np.array_equal(dv, want) and host_outside_intact(dblock, dv)
    hist, mask = C.update_inputs()
    hblock, hv = strided_host(hist, 9, 1)
    mblock, mv = strided_host(mask, 2, 3)
    check(lib.micv_mhi_update_host(ctx.handle, hv.ctypes.data, hv.strides[0], mv.ctypes.data, mv.strides[0],
                                   hist.shape[0], hist.shape[1], 300))
    assert np.array_equal(hv, M.update(hist, mask, 300)) and host_outside_intact(hblock, hv)
    assert np.array_equal(mv, mask) and host_outside_intact(mblock, mv)
    # micv_mhi_history_seq_host: frame pitch, row stride, output pitch and output row stride all above the dense ones
    h = C.HISTORY
    frames, want = C.history_frames(), C.history_expected()
    F, rows, cols = frames.shape
    fbig = np.full((F, rows + 2, cols + 11), SENTINEL, np.uint8)
    fv = fbig[:, 1:1 + rows, 6:6 + cols]
    fv[...] = frames
    save = np.array(h["save"], np.int32)
    obig = np.full((save.size, rows + 1, cols + 3), SENTINEL, np.uint8)
    ov = obig[:, :rows, 2:2 + cols]
    check(lib.micv_mhi_history_seq_host(ctx.handle, fv.ctypes.data, F, fv.strides[0], fv.strides[1], rows, cols,
                                        float(h["thresh"]), h["ksize"][0], h["ksize"][1], h["sigma"], h["tau"],
                                        save.ctypes.data, save.size, ov.ctypes.data, ov.strides[0], ov.strides[1]))
    assert np.array_equal(ov, want)
    ov[...] = SENTINEL
    assert (obig == SENTINEL).all()


# ------------------------------------------------------------------------------------------- one context, many shapes

def test_one_context_changing_shapes():
    """Small, large, small again, then historySequence (its planes sit behind frameDifference's words in the arena),
    then frameDifference: the scratch is carved anew per call and the arena grows, and no result changes."""
    from introtocomputervision_amd import _capi
    mhi = _mhi()
    ctx = _capi.Context(0)
    try:
        small, large = C.case("6x7-noise-b5x1-t2"), C.case("213x200-noise-b31x31-t1.7")
        mid = C.case("53x70-noise-b3x3-t1.7")
        h = C.HISTORY
        grew = []

        def run(c):
            f1, f2 = C.frames(c)
            got = host(mhi.frameDifference(dev(f1), dev(f2), c.thresh, c.ksize, c.sigma, ctx=ctx))
            assert np.array_equal(got, C.expected(c)), c.name
            grew.append(ctx.scratch_bytes())

        run(small); run(large); run(small); run(mid)
        got = mhi.historySequence(dev(C.history_frames()), h["thresh"], h["ksize"], h["sigma"], h["tau"],
                                  list(h["save"]), ctx=ctx)
        assert np.array_equal(host(got), C.history_expected())
        grew.append(ctx.scratch_bytes())
        run(large); run(small)
        got = mhi.historySequence(dev(C.history_frames()), h["thresh"], h["ksize"], h["sigma"], h["tau"],
                                  list(h["save"]), ctx=ctx)
        assert np.array_equal(host(got), C.history_expected())
        assert grew == sorted(grew) and grew[1] >= 213 * 4 * 8
    finally:
        ctx.close()
