"""mhi::frameDifference on colour frames (mhi.hip: mhi_blur_diff_bits_c_kernel in front of the bit-plane open), the
sequence with both save lists and the batch of videos, byte for byte against tests/_mhi_color_ref.py.  The shapes sit
at the 16-row / 64-column blur tile, the word and its aprons, the open's wave and workgroup, and below the structuring
element's size; channels are 3 and 4; no tolerance anywhere.

Which case shows which mistake is proved on the CPU by tests/test_mhi_color_ref.py (SHOWN_BY): all of them are cases of
test_frame_difference[53x70x3] or [53x70x4]."""
import ctypes

import numpy as np
import pytest

import _mhi_cases as C1
import _mhi_color_cases as C
import _mhi_color_ref as R
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
    """Copies a ([rows, cols] or [rows, cols, C]) into the block, `off` bytes in, `stride` bytes per row."""
    import torch
    strides = (stride, 1) if a.ndim == 2 else (stride, a.shape[2], 1)
    v = torch.as_strided(block, a.shape, strides, off)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def outside_intact(block, off, stride, rows, row_bytes):
    b = np.array(host(block))
    for y in range(rows):
        b[off + y * stride: off + y * stride + row_bytes] = SENTINEL
    return bool((b == SENTINEL).all())


def c_dev(ctx, f1, f2, rows, cols, ch, stride, c, out_ptr, dstride):
    lib, check = _lib()
    check(lib.micv_mhi_frame_difference_c_dev(ctx.handle, f1, f2, rows, cols, ch, stride, float(c.thresh), c.ksize[0],
                                              c.ksize[1], c.sigma, out_ptr, dstride, _stream()))


# ------------------------------------------------------------------------------------------- frameDifference

IDS = [(r, c, ch) for r, c in C.SHAPES for ch in C.CHANNELS]


@pytest.mark.parametrize("rows,cols,ch", IDS, ids=[f"{r}x{c}x{ch}" for r, c, ch in IDS])
def test_frame_difference(rows, cols, ch):
    mhi = _mhi()
    bad = []
    cs = C.cases_of(rows, cols, ch)
    assert cs
    for c in cs:
        f1, f2 = C.frames(c)
        want = C.expected(c)
        got = host(mhi.frameDifference(dev(f1), dev(f2), c.thresh, c.ksize, c.sigma))
        if not np.array_equal(got, want):
            bad.append((c.name, "dev", int((got != want).sum())))
        got = mhi.frameDifference(np.array(f1), np.array(f2), c.thresh, c.ksize, c.sigma)
        if not np.array_equal(got, want):
            bad.append((c.name, "host", int((got != want).sum())))
    assert not bad, bad


def test_one_channel_gives_the_old_entry_points_bytes(ctx):
    lib, check = _lib()
    for name in ("53x70-noise-b3x3-t1.7", "57x71-step-b1x1-t1", "58x128-noise-b31x31-t1.7", "6x7-step-b1x1-t0",
                 "209x64-moving-b7x3-t10"):
        c = C1.case(name)
        f1, f2 = C1.frames(c)
        d1, d2 = dev(f1), dev(f2)
        old, new = dev_block(c.rows * c.cols), dev_block(c.rows * c.cols)
        check(lib.micv_mhi_frame_difference_dev(ctx.handle, d1.data_ptr(), d2.data_ptr(), c.rows, c.cols, c.cols,
                                                float(c.thresh), c.ksize[0], c.ksize[1], c.sigma, old.data_ptr(), c.cols,
                                                _stream()))
        c_dev(ctx, d1.data_ptr(), d2.data_ptr(), c.rows, c.cols, 1, c.cols, c, new.data_ptr(), c.cols)
        assert np.array_equal(host(new), host(old)), name
        assert np.array_equal(host(new).reshape(c.rows, c.cols), C1.expected(c)), name
        # [rows, cols, 1] through Python
        got = _mhi().frameDifference(d1[..., None], d2[..., None], c.thresh, c.ksize, c.sigma)
        assert np.array_equal(host(got), C1.expected(c)), name


def test_four_channels_equal_three_on_the_first_three_planes():
    mhi = _mhi()
    for c in C.cases():
        if c.channels != 4 or (c.rows, c.cols) not in ((6, 7), (53, 70), (105, 133)):
            continue
        f1, f2 = C.frames(c)
        want = C.expected(c)
        got3 = host(mhi.frameDifference(dev(f1[..., :3]), dev(f2[..., :3]), c.thresh, c.ksize, c.sigma))
        assert np.array_equal(got3, want), c.name
        # another alpha, same mask
        g1, g2 = np.array(f1), np.array(f2)
        g1[..., 3], g2[..., 3] = 255 - g1[..., 3], 0
        assert np.array_equal(host(mhi.frameDifference(dev(g1), dev(g2), c.thresh, c.ksize, c.sigma)), want), c.name


PITCH_CASES = ("53x70x3-noise-b3x3-t1.7", "53x70x4-step-b1x1-t1", "17x64x3-noise-b31x31-t1.7", "6x7x4-step-b1x1-t0",
               "53x70x3-moving-b7x3-t40")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_pitched_and_unaligned_sources_and_destination(ctx, off):
    """Sources `off` and `off + 1` bytes into sentinel blocks with padded rows (an odd pad: the alignment changes from
    row to row), the destination `off` bytes in with an odd pitch and with a multiple of 4."""
    import torch
    for name in PITCH_CASES:
        c = C.case(name)
        f1, f2 = C.frames(c)
        want = C.expected(c)
        rb = c.cols * c.channels
        stride = rb + 9
        b1, b2 = dev_block(off + c.rows * stride + 8), dev_block(off + 1 + c.rows * stride + 8)
        v1, v2 = dev_view(b1, off, stride, f1), dev_view(b2, off + 1, stride, f2)
        # frameDifference takes one stride for both frames; the second view's base differs, its stride does not
        for dstride in (c.cols + 7 + (c.cols % 2), (c.cols + 8) // 4 * 4):
            block = dev_block(off + c.rows * dstride + 16)
            c_dev(ctx, v1.data_ptr(), v2.data_ptr(), c.rows, c.cols, c.channels, stride, c, block.data_ptr() + off, dstride)
            got = host(torch.as_strided(block, (c.rows, c.cols), (dstride, 1), off))
            assert np.array_equal(got, want), (name, dstride, int((got != want).sum()))
            assert outside_intact(block, off, dstride, c.rows, c.cols), (name, dstride)
        assert outside_intact(b1, off, stride, c.rows, rb) and outside_intact(b2, off + 1, stride, c.rows, rb)
        assert np.array_equal(host(v1), f1) and np.array_equal(host(v2), f2)
        # the Python flavour on views of a larger tensor
        assert np.array_equal(host(_mhi().frameDifference(v1, v2, c.thresh, c.ksize, c.sigma)), want), name


def test_host_entry_with_strided_arrays(ctx):
    lib, check = _lib()
    for name in ("53x70x3-noise-b3x3-t1.7", "53x70x4-noise-b7x3-t2", "15x58x4-step-b1x1-t1"):
        c = C.case(name)
        f1, f2 = C.frames(c)
        rows, cols, ch = f1.shape
        stride = cols * ch + 13
        srcs = []
        for f, lead in ((f1, 3), (f2, 1)):
            block = np.full(lead + rows * stride, SENTINEL, np.uint8)
            view = np.lib.stride_tricks.as_strided(block[lead:], f.shape, (stride, ch, 1))
            view[...] = f
            srcs.append((block, view))
        dblock = np.full(2 + rows * (cols + 5), SENTINEL, np.uint8)
        dv = np.lib.stride_tricks.as_strided(dblock[2:], (rows, cols), (cols + 5, 1))
        check(lib.micv_mhi_frame_difference_c_host(ctx.handle, srcs[0][1].ctypes.data, srcs[1][1].ctypes.data, rows, cols, ch,
                                                   stride, float(c.thresh), c.ksize[0], c.ksize[1], c.sigma, dv.ctypes.data,
                                                   cols + 5))
        assert np.array_equal(dv, C.expected(c)), name
        keep = dblock.copy()
        np.lib.stride_tricks.as_strided(keep[2:], (rows, cols), (cols + 5, 1))[...] = SENTINEL
        assert (keep == SENTINEL).all(), name


def test_one_context_changing_shapes_and_channels():
    from introtocomputervision_amd import _capi
    mhi = _mhi()
    ctx = _capi.Context(0)
    try:
        grew = []
        order = ("6x7x3-noise-b3x3-t1.7", "209x64x4-noise-b31x31-t1.7", "6x7x4-step-b1x1-t1", "105x133x3-noise-b7x3-t2",
                 "53x70x4-noise-b1x1-t2", "2x2x3-noise-b31x31-t2", "105x133x4-noise-b31x31-t2", "1x1x3-step-b1x1-t0")
        for name in order:
            c = C.case(name)
            f1, f2 = C.frames(c)
            assert np.array_equal(host(mhi.frameDifference(dev(f1), dev(f2), c.thresh, c.ksize, c.sigma, ctx=ctx)),
                                  C.expected(c)), name
            grew.append(ctx.scratch_bytes())
            if name.startswith("105x133x3"):  # a single-channel call and a sequence in between
                c1 = C1.case("53x70-noise-b3x3-t1.7")
                g1, g2 = C1.frames(c1)
                assert np.array_equal(host(mhi.frameDifference(dev(g1), dev(g2), c1.thresh, c1.ksize, c1.sigma, ctx=ctx)),
                                      C1.expected(c1))
                h = C.HISTORY
                got, gd = mhi.historySequence(dev(C.history_frames()), h["thresh"], h["ksize"], h["sigma"], h["tau"],
                                              list(h["save"]), ctx=ctx, saveDiffFrames=list(h["save_diff"]))
                assert np.array_equal(host(got), C.history_expected()[0]) and np.array_equal(host(gd), C.history_expected()[1])
        assert grew == sorted(grew)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------- the sequence

def test_sequence_with_both_save_lists():
    """9 x 53 x 70 x 3, unordered and repeated save numbers of both kinds: against the reference and against the loop of
    single calls; dense frames, frames cut out of a larger tensor, host arrays; each list alone."""
    import torch
    mhi = _mhi()
    h = C.HISTORY
    frames = C.history_frames()
    want_h, want_d = C.history_expected()
    args = (h["thresh"], h["ksize"], h["sigma"], h["tau"])
    got_h, got_d = mhi.historySequence(dev(frames), *args, list(h["save"]), saveDiffFrames=list(h["save_diff"]))
    assert np.array_equal(host(got_h), want_h) and np.array_equal(host(got_d), want_d)
    # the loop of single calls
    d = dev(frames)
    hist = torch.zeros((53, 70), dtype=torch.uint8, device="cuda")
    for j in range(1, 9):
        m = mhi.frameDifference(d[j - 1], d[j], h["thresh"], h["ksize"], h["sigma"])
        mhi.calcMotionHistory(hist, m, h["tau"])
        for i, s in enumerate(h["save"]):
            if s == j:
                assert torch.equal(got_h[i], hist), j
        for i, s in enumerate(h["save_diff"]):
            if s == j:
                assert torch.equal(got_d[i], m), j
    # a view with a larger frame pitch and row stride
    F, rows, cols, ch = frames.shape
    big = torch.full((F, rows + 5, cols + 9, ch), SENTINEL, dtype=torch.uint8, device="cuda")
    view = big[:, 2:2 + rows, 4:4 + cols]
    view.copy_(d)
    got_h, got_d = mhi.historySequence(view, *args, list(h["save"]), saveDiffFrames=list(h["save_diff"]))
    assert np.array_equal(host(got_h), want_h) and np.array_equal(host(got_d), want_d)
    # host arrays, strided
    hbig = np.full((F, rows + 3, cols + 6, ch), SENTINEL, np.uint8)
    hview = hbig[:, 1:1 + rows, 5:5 + cols]
    hview[...] = frames
    got_h, got_d = mhi.historySequence(hview, *args, list(h["save"]), saveDiffFrames=list(h["save_diff"]))
    assert np.array_equal(got_h, want_h) and np.array_equal(got_d, want_d)
    # histories alone (a bare array, as before), masks alone (nsave = 0: the loop runs to the diff list's maximum)
    only_h = mhi.historySequence(d, *args, list(h["save"]))
    assert np.array_equal(host(only_h), want_h)
    e, only_d = mhi.historySequence(d, *args, [], saveDiffFrames=[8, 3])
    assert e.shape[0] == 0 and np.array_equal(host(only_d), R.history_seq(frames, *args, (), (8, 3))[1])
    # four channels: the same as three
    f4 = C.history_frames(4)
    w4 = R.history_seq(f4, *args, h["save"], h["save_diff"])
    g4 = mhi.historySequence(dev(f4), *args, list(h["save"]), saveDiffFrames=list(h["save_diff"]))
    assert np.array_equal(host(g4[0]), w4[0]) and np.array_equal(host(g4[1]), w4[1])


def test_sequence_one_channel_equals_the_old_entry_point(ctx):
    lib, check = _lib()
    h = C1.HISTORY
    frames = dev(C1.history_frames())
    F, rows, cols = frames.shape
    save = np.array(h["save"], np.int32)
    old, new = dev_block(save.size * rows * cols), dev_block(save.size * rows * cols)
    check(lib.micv_mhi_history_seq_dev(ctx.handle, frames.data_ptr(), F, rows * cols, cols, rows, cols, float(h["thresh"]),
                                       h["ksize"][0], h["ksize"][1], h["sigma"], h["tau"], save.ctypes.data, save.size,
                                       old.data_ptr(), rows * cols, cols, _stream()))
    check(lib.micv_mhi_history_seq_c_dev(ctx.handle, frames.data_ptr(), F, rows * cols, cols, rows, cols, 1,
                                         float(h["thresh"]), h["ksize"][0], h["ksize"][1], h["sigma"], h["tau"],
                                         save.ctypes.data, save.size, new.data_ptr(), rows * cols, cols, None, 0, None, 0, 0,
                                         _stream()))
    assert np.array_equal(host(new), host(old))
    assert np.array_equal(host(new).reshape(save.size, rows, cols), C1.history_expected())


# ------------------------------------------------------------------------------------------- the batch

def _batch_call(ctx, vids, specs, blur, out, out_pitch, out_stride, nvideos=None, **over):
    lib, _ = _lib()
    V = len(vids) if nvideos is None else nvideos
    v0 = vids[0]
    ch = 1 if v0.dim() == 3 else v0.shape[3]
    a = dict(ptrs=(ctypes.c_void_p * len(vids))(*[v.data_ptr() for v in vids]),
             nfr=np.array([v.shape[0] for v in vids], np.int32), pitch=v0.stride(0), stride=v0.stride(1), rows=v0.shape[1],
             cols=v0.shape[2], ch=ch, thresh=np.array([s["thresh"] for s in specs], np.float64),
             tau=np.array([s["tau"] for s in specs], np.int32), save=np.array([s["save"] for s in specs], np.int32))
    a.update(over)
    rc = lib.micv_mhi_history_batch_dev(ctx.handle, a["ptrs"], a["nfr"].ctypes.data, a["pitch"], a["stride"], V, a["rows"],
                                        a["cols"], a["ch"], a["thresh"].ctypes.data, a["tau"].ctypes.data,
                                        a["save"].ctypes.data, blur[0][0], blur[0][1], blur[1], out, out_pitch, out_stride,
                                        _stream())
    # the host arrays may go as soon as the call is back
    for k in ("nfr", "thresh", "tau", "save"):
        a[k][...] = 0
    return rc


@pytest.mark.parametrize("channels", [3, 4])
def test_batch_equals_the_per_video_sequence(ctx, channels):
    """7 videos of 2 .. 9 frames, taus 1, 3 and 300, two thresholds, save numbers from 1 to F - 1, written into a
    patterned block with padded rows and planes: a video that has finished keeps its bytes while the others run on (it
    would decay or move otherwise), and nothing outside the planes is written."""
    import torch
    from introtocomputervision_amd import _capi
    mhi = _mhi()
    vids = [dev(v) for v in C.batch_videos(channels)]
    rows, cols = 53, 70
    ostride, opitch, off = cols + 5, (cols + 5) * rows + 11, 3
    block = dev_block(off + 7 * opitch)
    assert _batch_call(ctx, vids, C.BATCH, C.BATCH_BLUR, block.data_ptr() + off, opitch, ostride) == _capi.OK
    got = host(torch.as_strided(block, (7, rows, cols), (opitch, ostride, 1), off))
    want = C.batch_expected(channels)
    for v, b in enumerate(C.BATCH):
        seq = host(mhi.historySequence(vids[v], b["thresh"], *C.BATCH_BLUR, b["tau"], [b["save"]], ctx=ctx))[0]
        assert np.array_equal(got[v], seq), v
        assert np.array_equal(got[v], want[v]), v
    b = np.array(host(block))
    np.lib.stride_tricks.as_strided(b[off:], (7, rows, cols), (opitch, ostride, 1))[...] = SENTINEL
    assert (b == SENTINEL).all()
    assert np.array_equal(host(mhi.historyBatch(vids, [s["thresh"] for s in C.BATCH], *C.BATCH_BLUR,
                                                [s["tau"] for s in C.BATCH], [s["save"] for s in C.BATCH], ctx=ctx)), want)


def test_batch_in_pieces_and_one_channel(ctx):
    """More videos than one by-value table holds (32): the second piece reuses the first one's words.  One channel:
    the bytes of the old micv_mhi_history_seq_dev."""
    mhi = _mhi()
    vids3 = [dev(v) for v in C.batch_videos()]
    vids = [vids3[i % 7] for i in range(37)]
    specs = [C.BATCH[i % 7] for i in range(37)]
    got = host(mhi.historyBatch(vids, [s["thresh"] for s in specs], *C.BATCH_BLUR, [s["tau"] for s in specs],
                                [s["save"] for s in specs], ctx=ctx))
    want = C.batch_expected()
    for i in range(37):
        assert np.array_equal(got[i], want[i % 7]), i
    fr = C1.history_frames()
    mono = [dev(fr[:6]), dev(fr), dev(fr[2:])]
    saves, taus = [5, 8, 1], [3, 300, 1]
    got = host(mhi.historyBatch(mono, 20, (3, 3), 1.0, taus, saves, ctx=ctx))
    for v in range(3):
        old = host(mhi.historySequence(mono[v], 20, (3, 3), 1.0, taus[v], [saves[v]], ctx=ctx))[0]
        assert np.array_equal(got[v], old), v
        assert np.array_equal(got[v], M.history_seq(host(mono[v]), 20, (3, 3), 1.0, taus[v], [saves[v]])[0]), v


# ------------------------------------------------------------------------------------------- errors

def test_bad_arguments_name_the_argument(ctx):
    from introtocomputervision_amd import _capi
    lib, _ = _lib()
    c = C.case("6x7x3-noise-b3x3-t1.7")
    f1, f2 = (dev(f) for f in C.frames(c))
    out = dev_block(6 * 7)

    def fd(ch, stride):
        return lib.micv_mhi_frame_difference_c_dev(ctx.handle, f1.data_ptr(), f2.data_ptr(), 6, 7, ch, stride, 1.7, 3, 3, 1.0,
                                                   out.data_ptr(), 7, _stream())

    def err():
        return lib.micv_last_error().decode()

    for ch in (2, 5, 0):
        assert fd(ch, 64) == _capi.EINVAL and "channels" in err()
    assert fd(3, 20) == _capi.EINVAL and "stride" in err()
    assert fd(3, 21) == _capi.OK
    fr = dev(C.history_frames())
    F, rows, cols, ch = fr.shape
    o = dev_block(2 * rows * cols)

    def seq(ch, stride, save, sdiff):
        s, d = np.array(save, np.int32), np.array(sdiff, np.int32)
        return lib.micv_mhi_history_seq_c_dev(ctx.handle, fr.data_ptr(), F, fr.stride(0), stride, rows, cols, ch, 20.0, 3, 3,
                                              1.0, 3, s.ctypes.data if s.size else None, s.size, o.data_ptr(), rows * cols,
                                              cols, d.ctypes.data if d.size else None, d.size, o.data_ptr(), rows * cols, cols,
                                              _stream())

    assert seq(2, fr.stride(1), [1], []) == _capi.EINVAL and "channels" in err()
    assert seq(3, cols * 3 - 1, [1], []) == _capi.EINVAL and "stride" in err()
    assert seq(3, fr.stride(1), [F], []) == _capi.EINVAL and "save number" in err()
    assert seq(3, fr.stride(1), [0], []) == _capi.EINVAL and "save number" in err()
    assert seq(3, fr.stride(1), [1], [F]) == _capi.EINVAL and "save_diff" in err()
    assert seq(3, fr.stride(1), [], []) == _capi.EINVAL and "save" in err()
    # the batch: nothing is enqueued, so the patterned output stays as it is
    vids = [dev(v) for v in C.batch_videos()]
    block = dev_block(7 * rows * cols)
    call = lambda **kw: _batch_call(ctx, vids, C.BATCH, C.BATCH_BLUR, block.data_ptr(), rows * cols, cols, **kw)
    assert call(nvideos=0) == _capi.EINVAL and "nvideos" in err()
    assert call(ch=2) == _capi.EINVAL and "channels" in err()
    assert call(ch=5) == _capi.EINVAL and "channels" in err()
    assert call(stride=cols * 3 - 1) == _capi.EINVAL and "stride" in err()
    bad = np.array([s["save"] for s in C.BATCH], np.int32)
    bad[4] = C.BATCH[4]["F"]
    assert call(save=bad) == _capi.EINVAL and "save[4]" in err()
    bad = np.array([s["save"] for s in C.BATCH], np.int32)
    bad[6] = 0
    assert call(save=bad) == _capi.EINVAL and "save[6]" in err()
    assert (host(block) == SENTINEL).all()
    with pytest.raises(ValueError):
        _mhi().frameDifference(f1[..., :2], f2[..., :2], 1.7)
