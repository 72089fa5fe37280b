"""The "ps6: driver" block on the device (csrc/ps6.hip) against tests/_ps6_driver_ref.py, byte for byte: the dots and the
ring in one launch on every case of the restatement (padding included), the overlay from the filter's own device state,
pfDriver's loop body in place and into a separate image, and the whole loop as one call against per-frame calls and
against the plain tracker, whose states it must not perturb."""
import ctypes as C

import numpy as np
import pytest

import _ps6_driver_ref as R
from _ps6_driver_ref import scene

pytestmark = pytest.mark.gpu

CASES = R.cases()
EXPECTED = {c[0]: R.apply_case(c) for c in CASES}  # computed once, never written to
SIZE = (9.0, 7.0)


def _mods():
    import torch
    from introtocomputervision_amd import pf, ps6
    return torch, pf, ps6


def dev_image(torch, ch, pad):
    buf, _ = R.image(R.ROWS, R.COLS, ch, pad)
    t = torch.from_numpy(buf).cuda()
    return t, t.as_strided((R.ROWS, R.COLS, ch), (R.COLS * ch + pad, ch, 1))


def test_every_case_on_the_device():
    torch, _, ps6 = _mods()
    for name, ch, pad, particles, dot, box, box_colour in CASES:
        buf, view = dev_image(torch, ch, pad)
        p = torch.from_numpy(particles).cuda() if particles is not None else torch.zeros((0, 2), dtype=torch.float32, device="cuda")
        if box is None:
            ps6.drawParticles(view, p, dot)
        else:
            centre = torch.tensor(box[0], dtype=torch.float32, device="cuda")
            ps6.overlay(view, p, centre, box[1], dot, box_colour)
        assert np.array_equal(buf.cpu().numpy(), EXPECTED[name]), name


def test_every_case_from_host_memory():
    _, _, ps6 = _mods()
    for name, ch, pad, particles, dot, box, box_colour in CASES:
        buf, view = R.image(R.ROWS, R.COLS, ch, pad)
        p = particles if particles is not None else np.zeros((0, 2), np.float32)
        if box is None:
            ps6.drawParticles(view, p, dot)
        else:
            ps6.overlay(view, p, box[0], box[1], dot, box_colour)
        assert np.array_equal(buf, EXPECTED[name]), name


def test_dots_then_rectangle_as_two_calls_give_the_same_bytes():
    torch, _, ps6 = _mods()
    for name, ch, pad, particles, dot, box, box_colour in CASES:
        if box is None:
            continue
        buf, view = dev_image(torch, ch, pad)
        if particles is not None:
            ps6.drawParticles(view, torch.from_numpy(particles).cuda(), dot)
        ps6.rectangle(view, ps6.boxRect(box[0], box[1]), box_colour)
        assert np.array_equal(buf.cpu().numpy(), EXPECTED[name]), name


def test_integer_rectangles():
    torch, _, ps6 = _mods()
    for c in R.rect_cases():
        name, ch, pad, rect, colour = c
        want = R.apply_rect_case(c)
        buf, view = dev_image(torch, ch, pad)
        ps6.rectangle(view, rect, colour)
        assert np.array_equal(buf.cpu().numpy(), want), name
        hbuf, hview = R.image(R.ROWS, R.COLS, ch, pad)
        ps6.rectangle(hview, rect, colour)
        assert np.array_equal(hbuf, want), name


def test_box_rect_equals_the_restatement():
    _, _, ps6 = _mods()
    for name, (centre, size) in R.boxes().items():
        assert ps6.boxRect(centre, size) == R.box_rect(centre, size), name


def make_filter(pf, frames, pos, tex, n, mode):
    rows, cols = frames[0].shape[:2]
    return pf.ParticleFilter(tex, (cols, rows), n, mode, 10.0 if mode == pf.MEAN_SQ_ERR else 0.0, 3.0,
                             (float(pos[0][1]), float(pos[0][0])), alpha=0.15)


def state_bytes(st):
    return np.asarray(st).tobytes()


@pytest.mark.parametrize("ch", [1, 3])
def test_overlay_from_the_filters_own_state_after_a_tick(ch):
    torch, pf, ps6 = _mods()
    frames, pos, tex = scene(21, 48, 64, ch, 3)
    model = tex if ch == 3 else tex[:, :, 0]
    g = make_filter(pf, frames, pos, model, 300, pf.MEAN_SQ_ERR)
    for f in frames:
        d = torch.from_numpy(f).cuda()
        st = g.tick(d)
        painted = ps6.overlayFilter(g, d.clone(), SIZE)
        torch.cuda.synchronize()
        s = g.state_from_device(st)
        want = R.overlay(f, g.getParticles(), R.DOT, (s["x"], s["y"]), SIZE, R.BOX)
        assert np.array_equal(painted.cpu().numpy(), want)
        assert np.array_equal(d.cpu().numpy(), f)
        assert not np.array_equal(want, f)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_tick_display_in_place_and_into_a_separate_image(dev):
    torch, pf, ps6 = _mods()
    frames, pos, tex = scene(22, 48, 64, 3, 4)
    a, b, plain = (make_filter(pf, frames, pos, tex, 300, pf.MEAN_SQ_ERR) for _ in range(3))
    for f in frames:
        fa, fb = (torch.from_numpy(f).cuda(), torch.from_numpy(f).cuda()) if dev else (f.copy(), f.copy())
        sa, oa = ps6.tickDisplay(a, fa, SIZE, out=fa)
        sb, ob = ps6.tickDisplay(b, fb, SIZE)
        want_state = plain.tick(f)
        if dev:
            torch.cuda.synchronize()
            sa, sb, oa, ob, fb = a.state_from_device(sa), b.state_from_device(sb), oa.cpu().numpy(), ob.cpu().numpy(), fb.cpu().numpy()
        assert state_bytes(sa) == state_bytes(sb)
        assert (sa["x"], sa["y"], sa["x_var"], sa["y_var"]) == (want_state[0][0], want_state[0][1], want_state[1], want_state[2])
        assert np.array_equal(oa, ob) and np.array_equal(fb, f)  # equal bytes; the source of the separate form untouched
        assert np.array_equal(oa, R.overlay(f, a.getParticles(), R.DOT, (sa["x"], sa["y"]), SIZE, R.BOX))
        # the tracker never saw the paint: the models agree with the plain filter's
        assert np.array_equal(a.model()[0], plain.model()[0]) and np.array_equal(b.model()[0], plain.model()[0])


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("mode", [0, 1], ids=["mse", "hist"])
def test_sequence_as_one_call(mode, n):
    _, pf, ps6 = _mods()
    frames, pos, tex = scene(23 + mode, 48, 64, 3, 8)
    twin = make_filter(pf, frames, pos, tex, n, mode)
    want_states = twin.track(frames)
    per_frame = make_filter(pf, frames, pos, tex, n, mode)
    want_frames = []
    for f in frames:
        st, out = ps6.tickDisplay(per_frame, f, SIZE)
        want_frames.append(out)
        assert not np.array_equal(out, f)
    originals = [f.copy() for f in frames]
    for save, every in (((0, 3, 7), False), ((), False), ((), True), ((1, 2, 3, 4, 5), False)):  # the last: buffers re-used, t and t + 2 kept
        g = make_filter(pf, frames, pos, tex, n, mode)
        states, kept = ps6.trackDisplay(g, frames, SIZE, save, every)
        assert states.tobytes() == want_states.tobytes(), (save, every)  # the overlay never perturbs the tracker
        assert sorted(kept) == (list(range(len(frames))) if every else sorted(save))
        for t, img in kept.items():
            assert np.array_equal(img, want_frames[t]), (save, every, t)
        assert all(np.array_equal(a, b) for a, b in zip(frames, originals))


def test_pf_driver_and_the_problems():
    _, pf, ps6 = _mods()
    frames, pos, tex = scene(29, 48, 64, 3, 5)
    conf = dict(num_particles=65, mse_sigma=10.0, dynamics_sigma=3.0, alpha=0.15)
    bbox, size = (pos[0][1] + 0.4, pos[0][0] - 0.4), (7.2, 8.6)  # cvRound: the object's corner, 7 x 9
    states, kept = ps6.pfDriver(frames, bbox, size, conf, pf.MEAN_SQ_ERR, (1, 4, 28))
    assert sorted(kept) == [1, 4]
    g = pf.ParticleFilter(tex, (64, 48), 65, pf.MEAN_SQ_ERR, 10.0, 3.0, bbox)
    for t, f in enumerate(frames):
        st, out = ps6.tickDisplay(g, f, size)
        assert state_bytes(st) == states[t].tobytes()
        if t in kept:
            assert np.array_equal(out, kept[t])


def test_einval_paths_enqueue_nothing():
    torch, pf, ps6 = _mods()
    from introtocomputervision_amd._capi import EINVAL, lib
    from introtocomputervision_amd.lk import default_context
    ctx = default_context(0).handle
    rows, cols = 12, 16
    img = torch.full((rows, cols * 3), 0xA5, dtype=torch.uint8, device="cuda")
    xy = torch.tensor([[3.0, 3.0], [8.0, 6.0]], dtype=torch.float32, device="cuda")
    centre = torch.tensor([8.0, 6.0], dtype=torch.float32, device="cuda")
    col = (C.c_double * 4)(1, 2, 3, 4)
    ip, xp, cp = img.data_ptr(), xy.data_ptr(), centre.data_ptr()
    bad = [
        lib.micv_draw_particles_dev(ctx, None, rows, cols, 3, cols * 3, xp, 2, col, None),
        lib.micv_draw_particles_dev(ctx, ip, rows, cols, 3, cols * 3, None, 2, col, None),
        lib.micv_draw_particles_dev(ctx, ip, rows, cols, 3, cols * 3, xp, 2, None, None),
        lib.micv_draw_particles_dev(None, ip, rows, cols, 3, cols * 3, xp, 2, col, None),
        lib.micv_draw_particles_dev(ctx, ip, rows, cols, 3, cols * 3, xp, -1, col, None),
        lib.micv_draw_particles_dev(ctx, ip, rows, cols, 3, cols * 3 - 1, xp, 2, col, None),
        lib.micv_draw_particles_dev(ctx, ip, rows, cols, 2, cols * 3, xp, 2, col, None),
        lib.micv_draw_particles_dev(ctx, ip, 0, cols, 3, cols * 3, xp, 2, col, None),
        lib.micv_draw_rectangle_dev(ctx, None, rows, cols, 3, cols * 3, 1, 1, 5, 5, col, None),
        lib.micv_draw_rectangle_dev(ctx, ip, rows, cols, 2, cols * 3, 1, 1, 5, 5, col, None),
        lib.micv_draw_rectangle_dev(ctx, ip, rows, cols, 3, cols * 3 - 1, 1, 1, 5, 5, col, None),
        lib.micv_draw_rectangle_dev(ctx, ip, rows, cols, 3, cols * 3, 1, 1, 5, 5, None, None),
        lib.micv_ps6_overlay_list_dev(ctx, ip, rows, cols, 3, cols * 3, xp, 2, col, None, 5.0, 5.0, col, None),
        lib.micv_ps6_overlay_list_dev(ctx, ip, rows, cols, 2, cols * 3, xp, 2, col, cp, 5.0, 5.0, col, None),
        lib.micv_ps6_overlay_list_dev(ctx, ip, rows, cols, 3, cols * 3 - 1, xp, 2, col, cp, 5.0, 5.0, col, None),
    ]
    himg = np.full((rows, cols * 3), 0xA5, np.uint8)
    hxy = np.array([[3, 3], [8, 6]], np.float32)
    bad += [
        lib.micv_draw_particles_host(ctx, himg.ctypes.data, rows, cols, 2, cols * 3, hxy.ctypes.data, 2, col),
        lib.micv_draw_particles_host(ctx, himg.ctypes.data, rows, cols, 3, cols * 3 - 1, hxy.ctypes.data, 2, col),
        lib.micv_draw_particles_host(ctx, None, rows, cols, 3, cols * 3, hxy.ctypes.data, 2, col),
        lib.micv_draw_rectangle_host(ctx, himg.ctypes.data, rows, cols, 2, cols * 3, 1, 1, 5, 5, col),
        lib.micv_draw_rectangle_host(ctx, himg.ctypes.data, rows, cols, 3, cols * 3 - 1, 1, 1, 5, 5, col),
    ]
    # the filter forms
    frames, pos, tex = scene(31, rows, cols, 3, 3, obj=(5, 5))
    g = make_filter(pf, frames, pos, tex, 65, pf.MEAN_SQ_ERR)
    before = g.getParticles().copy()
    fr = torch.from_numpy(frames[0]).cuda()
    st = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    fp, sp = fr.data_ptr(), st.data_ptr()
    bad += [
        lib.micv_ps6_overlay_dev(None, ip, cols * 3, col, 5.0, 5.0, col, None),
        lib.micv_ps6_overlay_dev(g._h, None, cols * 3, col, 5.0, 5.0, col, None),
        lib.micv_ps6_overlay_dev(g._h, ip, cols * 3 - 1, col, 5.0, 5.0, col, None),
        lib.micv_ps6_overlay_dev(g._h, ip, cols * 3, None, 5.0, 5.0, col, None),
        lib.micv_ps6_tick_display_dev(g._h, None, cols * 3, ip, cols * 3, col, 5.0, 5.0, col, None, sp),
        lib.micv_ps6_tick_display_dev(g._h, fp, cols * 3, None, cols * 3, col, 5.0, 5.0, col, None, sp),
        lib.micv_ps6_tick_display_dev(g._h, fp, cols * 3 - 1, ip, cols * 3, col, 5.0, 5.0, col, None, sp),
        lib.micv_ps6_tick_display_dev(g._h, fp, cols * 3, ip, cols * 3 - 1, col, 5.0, 5.0, col, None, sp),
    ]
    hstate = np.full(5, -1, np.int32)
    hout = np.full((rows, cols * 3), 0xA5, np.uint8)
    bad += [
        lib.micv_ps6_tick_display_host(g._h, frames[0].ctypes.data, cols * 3 - 1, hout.ctypes.data, cols * 3, col, 5.0, 5.0, col, hstate.ctypes.data),
        lib.micv_ps6_tick_display_host(g._h, frames[0].ctypes.data, cols * 3, None, cols * 3, col, 5.0, 5.0, col, hstate.ctypes.data),
        lib.micv_ps6_tick_display_host(g._h, frames[0].ctypes.data, cols * 3, hout.ctypes.data, cols * 3, col, 5.0, 5.0, col, None),
    ]
    ptrs = (C.c_void_p * 3)(*[f.ctypes.data for f in frames])
    outs = [np.full((rows, cols * 3), 0xA5, np.uint8) for _ in range(2)]
    optrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    hstates = np.full(15, -1, np.int32)

    def seq(frames_p=ptrs, nframes=3, stride=cols * 3, save=(0, 2), out_p=optrs, ostride=cols * 3, states_p=hstates.ctypes.data):
        sv = (C.c_int * max(len(save), 1))(*save)
        return lib.micv_ps6_track_display_seq_host(g._h, frames_p, nframes, stride, col, 5.0, 5.0, col, sv, len(save), 0, out_p, ostride,
                                                   states_p)

    bad += [seq(save=(0, 3)), seq(save=(-1, 1)), seq(frames_p=None), seq(stride=cols * 3 - 1), seq(out_p=None), seq(ostride=cols * 3 - 1),
            seq(states_p=None), seq(nframes=0)]
    assert bad == [EINVAL] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((img == 0xA5).all()) and bool((st == -1).all()) and np.all(himg == 0xA5) and np.all(hout == 0xA5)
    assert np.all(hstate == -1) and np.all(hstates == -1) and all(np.all(o == 0xA5) for o in outs)
    assert np.array_equal(g.getParticles(), before)  # no tick ran
    assert np.array_equal(fr.cpu().numpy(), frames[0])
