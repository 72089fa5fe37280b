"""ps6 particle filter on the device (csrc/pf.hip) against the exact restatement tests/_pf_ref.py, bit for bit on every
tick: the state, the particles, the weights and the model (patch and histogram)."""
import ctypes as C

import numpy as np
import pytest

import _pf_ref as ref

pytestmark = pytest.mark.gpu


def _pf():
    from introtocomputervision_amd import pf
    return pf


def scene(seed, rows, cols, ch, nframes, obj=(9, 7), start=None, step=(2, 1)):
    """Textured background and a textured object moving `step` pixels per frame; the object's top-left per frame."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    bg = ((bg.astype(np.int32) + np.roll(bg, 1, 1)) // 2).astype(np.uint8)  # some spatial correlation
    tex = rng.integers(0, 256, (obj[0], obj[1], ch), dtype=np.uint8)
    y, x = start if start is not None else (rows // 3, cols // 3)
    frames, pos = [], []
    for _ in range(nframes):
        f = bg.copy()
        yy, xx = min(max(y, 0), rows - obj[0]), min(max(x, 0), cols - obj[1])
        f[yy:yy + obj[0], xx:xx + obj[1]] = tex
        frames.append(f if ch == 3 else f[:, :, 0].copy())
        pos.append((yy, xx))
        y, x = y + step[1], x + step[0]
    return frames, pos, tex


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_both(frames, model, n, mode, mse_sigma, sample_sigma, init=(-1.0, -1.0), alpha=0.1, flags=0,
             seed=0xFFFFFFFF, ticks=None):
    pf = _pf()
    rows, cols = frames[0].shape[:2]
    r = ref.PF(model, rows, cols, n, mode, mse_sigma, sample_sigma, init, alpha, flags, seed)
    g = pf.ParticleFilter(model, (cols, rows), n, mode, mse_sigma, sample_sigma, init, alpha, flags=flags, seed=seed)
    assert np.array_equal(bits(g.getParticles()), bits(r.particles)), "initial particles"
    assert np.array_equal(bits(g.weights()), bits(r.weights))
    statuses = []
    for t, f in enumerate(frames[:ticks]):
        want = r.tick(f)
        (gx, gy), gxv, gyv = g.tick(f)
        got = (gx, gy, gxv, gyv, g.last_status)
        assert [bits(np.float32(v)) for v in got[:4]] == [bits(np.float32(v)) for v in want[:4]], (t, got, want)
        assert got[4] == want[4], (t, got, want)
        assert np.array_equal(bits(g.getParticles()), bits(r.particles)), f"particles after tick {t}"
        assert np.array_equal(bits(g.weights()), bits(r.weights)), f"weights after tick {t}"
        patch, hist = g.model()
        assert np.array_equal(patch, r.model), f"model patch after tick {t}"
        assert np.array_equal(bits(hist), bits(r.hist)), f"model histogram after tick {t}"
        statuses.append(want[4])
    return g, r, statuses


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("mode,flags", [(ref.MSE, 0), (ref.MSE, ref.MSE_SIGNED), (ref.HIST, 0)])
def test_modes_track_bit_exact(mode, flags, ch):
    frames, pos, tex = scene(11 + ch, 40, 56, ch, 6)
    model = tex if ch == 3 else tex[:, :, 0]
    y0, x0 = pos[0]
    run_both(frames, model, 300, mode, 3.0 if mode == ref.MSE else 0.0, 2.5, init=(float(x0), float(y0)),
             alpha=0.15, flags=flags)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300, 700, 4096])
def test_particle_counts(n):
    frames, pos, tex = scene(5, 32, 40, 3, 3, obj=(5, 6))
    mode = ref.HIST if n in (63, 700) else ref.MSE
    run_both(frames, tex, n, mode, 10.0, 3.0, init=(float(pos[0][1]), float(pos[0][0])))


@pytest.mark.parametrize("shape", [(7, 5), (8, 6), (1, 1), (24, 30)], ids=["odd", "even", "1x1", "full"])
@pytest.mark.parametrize("mode", [ref.MSE, ref.HIST])
def test_patch_sizes(shape, mode):
    frames, pos, _ = scene(7, 24, 30, 3, 3, obj=(5, 5))
    model = frames[0][:shape[0], :shape[1]].copy()
    run_both(frames, model, 65, mode, 20.0, 4.0)


def test_particles_on_and_past_every_border():
    # GAUSSIAN init centred at (W - 0.25, H - 0.25) with sigma 0.4: particles in [W - 0.5, W) (cvRound gives W),
    # past the right / bottom borders, and (second filter) around the top-left corner.
    frames, _, _ = scene(9, 20, 26, 3, 4, obj=(4, 4))
    model = frames[0][:5, :4].copy()
    rows, cols = 20, 26
    init = (cols - 0.25 - 2.0, rows - 0.25 - 2.5)
    _, r, _ = run_both(frames, model, 300, ref.MSE, 30.0, 0.4, init=init)
    p0 = ref.gen_particles(0xFFFFFFFF, 300, False, cols, rows, 0.4, np.float32(cols - 0.25), np.float32(rows - 0.25))
    assert ((p0[:, 0] >= cols - 0.5) & (p0[:, 0] < cols)).any() and (p0[:, 0] >= cols).any()
    run_both(frames, model, 300, ref.HIST, 0.0, 0.6, init=(-2.25, -2.75))


def test_every_weight_underflows():
    frames, _, _ = scene(13, 24, 32, 3, 3)
    model = np.full((6, 6, 3), 255, np.uint8)
    frames = [np.zeros_like(f) for f in frames]
    _, _, st = run_both(frames, model, 64, ref.MSE, 1.5, 3.0, flags=ref.MSE_SIGNED)
    assert all(s & ref.STATUS_NO_WEIGHT for s in st)


def test_clamped_resampling_flag():
    # weights that underflow in float but not in double: every u >= cum[n-1] = 0 clamps to n - 1
    frames, _, _ = scene(14, 24, 32, 1, 2)
    model = np.full((6, 6), 255, np.uint8)
    frames = [np.full_like(f, 50) for f in frames]
    # mse = 205^2 = 42025 (signed); sigma^2 = 42025 / (2 * 730): sim ~ e^-730 ~ 1e-317 (double subnormal, float 0)
    sigma = (42025 / (2 * 730.0)) ** 0.5
    _, _, st = run_both(frames, model, 64, ref.MSE, sigma, 3.0, flags=ref.MSE_SIGNED)
    assert all(s & ref.STATUS_CLAMPED for s in st) and not any(s & ref.STATUS_NO_WEIGHT for s in st)


@pytest.mark.parametrize("init", [(-1.0, -1.0), (12.0, 9.0)], ids=["uniform", "gaussian"])
def test_init_modes(init):
    frames, _, tex = scene(15, 36, 48, 3, 3)
    run_both(frames, tex, 200, ref.MSE, 4.0, 5.0, init=init, seed=12345)


def test_sequence_equals_host_ticks_and_dev_agrees():
    import torch
    pf = _pf()
    frames, pos, tex = scene(21, 48, 64, 3, 8)
    init = (float(pos[0][1]), float(pos[0][0]))
    a = pf.ParticleFilter(tex, (64, 48), 300, pf.MEAN_SQ_ERR, 3.0, 2.0, init)
    b = pf.ParticleFilter(tex, (64, 48), 300, pf.MEAN_SQ_ERR, 3.0, 2.0, init)
    c = pf.ParticleFilter(tex, (64, 48), 300, pf.MEAN_SQ_ERR, 3.0, 2.0, init)
    states, parts = a.track(frames, with_particles=True)
    dstate = torch.empty(5, dtype=torch.int32, device="cuda")
    for t, f in enumerate(frames):
        (hx, hy), hxv, hyv = b.tick(f)
        host_state = np.array([(hx, hy, hxv, hyv, b.last_status)], pf.STATE_DTYPE)[0]
        assert host_state.tobytes() == states[t].tobytes(), t
        host_parts = b.getParticles()
        dstate = c.tick(torch.from_numpy(f).cuda())
        dparts = torch.empty((300, 2), dtype=torch.float32, device="cuda")
        c.getParticles(dparts)
        dw = torch.empty(300, dtype=torch.float32, device="cuda")
        c.weights(dw)
        torch.cuda.synchronize()
        assert np.array_equal(bits(parts[t]), bits(host_parts)), t
        assert np.array_equal(bits(dparts.cpu().numpy()), bits(host_parts)), t
        assert np.array_equal(bits(dw.cpu().numpy()), bits(b.weights())), t
        ds = pf.ParticleFilter.state_from_device(dstate)
        assert ds.tobytes() == states[t].tobytes(), t
    r = ref.PF(tex, 48, 64, 300, ref.MSE, 3.0, 2.0, init)
    for t, f in enumerate(frames):
        want = r.tick(f)
        assert [bits(np.float32(v)) for v in want[:4]] == [bits(np.float32(states[t][k]))
                                                           for k in ("x", "y", "x_var", "y_var")]
    # a tracked object: the estimate follows the object's centre
    cy, cx = pos[-1][0] + tex.shape[0] / 2, pos[-1][1] + tex.shape[1] / 2
    assert abs(states[-1]["x"] - cx) < 3 and abs(states[-1]["y"] - cy) < 3, (states[-1], cx, cy)


def test_full_size_pfconf1_head():
    """runProblem1's configuration on a 480 x 640 x 3 sequence with a 129 x 104 head model."""
    frames, pos, tex = scene(31, 480, 640, 3, 4, obj=(129, 104), start=(150, 300), step=(3, 2))
    run_both(frames, tex, 300, ref.MSE, 3.0, 6.5, init=(300.0, 150.0), alpha=0.1)


def test_einval_paths_enqueue_nothing():
    import torch
    pf = _pf()
    from introtocomputervision_amd._capi import EINVAL, lib
    from introtocomputervision_amd.lk import default_context
    ctx = default_context(0).handle
    model = np.zeros((4, 4, 3), np.uint8)
    h = C.c_void_p()

    def create(**kw):
        a = dict(model=model.ctypes.data, mrows=4, mcols=4, mstride=12, ch=3, rows=20, cols=20, n=10, mode=0,
                 mse=1.0, ss=1.0, ix=-1.0, iy=-1.0, alpha=0.1, flags=0, seed=0xFFFFFFFF)
        a.update(kw)
        return lib.micv_pf_create(ctx, a["model"], a["mrows"], a["mcols"], a["mstride"], a["ch"], a["rows"],
                                  a["cols"], a["n"], a["mode"], a["mse"], a["ss"], a["ix"], a["iy"], a["alpha"],
                                  a["flags"], a["seed"], C.byref(h))
    for bad in [dict(n=0), dict(n=4097), dict(ch=2), dict(ch=4), dict(mrows=21), dict(mcols=21), dict(mrows=0),
                dict(mode=2), dict(mse=0.0), dict(mse=float("inf")), dict(ss=float("nan")), dict(ss=-1.0),
                dict(alpha=float("inf")), dict(flags=2), dict(mstride=11), dict(model=None),
                dict(ix=5.0, iy=5.0, ss=0.0)]:
        assert create(**bad) == EINVAL, bad
    assert create(mode=1, mse=0.0) == 0  # MEAN_SHIFT_LT ignores mse_sigma
    lib.micv_pf_destroy(h)

    frames, pos, tex = scene(41, 30, 40, 3, 3)
    r = ref.PF(tex, 30, 40, 100, ref.MSE, 3.0, 2.0, (float(pos[0][1]), float(pos[0][0])))
    g = pf.ParticleFilter(tex, (40, 30), 100, pf.MEAN_SQ_ERR, 3.0, 2.0, (float(pos[0][1]), float(pos[0][0])))
    before = (g.getParticles().copy(), g.weights().copy())
    f = frames[0]
    st = np.zeros(1, pf.STATE_DTYPE)
    assert lib.micv_pf_tick_host(g._h, f.ctypes.data, 119, st.ctypes.data) == EINVAL
    assert lib.micv_pf_tick_host(g._h, None, 120, st.ctypes.data) == EINVAL
    assert lib.micv_pf_tick_host(None, f.ctypes.data, 120, st.ctypes.data) == EINVAL
    df = torch.from_numpy(f).cuda()
    assert lib.micv_pf_tick_dev(g._h, df.data_ptr(), 119, None, None) == EINVAL
    assert lib.micv_pf_tick_dev(g._h, None, 120, None, None) == EINVAL
    assert lib.micv_pf_track_seq_host(g._h, None, 1, 120, st.ctypes.data, None) == EINVAL
    ptrs = (C.c_void_p * 1)(f.ctypes.data)
    assert lib.micv_pf_track_seq_host(g._h, ptrs, 0, 120, st.ctypes.data, None) == EINVAL
    assert lib.micv_pf_track_seq_host(g._h, ptrs, 1, 100, st.ctypes.data, None) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(bits(g.getParticles()), bits(before[0])) and np.array_equal(bits(g.weights()), bits(before[1]))
    for t, fr in enumerate(frames):  # and the filter goes on as if nothing had been called
        want = r.tick(fr)
        (gx, gy), _, _ = g.tick(fr)
        assert (bits(np.float32(gx)), bits(np.float32(gy))) == (bits(np.float32(want[0])), bits(np.float32(want[1])))
        assert np.array_equal(bits(g.getParticles()), bits(r.particles)), t
