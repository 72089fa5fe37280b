"""A group of particle filters ticked together (micv_pf_group, csrc/pf.hip; the group form of the ps6 driver, csrc/ps6.hip)
against TWIN filters made with the same arguments and ticked alone: after every tick the state, the particles, the weights,
the model patch and the model histogram of every member must be the twin's, bit for bit.  The single path is pinned to the
restatement tests/_pf_ref.py by test_pf_gpu.py; one small group is checked against it directly as well, and the status-bit
members are run through it on the CPU (the one test here that needs no GPU)."""
import ctypes as C

import numpy as np
import pytest

import _pf_ref as ref

gpu = pytest.mark.gpu
ROWS, COLS = 24, 32
# the members of the status test: (model value, frame value, mode, flags, mse_sigma) and what each tick must report
CLAMP_SIGMA = (3 * 42025 / (2 * 730.0)) ** 0.5  # mse 3 * 205^2: sim ~ e^-730, a double subnormal that is 0 as a float
STATUSES = [ref.STATUS_NO_WEIGHT, ref.STATUS_CLAMPED, 0, 0]


def _pf():
    from introtocomputervision_amd import pf
    return pf


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def scene(seed, rows, cols, ch, nframes, obj=(9, 7), step=(2, 1)):
    """Textured background and a textured object moving `step` pixels per frame -> (frames, top-left per frame, texture)."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    bg = ((bg.astype(np.int32) + np.roll(bg, 1, 1)) // 2).astype(np.uint8)
    tex = rng.integers(0, 256, (obj[0], obj[1], ch), dtype=np.uint8)
    y, x = rows // 3, cols // 3
    frames, pos = [], []
    for _ in range(nframes):
        f = bg.copy()
        yy, xx = min(max(y, 0), rows - obj[0]), min(max(x, 0), cols - obj[1])
        f[yy:yy + obj[0], xx:xx + obj[1]] = tex
        frames.append(f if ch == 3 else f[:, :, 0].copy())
        pos.append((yy, xx))
        y, x = y + step[1], x + step[0]
    return frames, pos, tex


def make(spec, rows=ROWS, cols=COLS):
    """spec: dict(model, n, mode, mse, ss, init, alpha, flags, seed) -> pf.ParticleFilter."""
    pf = _pf()
    return pf.ParticleFilter(spec["model"], (cols, rows), spec["n"], spec["mode"], spec.get("mse", 3.0), spec.get("ss", 2.0),
                             spec.get("init", (-1.0, -1.0)), spec.get("alpha", 0.1), flags=spec.get("flags", 0),
                             seed=spec.get("seed", 0xFFFFFFFF))


def make_ref(spec, rows=ROWS, cols=COLS):
    return ref.PF(spec["model"], rows, cols, spec["n"], spec["mode"], spec.get("mse", 3.0), spec.get("ss", 2.0),
                  spec.get("init", (-1.0, -1.0)), spec.get("alpha", 0.1), spec.get("flags", 0), spec.get("seed", 0xFFFFFFFF))


def snapshot(f):
    patch, hist = f.model()
    return [bits(f.getParticles()).copy(), bits(f.weights()).copy(), patch, bits(hist).copy()]


def same_everywhere(members, twins, label):
    for k, (m, t) in enumerate(zip(members, twins)):
        for name, a, b in zip(("particles", "weights", "model patch", "model histogram"), snapshot(m), snapshot(t)):
            assert np.array_equal(a, b), f"{label}: member {k}: {name}"


def dev(f):
    import torch
    return torch.from_numpy(np.ascontiguousarray(f)).cuda()


def tick_both(group, twins, gframes, tframes, label):
    """One group tick on gframes (a tensor or K tensors) and one tick of every twin on its frame of tframes; -> the K
    state records of the group after comparing them and everything else with the twins'."""
    pf = _pf()
    st = group.tick(gframes)
    want = [pf.ParticleFilter.state_from_device(t.tick(f)) for t, f in zip(twins, tframes)]
    got = pf.FilterGroup.states_from_device(st)
    assert got.shape == (len(twins),)
    for k, w in enumerate(want):
        assert got[k].tobytes() == w.tobytes(), f"{label}: state of member {k}: {got[k]} != {w}"
    same_everywhere(group.filters, twins, label)
    return got


def mixed_specs(ch, frames, pos, tex):
    f0 = frames[0]
    model = (lambda a: a if ch == 3 else (a[:, :, 0] if a.ndim == 3 else a))
    y0, x0 = pos[0]
    return [dict(model=model(f0[5:6, 7:8].copy()), n=1, mode=ref.MSE, mse=20.0, ss=3.0, alpha=0.1, seed=11),
            dict(model=model(tex[:7, :5].copy()), n=64, mode=ref.MSE, flags=ref.MSE_SIGNED, mse=9.0, ss=2.5, init=(float(x0), float(y0)),
                 alpha=0.2, seed=12),
            dict(model=model(tex[:8, :6].copy()), n=65, mode=ref.HIST, ss=4.0, alpha=0.05, seed=13),
            dict(model=model(f0.copy()), n=300, mode=ref.HIST, ss=1.5, init=(0.0, 0.0), alpha=0.3, seed=14),
            dict(model=model(tex[:7, :5].copy()), n=4096, mode=ref.MSE, mse=30.0, ss=3.5, alpha=0.15, seed=0xFFFFFFFF)]


@gpu
@pytest.mark.parametrize("ch", [3, 1])
def test_mixed_members_on_one_shared_frame(ch):
    pf = _pf()
    frames, pos, tex = scene(100 + ch, ROWS, COLS, ch, 4)
    specs = mixed_specs(ch, frames, pos, tex)
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    group = pf.FilterGroup(members)
    same_everywhere(members, twins, "before the first tick")
    refs = [make_ref(s) for s in specs[:2]] if ch == 3 else []  # the two small members against the restatement itself
    for t, f in enumerate(frames):
        d = dev(f)
        states = tick_both(group, twins, d, [d] * len(twins), f"tick {t}")
        for k, r in enumerate(refs):
            want = r.tick(f)
            got = states[k]
            assert [bits(np.float32(got[n])) for n in ("x", "y", "x_var", "y_var")] == [bits(np.float32(v)) for v in want[:4]], (t, k)
            assert int(got["status"]) == want[4]
            assert np.array_equal(bits(members[k].getParticles()), bits(r.particles)), (t, k)
            assert np.array_equal(bits(members[k].weights()), bits(r.weights)), (t, k)
            assert np.array_equal(members[k].model()[0], r.model), (t, k)
    group.close()


@gpu
def test_a_frame_per_member_and_then_one_for_all():
    import torch
    pf = _pf()
    scenes = [scene(200 + k, ROWS, COLS, 3, 3) for k in range(4)]
    specs = [dict(model=scenes[k][2][:7, :5].copy(), n=n, mode=mode, mse=8.0, ss=2.0, alpha=0.1 + 0.05 * k, seed=20 + k)
             for k, (n, mode) in enumerate([(65, ref.MSE), (300, ref.HIST), (64, ref.MSE), (130, ref.HIST)])]
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    group = pf.FilterGroup(members)
    for t in range(3):
        frames = [dev(scenes[k][0][t]) for k in range(4)]
        wide = torch.full((ROWS, COLS + 8, 3), 77, dtype=torch.uint8, device="cuda")  # member 2's frame: a padded row stride
        wide[:, :COLS] = frames[2]
        frames[2] = wide[:, :COLS]
        assert frames[2].stride(0) == (COLS + 8) * 3
        tick_both(group, twins, frames, frames, f"own frames, tick {t}")
    shared = dev(scenes[0][0][2])
    tick_both(group, twins, shared, [shared] * 4, "one frame for all")
    tick_both(group, twins, [shared], [shared] * 4, "a list of one frame")
    group.close()


def status_specs():
    hot = np.full((6, 6, 3), 255, np.uint8)
    frames, pos, tex = scene(300, ROWS, COLS, 3, 3)
    specs = [dict(model=hot, n=64, mode=ref.MSE, flags=ref.MSE_SIGNED, mse=1.5, ss=3.0),
             dict(model=hot, n=64, mode=ref.MSE, flags=ref.MSE_SIGNED, mse=CLAMP_SIGMA, ss=3.0),
             dict(model=tex.copy(), n=100, mode=ref.MSE, mse=10.0, ss=2.0, init=(float(pos[0][1]), float(pos[0][0])), seed=31),
             dict(model=tex.copy(), n=100, mode=ref.HIST, ss=2.0, init=(float(pos[0][1]), float(pos[0][0])), seed=32)]
    per_tick = [[np.zeros((ROWS, COLS, 3), np.uint8), np.full((ROWS, COLS, 3), 50, np.uint8), f, f] for f in frames]
    return specs, per_tick


def test_the_status_members_give_their_statuses_in_the_restatement():
    """No GPU: the four members of the status test through tests/_pf_ref.py -- NO_WEIGHT, CLAMPED without NO_WEIGHT, and no
    bit on the two ordinary members, on each of the three ticks."""
    specs, per_tick = status_specs()
    refs = [make_ref(s) for s in specs]
    for t, frames in enumerate(per_tick):
        assert [r.tick(f)[4] for r, f in zip(refs, frames)] == STATUSES, t


@gpu
def test_status_bits_do_not_leak_between_members():
    pf = _pf()
    specs, per_tick = status_specs()
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    group = pf.FilterGroup(members)
    for t, frames in enumerate(per_tick):
        d = [dev(f) for f in frames]
        assert [int(v) for v in tick_both(group, twins, d, d, f"tick {t}")["status"]] == STATUSES, t
    group.close()


@gpu
def test_limits_of_the_member_count():
    pf = _pf()
    from introtocomputervision_amd._capi import EINVAL, lib
    frames, pos, tex = scene(400, ROWS, COLS, 3, 2)
    specs = [dict(model=tex[:5, :4].copy(), n=8, mode=ref.HIST if k % 3 == 0 else ref.MSE, mse=12.0, ss=2.0, seed=1000 + k)
             for k in range(65)]
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    one = pf.FilterGroup(members[:1])
    full = pf.FilterGroup(members[1:65])
    for t, f in enumerate(frames):
        d = dev(f)
        tick_both(one, twins[:1], d, [d], f"count 1, tick {t}")
        tick_both(full, twins[1:65], d, [d] * 64, f"count 64, tick {t}")
    handles = (C.c_void_p * 65)(*[m._h for m in members])
    h = C.c_void_p()
    assert lib.micv_pf_group_create(handles, 65, C.byref(h)) == EINVAL and not h
    assert lib.micv_pf_group_create(handles, 64, C.byref(h)) == 0 and h
    lib.micv_pf_group_destroy(h)
    one.close()
    full.close()


@gpu
def test_group_ticks_and_single_ticks_interleave():
    pf = _pf()
    frames, pos, tex = scene(500, ROWS, COLS, 3, 3)
    specs = [dict(model=tex[:7, :5].copy(), n=n, mode=mode, mse=8.0, ss=2.0, seed=40 + n) for n, mode in
             [(65, ref.MSE), (64, ref.HIST), (300, ref.MSE)]]
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    group = pf.FilterGroup(members)
    d = [dev(f) for f in frames]
    tick_both(group, twins, d[0], [d[0]] * 3, "group tick 0")
    a, b = members[1].tick(d[1]), twins[1].tick(d[1])  # member 1 alone; the other twins do not tick
    assert pf.ParticleFilter.state_from_device(a).tobytes() == pf.ParticleFilter.state_from_device(b).tobytes()
    same_everywhere(members, twins, "after the single tick")
    tick_both(group, twins, d[2], [d[2]] * 3, "group tick 2")
    group.close()


@gpu
def test_refusals_enqueue_nothing():
    import torch
    pf = _pf()
    from introtocomputervision_amd._capi import EINVAL, lib
    frames, pos, tex = scene(600, ROWS, COLS, 3, 2)
    spec = dict(model=tex[:7, :5].copy(), n=65, mode=ref.MSE, mse=8.0, ss=2.0)
    members = [make(dict(spec, seed=50 + k)) for k in range(3)]
    other_size = make(dict(spec, model=tex[:7, :5].copy()), rows=ROWS, cols=COLS + 1)
    other_channels = make(dict(spec, model=tex[:7, :5, 0].copy()))
    h = C.c_void_p()

    def create(filters):
        handles = (C.c_void_p * max(len(filters), 1))(*[f._h if f is not None else None for f in filters])
        rc = lib.micv_pf_group_create(handles, len(filters), C.byref(h))
        assert rc != 0 or h
        return rc
    for bad in ([members[0], other_size], [members[0], other_channels], [members[0], members[1], members[0]],
                [members[0], None], []):
        assert create(bad) == EINVAL and not h, bad
    for bad in ([], [members[0], other_size]):
        with pytest.raises(Exception):
            pf.FilterGroup(bad)
    group = pf.FilterGroup(members)
    tick = lib.micv_pf_group_tick_dev
    group.tick(dev(frames[0]))
    torch.cuda.synchronize()
    before = [snapshot(m) for m in members]
    d = [dev(frames[1]) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[x.data_ptr() for x in d])
    ok = (C.c_size_t * 3)(COLS * 3, COLS * 3, COLS * 3)
    states = torch.full((3, 5), -7, dtype=torch.int32, device="cuda")
    assert tick(group._h, ptrs, ok, 2, None, states.data_ptr()) == EINVAL  # neither 1 nor count
    assert tick(group._h, ptrs, ok, 0, None, states.data_ptr()) == EINVAL
    assert tick(group._h, ptrs, ok, 4, None, states.data_ptr()) == EINVAL
    assert tick(group._h, (C.c_void_p * 3)(d[0].data_ptr(), None, d[2].data_ptr()), ok, 3, None, states.data_ptr()) == EINVAL
    assert tick(group._h, (C.c_void_p * 1)(None), ok, 1, None, states.data_ptr()) == EINVAL
    assert tick(group._h, ptrs, (C.c_size_t * 3)(COLS * 3, COLS * 3, COLS * 3 - 1), 3, None, states.data_ptr()) == EINVAL
    assert tick(group._h, ptrs, (C.c_size_t * 1)(COLS * 3 - 1), 1, None, states.data_ptr()) == EINVAL
    assert tick(group._h, None, ok, 1, None, states.data_ptr()) == EINVAL and tick(None, ptrs, ok, 1, None, None) == EINVAL
    torch.cuda.synchronize()
    assert (states.cpu().numpy() == -7).all()
    for k, m in enumerate(members):
        for a, b in zip(snapshot(m), before[k]):
            assert np.array_equal(a, b), k
    # and the group goes on as if nothing had been called
    twins = [make(dict(spec, seed=50 + k)) for k in range(3)]
    for t in twins:
        t.tick(dev(frames[0]))
    tick_both(group, twins, d[0], [d[0]] * 3, "after the refusals")
    group.close()


@gpu
def test_states_dev_is_the_only_memory_written():
    import torch
    import _layout as L
    pf = _pf()
    from introtocomputervision_amd._capi import lib
    frames, pos, tex = scene(700, ROWS, COLS, 3, 1)
    specs = [dict(model=tex[:7, :5].copy(), n=n, mode=mode, mse=8.0, ss=2.0, seed=60 + n) for n, mode in
             [(65, ref.MSE), (64, ref.HIST), (9, ref.MSE)]]
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    group = pf.FilterGroup(members)
    s = L.slab([L.Plane("states", shape=(1, 15), dtype=np.int32, dense=True)])
    assert s.ptr("states") % 4 == 0
    d = dev(frames[0])
    ptrs, strides = (C.c_void_p * 1)(d.data_ptr()), (C.c_size_t * 1)(COLS * 3)
    assert lib.micv_pf_group_tick_dev(group._h, ptrs, strides, 1, torch.cuda.current_stream().cuda_stream, s.ptr("states")) == 0
    torch.cuda.synchronize()
    want = np.stack([t.tick(d).cpu().numpy() for t in twins]).reshape(1, 15)
    L.check(s, ["states"], {"states": want}, "micv_pf_group_tick_dev")
    same_everywhere(members, twins, "containment")
    group.close()


def padded_host_frames(frames, pad=8):
    out = []
    for f in frames:
        wide = np.full((f.shape[0], f.shape[1] + pad, 3), 99, np.uint8)
        wide[:, :f.shape[1]] = f
        out.append(wide[:, :f.shape[1]])
    return out


@gpu
def test_sequence_of_host_frames():
    pf = _pf()
    frames, pos, tex = scene(800, ROWS, COLS, 3, 5)
    frames = padded_host_frames(frames)
    assert frames[0].strides[0] == (COLS + 8) * 3
    specs = [dict(model=tex[:7, :5].copy(), n=n, mode=mode, mse=8.0, ss=2.0, seed=70 + n) for n, mode in
             [(65, ref.MSE), (300, ref.HIST), (1, ref.MSE)]]
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    group = pf.FilterGroup(members)
    states, parts = group.track(frames, with_particles=True)
    assert states.shape == (5, 3) and len(parts) == 3
    for k, t in enumerate(twins):
        ws, wp = t.track(frames, with_particles=True)
        assert np.ascontiguousarray(states[:, k]).tobytes() == ws.tobytes(), k
        assert parts[k].shape == wp.shape and np.array_equal(bits(parts[k]), bits(wp)), k
    same_everywhere(members, twins, "after the sequence")
    only = group.track(frames)  # without particles; the filters go on from where they are
    for k, t in enumerate(twins):
        assert np.ascontiguousarray(only[:, k]).tobytes() == t.track(frames).tobytes(), k
    group.close()


@gpu
@pytest.mark.parametrize("all_frames", [False, True])
def test_driver_over_a_group(all_frames):
    pf = _pf()
    from introtocomputervision_amd import ps6
    from introtocomputervision_amd._capi import EINVAL, MicvError
    frames, pos, tex = scene(900, ROWS, COLS, 3, 6)
    kept = [f.copy() for f in frames]
    specs = [dict(model=tex[:7, :5].copy(), n=n, mode=mode, mse=8.0, ss=2.0, seed=80 + n) for n, mode in
             [(65, ref.MSE), (300, ref.HIST), (64, ref.MSE)]]
    sizes = [(5.0, 7.0), (9.5, 6.0), (3.0, 3.0)]
    saves = [{0, 5}, {2}, set()]
    members, twins = [make(s) for s in specs], [make(s) for s in specs]
    group = pf.FilterGroup(members)
    states, pictures = ps6.trackDisplayGroup(group, frames, sizes, saves, allFrames=all_frames)
    assert states.shape == (6, 3)
    painted = 0
    for k, t in enumerate(twins):
        ws, wp = ps6.trackDisplay(t, frames, sizes[k], saves[k], allFrames=all_frames)
        assert np.ascontiguousarray(states[:, k]).tobytes() == ws.tobytes(), k
        assert sorted(pictures[k]) == sorted(wp) == (list(range(6)) if all_frames else sorted(saves[k])), k
        for i in wp:
            assert np.array_equal(pictures[k][i], wp[i]), (k, i)
            painted += int(not np.array_equal(wp[i], frames[i]))
    assert painted >= 3
    assert all(np.array_equal(a, b) for a, b in zip(frames, kept)), "the input frames were changed"
    same_everywhere(members, twins, "after the driver")
    with pytest.raises(MicvError) as e:
        ps6.trackDisplayGroup(group, frames, sizes, [{0}, {6}, set()])
    assert e.value.code == EINVAL
    with pytest.raises(MicvError) as e:
        ps6.trackDisplayGroup(group, frames, sizes, [{0}, {-1}, set()])
    assert e.value.code == EINVAL
    same_everywhere(members, twins, "after the refused calls")
    group.close()


@gpu
def test_run_problems_equals_the_three_run_problem_functions(monkeypatch):
    from introtocomputervision_amd import ps6
    rows, cols, nframes = 48, 64, 8
    rng = np.random.default_rng(1000)
    bg = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    head, hand = rng.integers(0, 256, (13, 10, 3), dtype=np.uint8), rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    clean, noisy = [], []
    for t in range(nframes):
        f = bg.copy()
        f[17 + t:30 + t, 32 + t:42 + t] = head
        f[38 - t // 2:47 - t // 2, 54 - t:61 - t] = hand
        clean.append(f)
        noisy.append(np.clip(f.astype(np.int16) + rng.integers(-20, 21, f.shape, dtype=np.int16), 0, 255).astype(np.uint8))
    # the reference's boxes (pres_debate.txt, Solution.cpp:144-145) scaled by a tenth; its configurations with fewer
    # particles and the sigmas scaled likewise
    bboxes = {"pres_debate": ((32.0, 17.0), (10.0, 13.0)), "noisy_debate": ((32.0, 17.0), (10.0, 13.0)),
              "hand": ((54.0, 38.0), (7.0, 9.0))}
    conf = lambda n, mse, dyn, alpha: dict(num_particles=str(n), mse_sigma=str(mse), dynamics_sigma=str(dyn), alpha=str(alpha))
    cfg = {"pfconf1": conf(60, 3, 1.5, 0.1), "pfconf1_noisy": conf(60, 3, 1.5, 0.1), "pfconf2": conf(130, 1.5, 2.8, 0.15),
           "pfconf2_noisy": conf(130, 1.5, 2.6, 0.15), "pfconf3_head": conf(65, 0, 1.2, 0.15), "pfconf3_hand": conf(64, 0, 2.8, 0.15)}
    monkeypatch.setattr(ps6, "HAND_BBOX", bboxes["hand"][0])
    monkeypatch.setattr(ps6, "HAND_SIZE", bboxes["hand"][1])
    for name, save in (("SAVE_1A", (1, 5, 144)), ("SAVE_1E", (0, 3, 46)), ("SAVE_2A", (2, 7, 150)), ("SAVE_2B", (2, 7, 150)),
                       ("SAVE_3A", (1, 5, 144)), ("SAVE_3B", (4, 6, 140))):
        monkeypatch.setattr(ps6, name, save)  # save sets that an 8-frame sequence reaches (and one index it does not)
    want = {}
    want.update(ps6.runProblem1(clean, noisy, cfg, bboxes))
    want.update(ps6.runProblem2(clean, noisy, cfg, bboxes))
    want.update(ps6.runProblem3(clean, noisy, cfg, bboxes))
    got = ps6.runProblems(clean, noisy, cfg, bboxes)
    assert list(got) == ["ps6-1-a", "ps6-1-e", "ps6-2-a", "ps6-2-b", "ps6-3-a", "ps6-3-b"] and sorted(want) == sorted(got)
    for key in want:
        (ws, wp), (gs, gp) = want[key], got[key]
        assert gs.dtype == ws.dtype and gs.shape == ws.shape == (nframes,) and gs.tobytes() == ws.tobytes(), key
        assert sorted(gp) == sorted(wp) and len(wp) == 2, key
        for i in wp:
            assert np.array_equal(gp[i], wp[i]) and not np.array_equal(wp[i], (noisy if key in ("ps6-1-e", "ps6-2-b") else clean)[i]), (key, i)
