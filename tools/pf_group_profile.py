"""Time a group of particle filters ticked together (micv_pf_group, csrc/pf.hip) against the same filters ticked one by one,
in the same process and the same build, on 480 x 640 x 3 synthetic frames with the head model (129 x 104) and the hand model
(87 x 73) and the particle counts of ps6.yaml (300 / 700).  Three comparisons, one JSON line per row:
  tick      micv_pf_group_tick_dev against the loop of micv_pf_tick_dev on one stream, frames on the device, per member and
            tick: K = 1, 2, 4, 6, 16, 64 of one kind, and the six filters of ps6 (K = 6), with one shared frame and with a
            frame per member;
  sequence  micv_pf_group_track_seq_host against K calls of micv_pf_track_seq_host, per frame of the video;
  problems  ps6.runProblems against runProblem1 + runProblem2 + runProblem3.
Clock: time.perf_counter around a synchronised window of --window calls (sequence / problems: one call), the median of
--repeats windows after one warm-up window; the two sides of a row alternate window by window.  The calls go through
ctypes with everything allocated beforehand.  Reads nothing but its own frames.
    python tools/pf_group_profile.py [--window 50] [--repeats 9] [--out profiles/pf_group/profile.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD, HAND = (129, 104), (87, 73)
HEAD_AT, HAND_AT = (320.0, 175.0), (540.0, 385.0)  # (x, y) of the boxes' top-left corners


def video(seed, count, noise=0):
    """A head and a hand texture moving over a textured background -> (frames, head texture, hand texture)."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    head = rng.integers(0, 256, HEAD + (3,), dtype=np.uint8)
    hand = rng.integers(0, 256, HAND + (3,), dtype=np.uint8)
    out = []
    for t in range(count):
        f = bg.copy()
        y, x = 175 + (t % 40), 320 + 2 * (t % 40)
        f[y:y + HEAD[0], x:x + HEAD[1]] = head
        y, x = 385 - (t % 40) // 2, 540 - (t % 40)
        f[y:y + HAND[0], x:x + HAND[1]] = hand
        if noise:
            f = np.clip(f.astype(np.int16) + rng.integers(-noise, noise + 1, f.shape, dtype=np.int16), 0, 255).astype(np.uint8)
        out.append(f)
    return out, head, hand


def median_windows(sides, repeats, sync):
    """sides: {name: callable running one window}.  One warm-up window each, then `repeats` rounds in which the sides
    alternate -> {name: (median seconds, [every window])}."""
    for fn in sides.values():
        fn()
        sync()
    times = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pf_group", "profile.jsonl"))
    a = ap.parse_args()
    import torch
    from introtocomputervision_amd import config, pf, ps6
    from introtocomputervision_amd._capi import check, lib
    frames, head, hand = video(7, a.frames)
    noisy = video(7, a.frames, noise=20)[0]
    dframes = [torch.from_numpy(f).cuda() for f in frames]
    stream = torch.cuda.current_stream().cuda_stream
    sync = torch.cuda.synchronize
    kinds = {"head_mse": (head, HEAD_AT, pf.MEAN_SQ_ERR, 300, 3.0, 6.5), "hand_mse": (hand, HAND_AT, pf.MEAN_SQ_ERR, 700, 1.5, 28.0),
             "head_hist": (head, HEAD_AT, pf.MEAN_SHIFT_LT, 300, 0.0, 4.7), "hand_hist": (hand, HAND_AT, pf.MEAN_SHIFT_LT, 700, 0.0, 28.0)}
    ps6_mix = ["head_mse", "hand_mse", "head_hist", "hand_hist", "head_mse", "hand_mse"]

    def make(kind, seed):
        tex, at, mode, n, mse, dyn = kinds[kind]
        return pf.ParticleFilter(tex, (640, 480), n, mode, mse, dyn, at, alpha=0.1, seed=seed)

    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def per_tick_row(label, names, per_member_frames):
        k = len(names)
        members = [make(kind, 1 + i) for i, kind in enumerate(names)]
        group = pf.FilterGroup(members)
        states = torch.empty((k, 5), dtype=torch.int32, device="cuda")
        nf = k if per_member_frames else 1
        # frame arguments of every call of a window, built beforehand
        gargs, largs = [], []
        for t in range(a.window):
            fr = [dframes[(t + i) % len(dframes)] for i in range(nf)]
            gargs.append(((C.c_void_p * nf)(*[f.data_ptr() for f in fr]), (C.c_size_t * nf)(*[640 * 3] * nf)))
            largs.append([fr[i if per_member_frames else 0].data_ptr() for i in range(k)])

        def run_group():
            for p, s in gargs:
                check(lib.micv_pf_group_tick_dev(group._h, p, s, nf, stream, states.data_ptr()))

        def run_loop():
            for ptrs in largs:
                for i, m in enumerate(members):
                    check(lib.micv_pf_tick_dev(m._h, ptrs[i], 640 * 3, stream, states.data_ptr() + 20 * i))
        res = median_windows({"group": run_group, "loop": run_loop}, a.repeats, sync)
        us = {s: res[s][0] * 1e6 / (a.window * k) for s in res}
        emit({"compare": "tick", "members": label, "K": k, "frames": "per member" if per_member_frames else "shared",
              "group_us_per_member_tick": round(us["group"], 2), "loop_us_per_member_tick": round(us["loop"], 2),
              "loop_over_group": round(us["loop"] / us["group"], 3),
              "group_window_ms": [round(v * 1e3, 3) for v in res["group"][1]], "loop_window_ms": [round(v * 1e3, 3) for v in res["loop"][1]]})
        group.close()
        for m in members:
            m.close()

    for kind in ("head_mse", "hand_hist"):
        for k in (1, 2, 4, 6, 16, 64):
            for own in (False, True):
                per_tick_row(kind, [kind] * k, own)
    for own in (False, True):
        per_tick_row("ps6 mix", ps6_mix, own)

    def sequence_row(label, names):
        k = len(names)
        members = [make(kind, 1 + i) for i, kind in enumerate(names)]
        group = pf.FilterGroup(members)
        res = median_windows({"group": lambda: group.track(frames), "loop": lambda: [m.track(frames) for m in members]}, a.repeats, sync)
        ms = {s: res[s][0] * 1e3 / len(frames) for s in res}
        emit({"compare": "sequence", "members": label, "K": k, "nframes": len(frames), "group_ms_per_frame": round(ms["group"], 4),
              "loop_ms_per_frame": round(ms["loop"], 4), "loop_over_group": round(ms["loop"] / ms["group"], 3)})
        group.close()
        for m in members:
            m.close()

    for k in (1, 2, 4, 6):
        sequence_row("head_mse", ["head_mse"] * k)
    sequence_row("ps6 mix", ps6_mix)

    cfg = config.load(os.path.join(ROOT, "tests", "golden", "ps6", "ps6.yaml"))
    box = (HEAD_AT, (float(HEAD[1]), float(HEAD[0])))
    bboxes = {"pres_debate": box, "noisy_debate": box}
    saves = dict(SAVE_1A=(8, 24, 39), SAVE_1E=(4, 12, 30), SAVE_2A=(5, 15, 35), SAVE_2B=(5, 15, 35), SAVE_3A=(8, 24, 39), SAVE_3B=(5, 15, 30))
    for name, v in saves.items():  # the reference's three pictures per run, at indices a 40-frame video reaches
        setattr(ps6, name, v)

    def three():
        out = {}
        for fn in (ps6.runProblem1, ps6.runProblem2, ps6.runProblem3):
            out.update(fn(frames, noisy, cfg, bboxes))
        return out
    x, y = three(), ps6.runProblems(frames, noisy, cfg, bboxes)
    equal = all(x[key][0].tobytes() == y[key][0].tobytes() and all(np.array_equal(x[key][1][i], y[key][1][i]) for i in x[key][1]) for key in x)
    res = median_windows({"group": lambda: ps6.runProblems(frames, noisy, cfg, bboxes), "loop": three}, a.repeats, sync)
    emit({"compare": "problems", "nframes": len(frames), "equal": bool(equal), "runProblems_ms": round(res["group"][0] * 1e3, 3),
          "runProblem1_2_3_ms": round(res["loop"][0] * 1e3, 3), "loop_over_group": round(res["loop"][0] / res["group"][0], 3)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
