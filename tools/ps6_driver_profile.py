#!/usr/bin/env python3
"""Times the ps6 driver on one MI355X at 720 x 1280 x 3 with 300 and with 700 particles (ps6.yaml's pfconf1 and pfconf2)
and writes profiles/ps6_driver/ps6_driver_bench.jsonl.  Per frame of a 32-frame host sequence:

  track_display_seq      micv_ps6_track_display_seq_host keeping three frames (the driver's saveFrames);
  track_display_seq_all  the same keeping every frame (what the driver hands to the video writer);
  track_seq              micv_pf_track_seq_host: the states alone, the floor;
  parent_device_part     the parent commit's way to the driver's output: micv_pf_tick_host + micv_pf_particles_host per
                         frame; its host loops (clone, dots, ring on one thread: tools/probes/ps6_host_loops.cpp, no
                         device involved) are timed apart and come on top for every frame.

Every form is warmed first; times are a host clock around whole calls that end synchronised, the median of five rounds with
the forms alternating.  No GPU: exits with an error, nothing is estimated.

    python tools/ps6_driver_profile.py --frames 32
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROBE_SRC = os.path.join(ROOT, "tools", "probes", "ps6_host_loops.cpp")
PROBE_BIN = os.path.join(ROOT, "tools", "probes", "_bin", "ps6_host_loops")


def probe(rows, cols, n, reps):
    if not os.path.exists(PROBE_BIN):
        os.makedirs(os.path.dirname(PROBE_BIN), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", PROBE_SRC, "-o", PROBE_BIN], check=True)
    out = subprocess.run([PROBE_BIN, "time", str(rows), str(cols), str(n), str(reps)], check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def sequence(rows, cols, nframes, obj=(87, 73)):
    rng = np.random.default_rng(606)
    bg = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    tex = rng.integers(0, 256, (obj[0], obj[1], 3), dtype=np.uint8)
    frames, y, x = [], rows // 3, cols // 3
    for t in range(nframes):
        f = bg.copy()
        f[y + t:y + t + obj[0], x + 2 * t:x + 2 * t + obj[1]] = tex
        frames.append(f)
    return frames, tex, (float(x), float(y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps6_driver", "ps6_driver_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("ps6_driver_profile: no GPU")
    from introtocomputervision_amd import pf, ps6

    rows, cols = 720, 1280
    frames, tex, init = sequence(rows, cols, args.frames)
    size = (float(tex.shape[1]), float(tex.shape[0]))
    save = (5, 15, 25)
    out_rows = []

    def emit(**kw):
        out_rows.append(kw)
        print(json.dumps(kw), flush=True)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / len(frames)

    for n, sigma, dyn in ((300, 3.0, 6.5), (700, 1.5, 28.0)):
        def filt():
            return pf.ParticleFilter(tex, (cols, rows), n, pf.MEAN_SQ_ERR, sigma, dyn, init)

        f_seq, f_all, f_plain, f_parent = filt(), filt(), filt(), filt()

        def parent():
            for f in frames:
                f_parent.tick(f)
                f_parent.getParticles()

        forms = {
            "track_display_seq": lambda: ps6.trackDisplay(f_seq, frames, size, save),
            "track_display_seq_all": lambda: ps6.trackDisplay(f_all, frames, size, (), True),
            "track_seq": lambda: f_plain.track(frames),
            "parent_device_part": parent,
        }
        for fn in forms.values():
            fn()
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(wall(fn))
        for k, v in got.items():
            emit(case="sequence", size=f"{rows}x{cols}x3", particles=n, frames=len(frames), form=k, ms_per_frame=round(float(np.median(v)), 4),
                 ms_min=round(min(v), 4), ms_max=round(max(v), 4), kept=len(save) if k == "track_display_seq" else (len(frames) if k.endswith("all") else 0),
                 clock="host, whole call, synchronised")
        host = probe(rows, cols, n, 50)
        emit(case="sequence", size=f"{rows}x{cols}x3", particles=n, form="parent_host_loops_one_thread", ms_per_frame=round(host["host_loops_ms_per_frame"], 4),
             note="clone + dots + ring per frame on the profiling host's CPU; comes on top of parent_device_part")

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in out_rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
