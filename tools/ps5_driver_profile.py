#!/usr/bin/env python3
"""Times the ps5 driver on one MI355X and writes profiles/ps5_driver/ps5_driver_bench.jsonl, at 480x640 and 1080p:

  arrows    the arrow launch (ps5.drawVelocityVectors in place) beside a device copy of the image, the floor;
  display   ps5.denseLKDisplay (pyramidal, window 15, 4 levels) against what the library offered before for the same
            outputs: grey conversion + the chain, a download of u and v, micv_viz's host loops on one thread
            (tools/probes/ps5_host_loops.cpp, timed apart: no device involved), and the JET batch on the device;
  montage   ps5.pyramidMontage of four f32 levels against the download of the levels + the host loops;
  sequence  ps5.warpDiffSequence (4 frames at pyramid level 1, window 15) against the separate calls
            (lk.calcOpticalFlow, lk.warp, a subtraction, display.normalizeMinMax per pair).

Every shape is warmed first; device times are events around `--reps` back-to-back calls on one stream (per-call Python
included), the median of five rounds with the sides alternating; host-clocked times end in a synchronise.
No GPU: exits with an error, nothing is estimated.

    python tools/ps5_driver_profile.py --reps 20
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
PROBE_SRC = os.path.join(ROOT, "tools", "probes", "ps5_host_loops.cpp")
PROBE_BIN = os.path.join(ROOT, "tools", "probes", "_bin", "ps5_host_loops")


def probe(what, rows, cols, reps):
    lib = os.path.join(ROOT, "introtocomputervision_amd")
    if not os.path.exists(PROBE_BIN):
        os.makedirs(os.path.dirname(PROBE_BIN), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", PROBE_SRC, "-o", PROBE_BIN, "-L" + lib, "-lmicv", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([PROBE_BIN, what, str(rows), str(cols), str(reps)], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps5_driver", "ps5_driver_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("ps5_driver_profile: no GPU")
    from introtocomputervision_amd import display, lk, ps5, pyr, synth

    rows_out = []

    def emit(**kw):
        rows_out.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def wall(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    def alternate(forms, reps, clock=timed, rounds=5):
        for fn in forms.values():
            fn()
            fn()
        torch.cuda.synchronize()
        got = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                got[k].append(clock(fn, reps))
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}

    for name, rows, cols in [("480x640", 480, 640), ("1080p", 1080, 1920)]:
        prev, nxt = synth.lk_pair(0x5EED0005, rows, cols, dx=3, dy=-2)
        p8, n8 = np.clip(prev, 0, 255).astype(np.uint8), np.clip(nxt, 0, 255).astype(np.uint8)
        dp, dn = torch.from_numpy(p8).cuda(), torch.from_numpy(n8).cuda()
        u, v, arrows, ju, jv = ps5.denseLKDisplay(dp, dn, mode="pyramidal", winSize=15, levels=4)
        canvas, spare = ps5.toBGR8(dp), torch.empty_like(arrows)
        res = alternate({"copy_bgr8": lambda: spare.copy_(canvas),
                         "arrows": lambda: ps5.drawVelocityVectors(canvas, u, v, inplace=True)}, args.reps)
        for form, (med, lo, hi) in res.items():
            emit(case="arrows", size=name, form=form, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))

        uv_host = [np.empty((rows, cols), np.float32), np.empty((rows, cols), np.float32)]

        def before_device_part():  # conversion + chain, the download the host loops need, the JET batch
            gp, gn = pyr.toGray(dp), pyr.toGray(dn)
            uu, vv = lk.calcOpticalFlowPyr(gp, gn, 15, 4)
            uv_host[0][:] = uu.cpu().numpy()
            uv_host[1][:] = vv.cpu().numpy()
            display.normalizeMinMax(torch.stack([uu, vv]), jet=True)

        res = alternate({"dense_lk_display": lambda: ps5.denseLKDisplay(dp, dn, mode="pyramidal", winSize=15, levels=4),
                         "before_device_part": before_device_part}, max(1, args.reps // 2), clock=wall)
        host = probe("arrows", rows, cols, 9)
        for form, (med, lo, hi) in res.items():
            emit(case="display", size=name, form=form, clock="host, synchronised", ms=round(med, 4), ms_min=round(lo, 4),
                 ms_max=round(hi, 4))
        emit(case="display", size=name, form="before_host_loops_arrows_one_thread", ms=host["ms_median"], ms_min=host["ms_min"])

        levels = pyr.makeGaussianPyramid(pyr.toGray(dp), 4)
        res = alternate({"montage": lambda: ps5.pyramidMontage(levels),
                         "download_levels": lambda: [a.cpu() for a in levels]}, args.reps, clock=wall)
        host = probe("montage", rows, cols, 9)
        for form, (med, lo, hi) in res.items():
            emit(case="montage", size=name, form=form, clock="host, synchronised", ms=round(med, 4), ms_min=round(lo, 4),
                 ms_max=round(hi, 4))
        emit(case="montage", size=name, form="before_host_loops_one_thread", ms=host["ms_median"], ms_min=host["ms_min"])

        seq = [synth.lk_pair(0x5EED0005 + t, rows, cols, dx=1 + t, dy=-1)[0] for t in range(4)]
        frames = torch.stack([pyr.makeGaussianPyramid(torch.from_numpy(f).cuda(), 2)[1] for f in seq])

        def separate():
            out = []
            for p in range(3):
                fu, fv = lk.calcOpticalFlow(frames[p], frames[p + 1], 15)
                out.append(display.normalizeMinMax(frames[p] - lk.warp(frames[p + 1], fu, fv)))
            return out

        res = alternate({"warp_diff_sequence": lambda: ps5.warpDiffSequence(frames, winSize=15), "separate_calls": separate},
                        max(1, args.reps // 2))
        for form, (med, lo, hi) in res.items():
            emit(case="sequence", size=name, level_size=list(frames.shape[1:]), pairs=3, form=form, ms=round(med, 4),
                 ms_min=round(lo, 4), ms_max=round(hi, 4))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows_out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
