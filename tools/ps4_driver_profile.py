#!/usr/bin/env python3
"""Times the ps4 driver on one MI355X at 480x640 with config/ps4.yaml's Harris parameters and writes
profiles/ps4_driver/ps4_driver_bench.jsonl:

  overlay   the launches of ps4.drawKeypoints and ps4.drawMatchLines on a 480 x 1280 canvas beside a device copy of that
            canvas, the floor; and the colour prologue alone (one lane walking 3 n steps), as the difference between a
            call with the chain's count and one with count 0;
  harris    ps4.harrisDisplay against the parent's way to the same three files: harris.cornersFromImage on the device,
            the downloads of gx, gy, R and the corner map, then the host loops of shim/micv_ps4.hpp on one thread
            (tools/probes/ps4_host_loops.cpp, timed apart: no device involved);
  panels    ps4.matchPanels against the parent's way: the downloads of both keypoint lists, the match list and the three
            counts, then the host loops.

Every shape is warmed first; device times are events around `--reps` back-to-back calls on one stream (per-call Python
included), the median of five rounds with the sides alternating; host-clocked times end in a synchronise.
No GPU: exits with an error, nothing is estimated.

    python tools/ps4_driver_profile.py --reps 20
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
PROBE_SRC = os.path.join(ROOT, "tools", "probes", "ps4_host_loops.cpp")
PROBE_BIN = os.path.join(ROOT, "tools", "probes", "_bin", "ps4_host_loops")


def probe(rows, cols, keypoints, matches, reps):
    if not os.path.exists(PROBE_BIN):
        os.makedirs(os.path.dirname(PROBE_BIN), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", PROBE_SRC, "-o", PROBE_BIN], check=True)
    out = subprocess.run([PROBE_BIN, str(rows), str(cols), str(max(keypoints, 1)), str(matches), str(reps)], check=True,
                         capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps4_driver", "ps4_driver_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("ps4_driver_profile: no GPU")
    from introtocomputervision_amd import config, harris, ps4, synth

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

    def report(case, res, **extra):
        for form, (med, lo, hi) in res.items():
            emit(case=case, size="480x640", form=form, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), **extra)

    rows, cols = 480, 640
    params = config.harris_params(config.load(os.path.join(ROOT, "tests", "golden", "config", "ps4.yaml")), "harris_trans")
    a = np.clip(synth.checkerboard(rows, cols, seed=0x5EED0004), 0, 255).astype(np.uint8)
    b = np.ascontiguousarray(np.roll(a, (7, 11), axis=(0, 1)))
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    cap = 4096
    p = ps4.runProblem2(da, db, params, capacity=cap)
    na, nb, nm = int(p["a"]["count"].item()), int(p["b"]["count"].item()), int(p["match_count"].item())
    emit(case="chain", size="480x640", corners_a=na, corners_b=nb, matches=nm, capacity=cap)
    kpa, kpb, m = p["kp_a"], p["kp_b"], p["matches"]
    ca, cb, cm = p["a"]["count"], p["b"]["count"], p["match_count"]
    zero = torch.zeros_like(ca)

    canvas = p["keypoints_panel"].clone()
    spare = torch.empty_like(canvas)
    state = ps4.rngState(canvas)
    res = alternate({
        "copy_canvas": lambda: spare.copy_(canvas),
        "keypoints_a": lambda: ps4.drawKeypoints(None, kpa, count=ca, rng_state=state, canvas=canvas[:, :cols], x0=0),
        "keypoints_a_count0": lambda: ps4.drawKeypoints(None, kpa, count=zero, rng_state=state, canvas=canvas[:, :cols], x0=0),
        "match_lines": lambda: ps4.drawMatchLines(canvas, kpa, kpb, m, count=cm, x_offset=cols),
        "match_lines_count0": lambda: ps4.drawMatchLines(canvas, kpa, kpb, m, count=zero, x_offset=cols),
    }, args.reps)
    report("overlay", res, strokes_a=na, lines=nm)

    f = da.to(torch.float32)
    hp = (params["sobel_kernel_size"], params["window_size"], params["gaussian_sigma"], params["alpha"], params["response_threshold"],
          params["min_distance"])

    def parent_harris():  # the chain, then what the host loops need
        d = harris.cornersFromImage(f, *hp, capacity=cap, want_response=True, want_corners=True, lazy=True)
        return [d[k].cpu() for k in ("gx", "gy", "response", "corners")]

    res = alternate({"harris_display": lambda: ps4.harrisDisplay(f, *hp, capacity=cap), "parent_device_part": parent_harris},
                    max(1, args.reps // 2), clock=wall)
    report("harris", res, clock="host, synchronised")

    def parent_panels():  # the lists and the counts the host loops need
        return [t.cpu() for t in (kpa, kpb, m, ca, cb, cm)]

    res = alternate({"match_panels": lambda: ps4.matchPanels(da, db, kpa, kpb, m, ca, cb, cm), "parent_device_part": parent_panels},
                    max(1, args.reps // 2), clock=wall)
    report("panels", res, clock="host, synchronised")

    host = probe(rows, cols, max(na, nb), nm, 9)
    emit(case="harris", size="480x640", form="parent_host_loops_one_thread", ms=host["dots_ms"],
         note="drawDots alone; the two normalisations of the gradient panel and of R come on top")
    emit(case="panels", size="480x640", form="parent_host_loops_one_thread", ms=round(host["keypoint_panel_ms"] + host["match_panel_ms"], 4),
         keypoint_panel_ms=host["keypoint_panel_ms"], match_panel_ms=host["match_panel_ms"], keypoints=host["keypoints"], matches=host["matches"])

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows_out:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
