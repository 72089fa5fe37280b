#!/usr/bin/env python3
"""Times disparityNCorr on 8-bit images (micv_disparity_ncorr_u8_*) beside the parent commit's way of doing the same thing --
micv_disparity_ncorr_* on float copies of the images, looped for a batch -- on one MI355X, and writes
profiles/stereo_ncc_u8/stereo_ncc_u8_bench.jsonl.

  ps2      511 x 640, radius 7, [-95, 0], COLS_2R (cuda::disparityNCorr as written)
  C3       1080 x 1920, radius 5, [-127, 0], flags 0
  forms    f32_dev, f32_loop_8 (eight f32 calls back to back: the yardstick), u8_dev, u8_batch_8, u8_batch_27, u8_host, f32_host

Every form is warmed first; times are a host clock around `--calls` calls that end in a synchronise, the median of five
rounds with the forms alternating: enqueue plus execution of back-to-back calls, not kernel times, divided by the pairs a
call searches.  The entry points are called directly on buffers allocated once.  No GPU: exits with an error, nothing is
estimated.

    python tools/stereo_ncc_u8_profile.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("ps2", 511, 640, 7, -95, 0, 1), ("C3", 1080, 1920, 5, -127, 0, 0))
BATCHES = (8, 27)
LOOP = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_ncc_u8", "stereo_ncc_u8_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("stereo_ncc_u8_profile: no GPU")
    from introtocomputervision_amd import synth
    from introtocomputervision_amd._capi import check, lib
    from introtocomputervision_amd.lk import _ctx_for

    out_rows = []

    def emit(**kw):
        out_rows.append(kw)
        print(json.dumps(kw), flush=True)

    def wall(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / calls

    for case, rows, cols, rad, lo, hi, flags in CASES:
        nmax = max(BATCHES)
        # (eight distinct pairs, repeated to fill the larger batch: the search has no data-dependent exit)
        pairs = [synth.stereo_pair(0x5EED0F20 + i, rows, cols)[:2] for i in range(LOOP)]
        q = lambda a: np.clip(np.round(a), 0, 255).astype(np.uint8)  # noqa: E731
        l8, r8 = (np.stack([q(pairs[i % LOOP][k]) for i in range(nmax)]) for k in (0, 1))
        lf, rf = l8[:LOOP].astype(np.float32), r8[:LOOP].astype(np.float32)
        d8l, d8r, dfl, dfr = (torch.from_numpy(a).cuda() for a in (l8, r8, lf, rf))
        disp = torch.empty((nmax, rows, cols), dtype=torch.int8, device="cuda")
        hdisp = np.empty((rows, cols), np.int8)
        h, s = _ctx_for(d8l, None).handle, torch.cuda.current_stream().cuda_stream
        n, tail = rows * cols, (rows, cols, rad, lo, hi, flags)

        def u8_dev(i=0):
            check(lib.micv_disparity_ncorr_u8_dev(h, d8l[i].data_ptr(), cols, d8r[i].data_ptr(), cols, *tail, disp[i].data_ptr(), cols, s))

        def f32_dev(i=0):
            check(lib.micv_disparity_ncorr_dev(h, dfl[i].data_ptr(), dfr[i].data_ptr(), rows, cols, cols * 4, rad, lo, hi, flags,
                                               disp[i].data_ptr(), cols, s))

        def u8_host():
            check(lib.micv_disparity_ncorr_u8_host(h, l8[0].ctypes.data, cols, r8[0].ctypes.data, cols, *tail, hdisp.ctypes.data, cols))

        def f32_host():
            check(lib.micv_disparity_ncorr_host(h, lf[0].ctypes.data, rf[0].ctypes.data, rows, cols, cols * 4, rad, lo, hi, flags,
                                                hdisp.ctypes.data, cols))

        def u8_batch(b):
            check(lib.micv_disparity_ncorr_u8_batch_dev(h, d8l.data_ptr(), n, cols, d8r.data_ptr(), n, cols, b, *tail, disp.data_ptr(), n, cols, s))

        def f32_loop():
            for i in range(LOOP):
                f32_dev(i)

        forms = {"f32_dev": (f32_dev, 1), f"f32_loop_{LOOP}": (f32_loop, LOOP), "u8_dev": (u8_dev, 1)}
        for b in BATCHES:
            forms[f"u8_batch_{b}"] = (lambda b=b: u8_batch(b), b)
        forms["u8_host"], forms["f32_host"] = (u8_host, 1), (f32_host, 1)
        for fn, _ in forms.values():
            fn()
        torch.cuda.synchronize()
        # the batch against the loop of f32 calls, before anything is timed
        u8_batch(LOOP)
        a = disp[:LOOP].clone()
        f32_loop()
        if not torch.equal(a, disp[:LOOP]):
            sys.exit(f"stereo_ncc_u8_profile: {case}: the u8 batch differs from the f32 calls")
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, (fn, b) in forms.items():
                got[k].append(wall(fn, args.calls) / b)
        for k, v in got.items():
            emit(case=case, size=f"{rows}x{cols}", radius=rad, disparities=[lo, hi], flags=flags, form=k, pairs_per_call=forms[k][1],
                 calls_per_window=args.calls, ms_per_pair=round(float(np.median(v)), 4), ms_min=round(min(v), 4),
                 ms_max=round(max(v), 4), clock="host, synchronised after the calls")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in out_rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
