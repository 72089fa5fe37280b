#!/usr/bin/env python3
"""Times disparitySSD on 8-bit images (micv_disparity_ssd_u8_*) beside the parent commit's way of doing the same thing --
micv_disparity_ssd_* on float copies of the images, looped for a batch -- on one MI355X, and writes
profiles/stereo_u8/stereo_u8_bench.jsonl.

  C3       1080 x 1920, radius 5, [-127, 0], flags 0:                        u8_dev, f32_dev, u8_host, f32_host
  ps2      511 x 640, radius 7, [-95, 0], COLS_2R | MIN_SSD_5E6 (as written): the same four, u8_batch of 4 / 8 / 16 pairs and
           f32_loop of as many f32 calls back to back (both per pair)

Every form is warmed first; times are a host clock around `--calls` calls that end in a synchronise, the median of five
rounds with the forms alternating: enqueue plus execution of back-to-back calls, not kernel times.  The entry points are
called directly on buffers allocated once.  No GPU: exits with an error, nothing is estimated.

    python tools/stereo_u8_profile.py
    rocprofv3 --kernel-trace --stats -d <dir> -o u8 --output-format csv -- python tools/stereo_u8_profile.py --trace
    python tools/stereo_u8_profile.py --by-grid <dir>/.../u8_kernel_trace.csv     # device time per (kernel, grid)

--trace issues every device form twenty times and measures nothing: the per-kernel split (the u8 pre-pass beside the f32
one, the search of a batch beside the single searches) comes from the trace, never combined with counters.
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("C3", 1080, 1920, 5, -127, 0, 0, ()), ("ps2", 511, 640, 7, -95, 0, 3, (4, 8, 16)))


def by_grid(path):
    """Device time per (kernel, grid in work-items) of a rocprofv3 kernel trace, microseconds.  Searches of different
    numbers of pairs can have the same grid (the tiling trades pairs for columns per wave), so a search launch is also
    keyed by the strips of the pre-pass launched in front of it (its grid's y = pairs x strips per pair)."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    groups, strips = {}, 0
    for row in rows:
        name = re.sub(r"^void (micv::)?(\(anonymous namespace\)::)?", "", row["Kernel_Name"]).split("(")[0]
        if name.startswith("stereo_prep"):
            strips = int(row["Grid_Size_Y"])
        key = (name, int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]), int(row["Grid_Size_Z"]),
               strips if name.startswith("stereo_exact_kernel") else 0)
        groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    print("# device time per (kernel, grid in work-items[, strips of the pre-pass in front of a search]), microseconds")
    for (name, gx, gy, gz, st), v in sorted(groups.items(), key=lambda kv: -float(np.median(kv[1])) * len(kv[1])):
        tag = f"  strips {st:>5}" if st else " " * 14
        print(f"{name:<40} grid {gx:>8} x {gy:>5} x {gz:>3}{tag}  calls {len(v):>4}  median {np.median(v):>8.2f}  min {min(v):>8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--by-grid", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_u8", "stereo_u8_bench.jsonl"))
    args = ap.parse_args()
    if args.by_grid:
        return by_grid(args.by_grid)

    import torch
    if not torch.cuda.is_available():
        sys.exit("stereo_u8_profile: no GPU")
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

    for case, rows, cols, rad, lo, hi, flags, batches in CASES:
        nmax = max(batches, default=1)
        pairs = [synth.stereo_pair(0x5EED0F20 + i, rows, cols)[:2] for i in range(nmax)]
        q = lambda a: np.clip(np.round(a), 0, 255).astype(np.uint8)  # noqa: E731
        l8, r8 = np.stack([q(p[0]) for p in pairs]), np.stack([q(p[1]) for p in pairs])
        lf, rf = l8.astype(np.float32), r8.astype(np.float32)
        d8l, d8r, dfl, dfr = (torch.from_numpy(a).cuda() for a in (l8, r8, lf, rf))
        disp = torch.empty((nmax, rows, cols), dtype=torch.int8, device="cuda")
        hdisp = np.empty((rows, cols), np.int8)
        h, s = _ctx_for(d8l, None).handle, torch.cuda.current_stream().cuda_stream
        n, tail = rows * cols, (rows, cols, rad, lo, hi, flags)

        def u8_dev(i=0):
            check(lib.micv_disparity_ssd_u8_dev(h, d8l[i].data_ptr(), cols, d8r[i].data_ptr(), cols, *tail, disp[i].data_ptr(), cols, s))

        def f32_dev(i=0):
            check(lib.micv_disparity_ssd_dev(h, dfl[i].data_ptr(), dfr[i].data_ptr(), rows, cols, cols * 4, rad, lo, hi, flags,
                                             disp[i].data_ptr(), cols, s))

        def u8_host():
            check(lib.micv_disparity_ssd_u8_host(h, l8[0].ctypes.data, cols, r8[0].ctypes.data, cols, *tail, hdisp.ctypes.data, cols))

        def f32_host():
            check(lib.micv_disparity_ssd_host(h, lf[0].ctypes.data, rf[0].ctypes.data, rows, cols, cols * 4, rad, lo, hi, flags,
                                              hdisp.ctypes.data, cols))

        def u8_batch(b):
            check(lib.micv_disparity_ssd_u8_batch_dev(h, d8l.data_ptr(), n, cols, d8r.data_ptr(), n, cols, b, *tail, disp.data_ptr(), n, cols, s))

        def f32_loop(b):
            for i in range(b):
                f32_dev(i)

        forms = {"u8_dev": (u8_dev, 1), "f32_dev": (f32_dev, 1)}
        for b in batches:
            forms[f"u8_batch_{b}"] = (lambda b=b: u8_batch(b), b)
            forms[f"f32_loop_{b}"] = (lambda b=b: f32_loop(b), b)
        if args.trace:
            for fn, _ in forms.values():
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
            continue
        forms["u8_host"], forms["f32_host"] = (u8_host, 1), (f32_host, 1)
        for fn, _ in forms.values():
            fn()
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, (fn, b) in forms.items():
                got[k].append(wall(fn, max(1, args.calls // b)) / b)
        for k, v in got.items():
            emit(case=case, size=f"{rows}x{cols}", radius=rad, disparities=[lo, hi], flags=flags, form=k, pairs_per_call=forms[k][1],
                 ms_per_pair=round(float(np.median(v)), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                 clock="host, synchronised after the calls")
    if args.trace:
        print("stereo_u8_profile: trace run done")
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in out_rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
