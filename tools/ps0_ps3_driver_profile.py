#!/usr/bin/env python3
"""Times ps0.run and the ps3 driver's drawing on one MI355X at 512 x 512 x 3 and at 1080 x 1920 x 3 and writes
profiles/ps0_ps3_driver/ps0_ps3_driver_bench.jsonl.

ps0, per call (the nine pictures and the record; noise planes on the device):
  ps0_run             ps0.run on device tensors: three launches;
  ps0_separate_calls  the separate `_dev` calls (3 x extractChannel of image1 + 1 of image2, swapRedBlue, pixelReplacement,
                      meanStdDev, doArithmeticOperations on the device record, translateImg, subtract, 2 x addGaussianNoise);
  ps0_bytes_copy      a device copy of as many bytes as ps0.run reads and writes (the floor);
  ps0_numpy_one_thread  the numpy restatement tests/_ps0_ref.py on this host's CPU (no device involved).
ps3, per call (two pictures), n = 20 and n = 2000 point pairs, the points already n x 2 on the device (the entry points are
called directly, so a call is the library's launches and nothing else):
  epipolar_display      micv_ps3_epipolar_display_dev in place: ONE launch (end points and lines);
  endpoints_then_lines  2 x micv_epipolar_endpoints_dev + 2 x micv_draw_epipolar_lines_dev: four launches;
  picture_copy          a device copy of both pictures, what a not-in-place call adds;
  parent_device_part    the parent commit's way: 2 x micv_epipolar_endpoints_host, then the upload of the two pictures that
                        the host has drawn; its host loop (clone + n micv_viz::line walks per picture on one thread:
                        tools/probes/ps3_host_loops.cpp, no device involved) is timed apart and comes on top.

Every form is warmed first; times are a host clock around `--calls` calls that end in a synchronise, the median of five
rounds with the forms alternating.  They are enqueue plus execution of back-to-back calls, not kernel times.  No GPU: exits
with an error, nothing is estimated.

    python tools/ps0_ps3_driver_profile.py
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PROBE_SRC = os.path.join(ROOT, "tools", "probes", "ps3_host_loops.cpp")
PROBE_BIN = os.path.join(ROOT, "tools", "probes", "_bin", "ps3_host_loops")


def probe(rows, cols, n, reps):
    if not os.path.exists(PROBE_BIN):
        os.makedirs(os.path.dirname(PROBE_BIN), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", PROBE_SRC, "-o", PROBE_BIN], check=True)
    out = subprocess.run([PROBE_BIN, "time", str(rows), str(cols), str(n), str(reps)], check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def scene(rows, cols, n, seed):
    """Two pictures, n point pairs (2 x n) and an F whose lines cross the pictures at every slope."""
    rng = np.random.default_rng(seed)
    pics = [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in range(2)]
    pts = [np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)]).astype(np.float32) for _ in range(2)]
    F = rng.normal(0, 1, (3, 3)).astype(np.float32)
    F[:2, :2] *= np.float32(1.0 / max(rows, cols))
    return pics, pts, F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps0_ps3_driver", "ps0_ps3_driver_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("ps0_ps3_driver_profile: no GPU")
    import _ps0_ref as R0
    from introtocomputervision_amd import display, geometry, ps0, ps3
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

    def measure(forms, launches, calls=None, **tags):
        calls = calls or args.calls
        for fn in forms.values():
            fn()
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(wall(fn, calls))
        for k, v in got.items():
            emit(**tags, form=k, ms_per_call=round(float(np.median(v)), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                 library_launches=launches.get(k), calls=calls, clock="host, synchronised after the calls")

    for rows, cols in ((512, 512), (1080, 1920)):
        # ---- ps0
        pics, _, _ = scene(rows, cols, 4, 77)
        d1, d2 = (torch.from_numpy(p).cuda() for p in pics)
        rng = display.RNG(5)
        ng, nb = display.randn((rows, cols), 0, 5, rng), display.randn((rows, cols), 0, 5, rng)
        dg, db = torch.from_numpy(ng).cuda(), torch.from_numpy(nb).cuda()
        n = rows * cols
        moved = (3 * n + 8 * n + 3 * n + n) + (3 * n + 7 * n + n)  # image1, noise, image2, green again | swapped, planes, replaced
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def separate():
            green, red, blue = (ps0.extractChannel(d1, c) for c in (1, 2, 0))
            ps0.swapRedBlue(d1)
            ps0.pixelReplacement(red, ps0.extractChannel(d2, 2))
            ps0.doArithmeticOperations(green, ps0.meanStdDev(green))
            ps0.subtract(green, ps0.translateImg(green, -2, 0))
            ps0.addGaussianNoise(green, noise=dg)
            ps0.addGaussianNoise(blue, noise=db)

        measure({"ps0_run": lambda: ps0.run(d1, d2, dg, db), "ps0_separate_calls": separate, "ps0_bytes_copy": lambda: dst.copy_(src)},
                {"ps0_run": 3, "ps0_separate_calls": 13, "ps0_bytes_copy": 1}, size=f"{rows}x{cols}x3", bytes_moved=moved)
        t0 = time.perf_counter()
        for _ in range(3):
            R0.run(pics[0], pics[1], ng, nb)
        emit(size=f"{rows}x{cols}x3", form="ps0_numpy_one_thread", ms_per_call=round(1e3 * (time.perf_counter() - t0) / 3, 3),
             note="tests/_ps0_ref.py on the profiling host's CPU")

        # ---- ps3
        col = (C.c_double * 4)(*ps3.LINE_COLOR)
        for npts in (20, 2000):
            pics, pts, F = scene(rows, cols, npts, 323 + npts)
            dA, dB = (torch.from_numpy(p).cuda() for p in pics)
            cA, cB = torch.empty_like(dA), torch.empty_like(dB)
            ra, rb = (torch.from_numpy(np.ascontiguousarray(p.T)).cuda() for p in pts)  # n x 2, as the C ABI takes them
            dF = torch.from_numpy(F).cuda()
            eA, eB = (torch.empty((npts, 6), dtype=torch.float32, device="cuda") for _ in range(2))
            h, s = _ctx_for(dA, None).handle, torch.cuda.current_stream().cuda_stream
            stride = cols * 3

            def one_launch():
                check(lib.micv_ps3_epipolar_display_dev(h, dF.data_ptr(), ra.data_ptr(), rb.data_ptr(), npts, dA.data_ptr(), stride, rows, cols,
                                                        dB.data_ptr(), stride, rows, cols, 3, 0, col, dA.data_ptr(), stride, dB.data_ptr(),
                                                        stride, None, s))

            def two_step():
                check(lib.micv_epipolar_endpoints_dev(h, dF.data_ptr(), rb.data_ptr(), npts, 0, rows, cols, 0, eA.data_ptr(), s))
                check(lib.micv_draw_epipolar_lines_dev(h, dA.data_ptr(), rows, cols, 3, stride, eA.data_ptr(), npts, col, s))
                check(lib.micv_epipolar_endpoints_dev(h, dF.data_ptr(), ra.data_ptr(), npts, 1, rows, cols, 0, eB.data_ptr(), s))
                check(lib.micv_draw_epipolar_lines_dev(h, dB.data_ptr(), rows, cols, 3, stride, eB.data_ptr(), npts, col, s))

            def copies():
                cA.copy_(dA)
                cB.copy_(dB)

            def parent():
                geometry.fundamental.epipolarEndpoints(F, pts[1], 0, rows, cols)
                geometry.fundamental.epipolarEndpoints(F, pts[0], 1, rows, cols)
                torch.from_numpy(pics[0]).cuda()
                torch.from_numpy(pics[1]).cuda()

            measure({"epipolar_display": one_launch, "endpoints_then_lines": two_step, "picture_copy": copies, "parent_device_part": parent},
                    {"epipolar_display": 1, "endpoints_then_lines": 4, "picture_copy": 2, "parent_device_part": 2}, size=f"{rows}x{cols}x3",
                    n=npts)
            host = probe(rows, cols, npts, 20 if npts > 100 else 200)
            emit(size=f"{rows}x{cols}x3", n=npts, form="parent_host_loop_one_thread", ms_per_call=round(2 * host["viz_line_ms_per_picture"], 4),
                 line_wide_ms_per_call=round(2 * host["line_wide_ms_per_picture"], 4),
                 note="2 x (clone + n micv_viz::line walks) on the profiling host's CPU; comes on top of parent_device_part")

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in out_rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
