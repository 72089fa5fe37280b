#!/usr/bin/env python3
"""The display tail on the device (csrc/display.hip) against the host path it replaces; one JSON line per case.
  copy       the device copy bandwidth of this run (a 256 MiB f32 buffer copied by torch): the floor's yardstick
  normalize  micv_normalize_minmax[_batch]_dev, f32 -> JET, one field and a batch of 16 (per image) at 480x640, 1080p, 4K,
             alternated, beside the floor (source read twice + 3 bytes per pixel written) / copy bandwidth; and the int8 ->
             u8 form of the ps2 maps
  host       the same work on the path that existed before: download of the f32 field (pageable host memory), then
             micv_viz::normalize_minmax_u8 + apply_colormap_jet on one thread (tools/probes/display_host_loops.cpp); beside
             it the device call followed by the download of the B, G, R image, and the whole `_host` call (upload included)
  ps2        one pair-and-display block at 511 x 640, radius 7, range 95, SSD and NCC: micv_disparity_pair_display_dev +
             download of the three images and two maps, against the two existing disparity calls + download of the maps
             (+ the host loops, from the probe); and the device time of the chain against the two searches alone
Device times: warm-up, then --reps groups of --inner back-to-back calls between two device events, the median group per
call; variants that are compared are timed in turn inside every repetition.  Host-clocked times end in a synchronise.
  python tools/display_bench.py [--reps n] [--inner n] [--out file] [--only normalize,host,ps2]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from introtocomputervision_amd import stereo, synth  # noqa: E402
from introtocomputervision_amd._capi import DEPTH_8S, DEPTH_32F, check, lib  # noqa: E402
from introtocomputervision_amd.match import _host_ctx  # noqa: E402

SIZES = [(480, 640), (1080, 1920), (2160, 3840)]
PROBE_SRC = os.path.join(ROOT, "tools", "probes", "display_host_loops.cpp")
PROBE_BIN = os.path.join(ROOT, "tools", "probes", "_bin", "display_host_loops")


def group_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def stats(v):
    return {"ms": float(np.median(v)), "ms_min": float(np.min(v)), "ms_std": float(np.std(v))}


def time_alternated(fns, reps, inner):
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(group_ms(fn, inner))
    return [stats(v) for v in ms]


def host_clock_alternated(fns, reps):
    """Each fn ends in a synchronise; one call of each per repetition, in turn."""
    for fn in fns:
        fn()
        fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ms[i].append(1e3 * (time.perf_counter() - t0))
    return [stats(v) for v in ms]


def host_loops(mode, rows, cols, reps):
    if not os.path.exists(PROBE_BIN):
        os.makedirs(os.path.dirname(PROBE_BIN), exist_ok=True)
        libdir = os.path.join(ROOT, "introtocomputervision_amd")
        subprocess.run(["g++", "-std=c++17", "-O2", PROBE_SRC, "-o", PROBE_BIN, "-L" + libdir, "-lmicv", "-Wl,-rpath," + libdir],
                       check=True)
    out = subprocess.run([PROBE_BIN, mode, str(rows), str(cols), str(reps)], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="normalize,host,ps2")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing of a device kernel"
    h = _host_ctx().handle
    s = torch.cuda.current_stream().cuda_stream
    only = set(a.only.split(","))
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    n = 64 << 20
    x, y = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    x.fill_(1.0)
    r = time_alternated([lambda: y.copy_(x)], a.reps, 10)[0]
    bw = 2 * 4 * n / (r["ms"] * 1e-3)
    emit({"case": "copy", "bytes_each_way": 4 * n, **r, "copy_bytes_per_s": bw})
    del x, y

    gen = torch.Generator(device="cuda").manual_seed(7)
    B = 16
    for rows, cols in SIZES:
        px = rows * cols
        if not ({"normalize", "host"} & only):
            break
        many = torch.randn((B, rows, cols), device="cuda", generator=gen) * 3 + 0.5
        one = many[0]
        jet = torch.empty((B, rows, cols, 3), dtype=torch.uint8, device="cuda")
        maps = torch.randint(-95, 1, (B, rows, cols), dtype=torch.int8, device="cuda")
        u8 = torch.empty((B, rows, cols), dtype=torch.uint8, device="cuda")

        def single():
            check(lib.micv_normalize_minmax_dev(h, one.data_ptr(), DEPTH_32F, rows, cols, cols * 4, None, 0, None, 0,
                                                jet.data_ptr(), cols * 3, None, s))

        def batch():
            check(lib.micv_normalize_minmax_batch_dev(h, many.data_ptr(), px * 4, DEPTH_32F, B, rows, cols, cols * 4, None, 0, 0,
                                                      None, 0, 0, jet.data_ptr(), px * 3, cols * 3, None, s))

        def single_i8():
            check(lib.micv_normalize_minmax_dev(h, maps.data_ptr(), DEPTH_8S, rows, cols, cols, u8.data_ptr(), cols, None, 0,
                                                None, 0, None, s))

        def jet_only():  # the apply pass alone (u8 -> B, G, R): what a one-launch normalise could at best come down to
            check(lib.micv_apply_colormap_jet_dev(h, u8.data_ptr(), rows, cols, cols, jet.data_ptr(), cols * 3, s))

        if "normalize" in only:
            rs, rb, ri, rj = time_alternated([single, batch, single_i8, jet_only], a.reps, a.inner if rows < 2000 else 10)
            floor = 1e3 * (2 * 4 + 3) * px / bw
            emit({"case": "normalize", "rows": rows, "cols": cols, "src": "f32", "out": "jet", "single_ms": rs["ms"],
                  "single_std_ms": rs["ms_std"], "batch16_ms_per_image": rb["ms"] / B, "batch16_std_ms_per_image": rb["ms_std"] / B,
                  "floor_ms": floor, "bytes_read_twice_plus_written": 11 * px, "single_ratio_to_floor": rs["ms"] / floor,
                  "batch16_ratio_to_floor": rb["ms"] / B / floor, "int8_to_u8_single_ms": ri["ms"], "int8_to_u8_std_ms": ri["ms_std"],
                  "int8_floor_ms": 1e3 * 3 * px / bw, "apply_colormap_alone_ms": rj["ms"], "apply_colormap_alone_std_ms": rj["ms_std"]})

        if "host" in only:
            field = np.empty((rows, cols), np.float32)
            field_t = torch.from_numpy(field)  # pageable, like a cv::Mat
            img = np.empty((rows, cols, 3), np.uint8)
            img_t = torch.from_numpy(img)
            src_host = one.cpu().numpy()

            def download_field():
                field_t.copy_(one)
                torch.cuda.synchronize()

            def device_then_download():
                single()
                img_t.copy_(jet[0])
                torch.cuda.synchronize()

            def host_entry():
                check(lib.micv_normalize_minmax_host(h, src_host.ctypes.data, DEPTH_32F, rows, cols, cols * 4, None, 0, None, 0,
                                                     img.ctypes.data, cols * 3, None))

            rd, rn, rh = host_clock_alternated([download_field, device_then_download, host_entry], a.reps)
            loops = host_loops("jet", rows, cols, a.reps)
            emit({"case": "host", "rows": rows, "cols": cols, "download_f32_field_ms": rd["ms"], "download_std_ms": rd["ms_std"],
                  "host_loops_one_thread_ms": loops["ms"], "host_loops_std_ms": loops["ms_std"],
                  "old_path_ms": rd["ms"] + loops["ms"], "device_call_plus_download_of_bgr_ms": rn["ms"],
                  "device_call_plus_download_std_ms": rn["ms_std"], "host_entry_upload_included_ms": rh["ms"],
                  "host_entry_std_ms": rh["ms_std"], "old_over_new": (rd["ms"] + loops["ms"]) / rn["ms"]})
        del many, jet, maps, u8

    if "ps2" in only:
        rows, cols, rad, rng = 511, 640, 7, 95
        left, right, _ = synth.stereo_pair(0x5EED0F20, rows, cols)
        L, R = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        dl, dr = (torch.empty((rows, cols), dtype=torch.int8, device="cuda") for _ in range(2))
        imgs = torch.empty((3, rows, cols), dtype=torch.uint8, device="cuda")
        hmaps = torch.from_numpy(np.empty((2, rows, cols), np.int8))
        himgs = torch.from_numpy(np.empty((3, rows, cols), np.uint8))
        px = rows * cols
        loops = host_loops("ps2", rows, cols, a.reps)
        for name, metric, flags, fn in (("ssd", stereo.SSD, stereo.AS_WRITTEN_CUDA, lib.micv_disparity_ssd_dev),
                                        ("ncc", stereo.NCC, 1, lib.micv_disparity_ncorr_dev)):
            def two_calls():
                check(fn(h, L.data_ptr(), R.data_ptr(), rows, cols, cols * 4, rad, -rng, 0, flags, dl.data_ptr(), cols, s))
                check(fn(h, R.data_ptr(), L.data_ptr(), rows, cols, cols * 4, rad, 0, rng, flags, dr.data_ptr(), cols, s))

            def chain():
                check(lib.micv_disparity_pair_display_dev(h, L.data_ptr(), R.data_ptr(), rows, cols, cols * 4, 1.0, None, None, 0,
                                                          rad, rng, metric, flags, dl.data_ptr(), dr.data_ptr(), cols,
                                                          imgs.data_ptr(), imgs.data_ptr() + px, imgs.data_ptr() + 2 * px, cols,
                                                          None, s))

            def old_end_to_end():
                two_calls()
                hmaps[0].copy_(dl)
                hmaps[1].copy_(dr)
                torch.cuda.synchronize()

            def new_end_to_end():
                chain()
                hmaps[0].copy_(dl)
                hmaps[1].copy_(dr)
                himgs.copy_(imgs)
                torch.cuda.synchronize()

            r2, rc = time_alternated([two_calls, chain], a.reps, 5)
            ro, rn = host_clock_alternated([old_end_to_end, new_end_to_end], a.reps)
            emit({"case": "ps2", "metric": name, "rows": rows, "cols": cols, "radius": rad, "range": rng,
                  "two_searches_device_ms": r2["ms"], "two_searches_std_ms": r2["ms_std"], "chain_device_ms": rc["ms"],
                  "chain_std_ms": rc["ms_std"], "display_tail_device_ms": rc["ms"] - r2["ms"],
                  "old_searches_plus_download_of_maps_ms": ro["ms"], "old_std_ms": ro["ms_std"],
                  "host_loops_one_thread_ms": loops["ms"], "host_loops_std_ms": loops["ms_std"],
                  "old_path_ms": ro["ms"] + loops["ms"], "new_chain_plus_downloads_ms": rn["ms"], "new_std_ms": rn["ms_std"]})

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
