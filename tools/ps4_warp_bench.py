#!/usr/bin/env python3
"""ps4 registration on the device (csrc/warp.hip): device-event timings, one JSON line per case.
  copy     the device copy bandwidth of this run (a 256 MiB f32 buffer copied by torch), the floor's yardstick
  single   micv_warp_affine_dev, u8 and f32, 480x640 / 1080p / 4K, a 10 degree similarity about the centre; next to each
           time the floor (bytes read + bytes written) / copy bandwidth and the ratio time / floor
  batch    micv_warp_affine_batch_dev of 64 images at 1080p against 64 single launches, alternated, per image
  fused    micv_register_blend_dev against micv_invert_affine_dev + micv_warp_affine_dev + micv_add_weighted_dev, alternated
  numpy    tests/_warp_ref.py (a numpy restatement of the contract, NOT OpenCV) on one CPU thread at the same sizes
Warm-up, then --reps timed groups of --inner back-to-back calls between two device events; clock_ms = median group / inner.
  python tools/ps4_warp_bench.py [--reps n] [--inner n] [--out file] [--no-numpy] [--only single,batch,fused]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _warp_ref as wr  # noqa: E402
from introtocomputervision_amd import synth  # noqa: E402
from introtocomputervision_amd._capi import DEPTH_8U, DEPTH_32F, check, lib  # noqa: E402
from introtocomputervision_amd.match import _host_ctx  # noqa: E402

SIZES = [(480, 640), (1080, 1920), (2160, 3840)]


def group_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def time_alternated(fns, reps, inner):
    """Every variant warmed up, then one timed group of each per repetition, in turn."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(group_ms(fn, inner))
    return [{"ms": float(np.median(v)), "ms_min": float(np.min(v)), "ms_std": float(np.std(v))} for v in ms]


def similarity(rows, cols, deg=10.0, scale=1.1):
    t = np.deg2rad(deg)
    a, b = scale * np.cos(t), scale * np.sin(t)
    cx, cy = (cols - 1) / 2, (rows - 1) / 2
    return np.array([[a, -b, cx - a * cx + b * cy], [b, a, cy - b * cx - a * cy]], np.float32)


def image(rows, cols, dtype):
    # a 256 x 256 texture tiled: the content does not change the time, and the generator is slow at 4K
    t = np.tile(synth.smooth_noise(0x5EED00B0, 256, 256, passes=1), (rows // 256 + 1, cols // 256 + 1))[:rows, :cols]
    return np.ascontiguousarray(t.astype(dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--only", default="single,batch,fused", help="comma-separated cases to time (copy always runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing of a device kernel"
    h = _host_ctx().handle
    s = torch.cuda.current_stream().cuda_stream
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

    only = set(a.only.split(","))
    for dtype, depth in ((np.uint8, DEPTH_8U), (np.float32, DEPTH_32F)) if "single" in only else ():
        e = np.dtype(dtype).itemsize
        for rows, cols in SIZES:
            src = torch.from_numpy(image(rows, cols, dtype)).cuda()
            dst = torch.empty_like(src)
            m = torch.from_numpy(similarity(rows, cols)).cuda()
            for flags, mode in ((0, "linear"), (wr.WARP_NEAREST, "nearest")):
                def fn():
                    check(lib.micv_warp_affine_dev(h, src.data_ptr(), depth, rows, cols, cols * e, m.data_ptr(), flags,
                                                   dst.data_ptr(), rows, cols, cols * e, s))
                r = time_alternated([fn], a.reps, a.inner)[0]
                floor_ms = 1e3 * 2 * rows * cols * e / bw
                rec = {"case": "single", "dtype": np.dtype(dtype).name, "mode": mode, "rows": rows, "cols": cols, **r,
                       "bytes_read_plus_written": 2 * rows * cols * e, "floor_ms": floor_ms, "ratio_to_floor": r["ms"] / floor_ms}
                if not a.no_numpy and flags == 0:
                    hs, hm = src.cpu().numpy(), m.cpu().numpy()
                    t0 = time.perf_counter()
                    wr.warp_affine(hs, hm)
                    rec["numpy_restatement_ms_one_thread"] = 1e3 * (time.perf_counter() - t0)
                emit(rec)

    rows, cols, count = 1080, 1920, 64
    for dtype, depth in ((np.uint8, DEPTH_8U), (np.float32, DEPTH_32F)) if "batch" in only else ():
        e = np.dtype(dtype).itemsize
        base = image(rows, cols, dtype)
        srcs = torch.from_numpy(np.stack([np.roll(base, 3 * i, axis=1) for i in range(count)])).cuda()
        dsts = torch.empty_like(srcs)
        ms = torch.from_numpy(np.stack([similarity(rows, cols, 10.0 - 0.2 * i, 1.1 - 0.002 * i) for i in range(count)])).cuda()
        pitch = rows * cols * e

        def batch():
            check(lib.micv_warp_affine_batch_dev(h, srcs.data_ptr(), pitch, depth, rows, cols, cols * e, ms.data_ptr(), count, 0,
                                                 dsts.data_ptr(), pitch, rows, cols, cols * e, s))

        def singles():
            for i in range(count):
                check(lib.micv_warp_affine_dev(h, srcs.data_ptr() + i * pitch, depth, rows, cols, cols * e, ms.data_ptr() + 24 * i, 0,
                                               dsts.data_ptr() + i * pitch, rows, cols, cols * e, s))

        rb, rs = time_alternated([batch, singles], a.reps, 4)
        floor_ms = 1e3 * 2 * pitch / bw
        emit({"case": "batch", "dtype": np.dtype(dtype).name, "rows": rows, "cols": cols, "count": count,
              "batch_ms_per_image": rb["ms"] / count, "singles_ms_per_image": rs["ms"] / count,
              "singles_std_ms_per_image": rs["ms_std"] / count, "batch_std_ms_per_image": rb["ms_std"] / count,
              "floor_ms_per_image": floor_ms,
              "batch_not_slower": rb["ms"] / count <= rs["ms"] / count + rs["ms_std"] / count})

    for dtype, depth in ((np.uint8, DEPTH_8U), (np.float32, DEPTH_32F)) if "fused" in only else ():
        e = np.dtype(dtype).itemsize
        for rows, cols in SIZES:
            A = torch.from_numpy(image(rows, cols, dtype)).cuda()
            Bm = torch.roll(A, 5, 1).contiguous()
            m = torch.from_numpy(similarity(rows, cols)).cuda()
            inv = torch.empty_like(m)
            W, O = torch.empty_like(A), torch.empty_like(A)
            st = cols * e

            def fused():
                check(lib.micv_register_blend_dev(h, A.data_ptr(), st, Bm.data_ptr(), st, depth, rows, cols, m.data_ptr(), None, st,
                                                  O.data_ptr(), st, s))

            def fused_with_warped():
                check(lib.micv_register_blend_dev(h, A.data_ptr(), st, Bm.data_ptr(), st, depth, rows, cols, m.data_ptr(),
                                                  W.data_ptr(), st, O.data_ptr(), st, s))

            def three():
                check(lib.micv_invert_affine_dev(h, m.data_ptr(), 1, inv.data_ptr(), s))
                check(lib.micv_warp_affine_dev(h, Bm.data_ptr(), depth, rows, cols, st, inv.data_ptr(), 0, W.data_ptr(), rows, cols,
                                               st, s))
                check(lib.micv_add_weighted_dev(h, A.data_ptr(), st, 0.5, W.data_ptr(), st, 0.5, 0.0, depth, rows, cols,
                                                O.data_ptr(), st, s))

            rf, rw, r3 = time_alternated([fused, fused_with_warped, three], a.reps, a.inner)
            emit({"case": "fused", "dtype": np.dtype(dtype).name, "rows": rows, "cols": cols, "fused_ms": rf["ms"],
                  "fused_std_ms": rf["ms_std"], "fused_with_warped_ms": rw["ms"], "three_calls_ms": r3["ms"],
                  "three_calls_std_ms": r3["ms_std"], "floor_ms_fused": 1e3 * 3 * rows * cols * e / bw,
                  "fused_faster_by_more_than_spread": r3["ms"] - rf["ms"] > max(rf["ms_std"], r3["ms_std"])})

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
