#!/usr/bin/env python3
"""Times the ps1 driver on one MI355X and writes profiles/ps1_driver/ps1_driver_bench.jsonl:

  * the circle search over a radius range: the one-call form (with and without accumulators) against the per-radius loop
    of houghCirclesAccumulate + findLocalMaxima -- with the host read of every count, as the shim's radius loop ran it
    before the one-call form existed, and with lazy=True (no read) -- the sides alternating in the same run;
  * erode, the float blur, the two draw calls and a whole problem-7 chain, each beside a device-to-device copy of the
    image (the copy floor), the chain also beside the numpy restatement on one CPU thread.

Every shape is warmed first; times are device events around `--reps` calls on one stream (per-call Python included).
No GPU: exits with an error, nothing is estimated.

    python tools/ps1_driver_profile.py --reps 20
    python tools/ps1_driver_profile.py --reps 3 --only search --no-numpy     (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["search", "stages"], default=None)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps1_driver", "ps1_driver_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("ps1_driver_profile: no GPU")
    from introtocomputervision_amd import hough, ps1, synth

    rows_out = []

    def emit(**kw):
        rows_out.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn, reps):
        """ms per call: device events around `reps` calls (the work ends before the second event)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def alternate(forms, reps, rounds=5):
        """forms: name -> callable.  Each round times every form once; returns name -> (median, min, max) ms."""
        for fn in forms.values():  # warm every shape
            fn()
            fn()
        torch.cuda.synchronize()
        got = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, reps))
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}

    sizes = [("480x640", 480, 640), ("1080p", 1080, 1920)]

    if args.only in (None, "search"):
        for name, rows, cols in sizes:
            mask, _, _ = synth.hough_mask(rows, cols)
            d = torch.from_numpy(mask).cuda()
            tiles = ((cols + 63) // 64) * ((rows + 31) // 32)
            for r0, r1, k, thr in [(20, 50, 10, 130), (20, 40, 5, 110)]:
                n = r1 - r0 + 1

                def loop_sync():
                    for r in range(r0, r1 + 1):
                        hough.findLocalMaxima(hough.houghCirclesAccumulate(d, r), k, thr)  # reads the count: a host sync

                def loop_lazy():
                    for r in range(r0, r1 + 1):
                        hough.findLocalMaxima(hough.houghCirclesAccumulate(d, r), k, thr, lazy=True)

                forms = {
                    "range": lambda: ps1.houghCirclesSearch(d, r0, r1, k, thr, lazy=True),
                    "range_acc": lambda: ps1.houghCirclesSearch(d, r0, r1, k, thr, lazy=True, accumulators=True),
                    "loop_sync": loop_sync,
                    "loop_lazy": loop_lazy,
                }
                res = alternate(forms, max(1, args.reps // 4))
                # same peaks from both sides, at the size that is timed
                pk, cnt = ps1.houghCirclesSearch(d, r0, r1, k, thr, lazy=True)
                cnt = cnt.cpu().numpy()
                for i, r in enumerate(range(r0, r1 + 1)):
                    ref = hough.findLocalMaxima(hough.houghCirclesAccumulate(d, r), k, thr).cpu().numpy()
                    assert len(ref) == cnt[i] and np.array_equal(ref, pk[i, :cnt[i]].cpu().numpy()), (name, r)
                for form, (med, lo, hi) in res.items():
                    emit(case="radius_search", size=name, radii=[r0, r1], num_peaks=k, threshold=thr, form=form,
                         ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), us_per_radius=round(1e3 * med / n, 2),
                         workgroups_per_vote_launch=tiles * n if form.startswith("range") else tiles,
                         vote_launches=1 if form.startswith("range") else n, edge_points=int((mask > 0).sum()),
                         peaks_found=int(cnt.sum()))

    if args.only in (None, "stages"):
        import _ps1_driver_ref as R
        for name, rows, cols in sizes:
            rng = np.random.default_rng(rows)
            yy, xx = np.mgrid[0:rows, 0:cols]
            img = np.full((rows, cols), 200.0)
            for i in range(12):
                cy, cx, r = rng.integers(45, rows - 45), rng.integers(45, cols - 45), rng.integers(20, 41)
                img[np.hypot(yy - cy, xx - cx) <= r] = 40
            img = (img + rng.random((rows, cols)) * 6).astype(np.float32)
            d = torch.from_numpy(img).cuda()
            rgb = ps1.gray2rgb(d)
            scratch_f, scratch_rgb = torch.empty_like(d), torch.empty_like(rgb)
            edge_cfg, circ_cfg = (3, 1.0, 35, 130), (20, 40, 10, 135)  # problem 7 of config/ps1.yaml
            edges = ps1.generateEdge(ps1.erode(d, 5), *edge_cfg)
            pk, cnt = ps1.houghCirclesSearch(edges, *circ_cfg, lazy=True)
            acc = hough.houghLinesAccumulate(edges, 1, 1)
            lpk, lcnt = hough.findLocalMaxima(acc, 10, 105, lazy=True)

            def chain():
                e = ps1.generateEdge(ps1.erode(d, 5), *edge_cfg)
                p, c = ps1.houghCirclesSearch(e, *circ_cfg, lazy=True)
                return ps1.drawCircles(ps1.gray2rgb(d), p, circ_cfg[0], counts=c)

            forms = {
                "copy_f32": lambda: scratch_f.copy_(d),
                "copy_rgb8": lambda: scratch_rgb.copy_(rgb),
                "erode5_f32": lambda: ps1.erode(d, 5),
                "blur13_f32": lambda: ps1.gaussianBlur(d, 13, 4.0),
                "draw_circles": lambda: ps1.drawCircles(rgb, pk, circ_cfg[0], counts=cnt),
                "draw_lines": lambda: ps1.drawLinesParametric(rgb, lpk, 1, 1, count=lcnt),
                "problem7_chain": chain,
            }
            res = alternate(forms, args.reps)
            for form, (med, lo, hi) in res.items():
                emit(case="stage", size=name, form=form, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                     circles=int(cnt.sum().item()), lines=int(lcnt.item()))
            if not args.no_numpy and name == "480x640":
                t0 = time.perf_counter()
                _, marked = R.problem7(img, edge_cfg, circ_cfg)
                cpu_ms = 1e3 * (time.perf_counter() - t0)
                assert np.array_equal(chain().cpu().numpy(), marked)
                emit(case="stage", size=name, form="problem7_numpy_restatement_one_thread", ms=round(cpu_ms, 1))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows_out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
