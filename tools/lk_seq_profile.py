#!/usr/bin/env python3
"""What pyramidal LK over a device-resident frame sequence costs per pair: the per-pair loop, the batch entry on grey
planes, and micv_lk_flow_seq_async, which converts and decimates every frame once and runs all pairs as one batch.

    python tools/lk_seq_profile.py [--out profiles/lk_seq] [--rounds 9] [--no-timing] [--no-resources] [--quick]

Sizes 480 x 640 and 1080 x 1920; frames 8-bit BGR and 8-bit grey; F = 3, 9, 27; window 15 / 5 levels and window 21 / 4
levels.  Per configuration, microseconds per PAIR:
  (a) loop            micv_to_gray_f32_dev per frame + micv_lk_flow_pyr_dev per pair: the only way before this entry
  (b) gray + batch    micv_to_gray_f32_dev per frame + ONE micv_lk_flow_pyr_batch_dev with next = prev + one frame
  (c) seq mp=0|4|16   micv_lk_flow_seq_async with max_pairs 0 (pieces of 8), 4 and 16
  (d) microseconds per FRAME of the grey-and-pyramid launch alone (micv_gray_pyramid_seq_async), of a device copy that
      moves the bytes it reads and writes (its floor), and of the F grey launches + one build launch it replaces
  (e) display seq     micv_dense_lk_display_seq_async against the loop of micv_dense_lk_display_dev (1080p and 480p, BGR)
  (f) host            micv_lk_flow_seq_host against a trial that uploads chunks of 9 frames, runs micv_lk_flow_seq_async
      on each and downloads the flows (1080p BGR; measured only, nothing in the library does this)
Every figure is the median over `rounds` windows, host clock around a window of calls that ends in a device synchronise,
the variants alternating round by round in one process on one build; min and max are the spread.  The results are
compared before anything is timed.  The timing needs a GPU; there is no fallback.

resources.txt in the same directory is the compiler's report for the kernels of pyramid.hip (tools/kernel_resources.py);
it needs the compiler and no GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resources(out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "pyramid"], capture_output=True, text=True)
    if r.returncode:
        raise SystemExit("lk_seq_profile: the resource report failed:\n" + r.stderr)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write(r.stdout)
    print(r.stdout, end="")


def make_frames(nframes, rows, cols, cn):
    """A smooth texture per channel drifting by (2, 1) pixels per frame, 8 bit."""
    rng = np.random.default_rng(rows * 7 + cols)
    base = rng.integers(0, 256, (rows // 8 + 9, cols // 8 + 9, cn)).astype(np.float32)
    base = np.kron(base, np.ones((8, 8, 1), np.float32))[:rows + 64, :cols + 64]
    for _ in range(2):
        base = (base + np.roll(base, 3, 0) + np.roll(base, 3, 1) + np.roll(base, (3, 3), (0, 1))) / 4
    out = np.stack([base[64 - t:64 - t + rows, 64 - 2 * t:64 - 2 * t + cols] for t in range(nframes)])
    out = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out if cn > 1 else out[..., 0]


def measure(variants, rounds, target_s=0.004):
    """variants: name -> (fn, units per call).  Median / min / max seconds per unit over `rounds` alternating windows."""
    import torch
    calls = {}
    for v, (fn, _) in variants.items():  # warm-up (code objects, the arena) and the window length
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        calls[v] = max(1, min(200, int(target_s / max(time.perf_counter() - t0, 1e-6))))
    times = {v: [] for v in variants}
    for _ in range(rounds):
        for v, (fn, n) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls[v]):
                fn()
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) / (calls[v] * n))
    return {v: (sorted(ts), calls[v]) for v, ts in times.items()}


def timing(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lk_seq_profile: no GPU (timings are only taken on one)")
    from introtocomputervision_amd import _capi, lk, ps5
    lib = _capi.lib
    s = torch.cuda.current_stream().cuda_stream
    ctx = lk.default_context(0, s)
    h = ctx.handle
    lines = []

    def record(part, cfg, unit, res):
        for v, (ts, calls) in res.items():
            rec = dict(part=part, **cfg, variant=v)
            rec.update({f"us_per_{unit}_median": round(1e6 * ts[len(ts) // 2], 2), f"us_per_{unit}_min": round(1e6 * ts[0], 2),
                        f"us_per_{unit}_max": round(1e6 * ts[-1], 2), "rounds": len(ts), "calls_per_window": calls})
            lines.append(rec)
            print(json.dumps(rec), flush=True)

    sizes = [(480, 640)] if a.quick else [(480, 640), (1080, 1920)]
    counts = (3, 9) if a.quick else (3, 9, 27)
    for rows, cols in sizes:
        for cn, fmt in ((3, "u8 bgr"), (1, "u8 grey")):
            all_frames = torch.from_numpy(make_frames(max(counts), rows, cols, cn)).cuda()
            for nf in counts:
                fr = all_frames[:nf]
                fp, row = fr.stride(0), fr.stride(1)
                grey = torch.empty((nf, rows, cols), dtype=torch.float32, device="cuda")
                u = torch.empty((nf - 1, rows, cols), dtype=torch.float32, device="cuda")
                v = torch.empty_like(u)
                n4, pb = cols * 4, rows * cols * 4

                def to_gray():
                    for t in range(nf):
                        lib.micv_to_gray_f32_dev(h, fr.data_ptr() + t * fp, rows, cols, row, cn, 0, grey.data_ptr() + t * pb, n4, s)

                for win, levels in ((15, 5), (21, 4)):
                    def loop():
                        to_gray()
                        for p in range(nf - 1):
                            _capi.check(lib.micv_lk_flow_pyr_dev(h, grey.data_ptr() + p * pb, grey.data_ptr() + (p + 1) * pb, rows, cols, n4, win,
                                                                 levels, u.data_ptr() + p * pb, v.data_ptr() + p * pb, n4, s))

                    def batch():
                        to_gray()
                        _capi.check(lib.micv_lk_flow_pyr_batch_dev(h, grey.data_ptr(), grey.data_ptr() + pb, nf - 1, pb, rows, cols, n4, win, levels,
                                                                   u.data_ptr(), v.data_ptr(), pb, n4, s))

                    def seq(mp):
                        _capi.check(lib.micv_lk_flow_seq_async(h, fr.data_ptr(), fp, nf, rows, cols, row, cn, 0, win, levels, mp, u.data_ptr(),
                                                               v.data_ptr(), pb, n4, s))

                    loop()
                    eu, ev = u.clone(), v.clone()
                    for fn in (batch, lambda: seq(0), lambda: seq(4), lambda: seq(16)):  # the same bytes every way
                        u.zero_()
                        fn()
                        assert torch.equal(u, eu) and torch.equal(v, ev)
                    variants = {"(a) loop": (loop, nf - 1), "(b) gray + batch": (batch, nf - 1)}
                    for mp in (0, 4, 16):
                        variants[f"(c) seq max_pairs={mp}"] = ((lambda mp=mp: seq(mp)), nf - 1)
                    cfg = dict(size=f"{rows}x{cols}", format=fmt, frames=nf, win=win, levels=levels)
                    record("flow", cfg, "pair", measure(variants, a.rounds))

                # (d) the grey-and-pyramid launch alone, 5 levels
                levels = 5
                lv = [grey] + [torch.empty((nf, rows >> l, cols >> l), dtype=torch.float32, device="cuda") for l in range(1, levels)]
                arr = (_capi.vp * levels)(*[None if l == 0 else t.data_ptr() for l, t in enumerate(lv)])
                moved = nf * rows * cols * cn + sum(t.numel() * 4 for t in lv)  # bytes read + bytes written
                ca = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
                cb = torch.empty_like(ca)

                def kernel():
                    _capi.check(lib.micv_gray_pyramid_seq_async(h, fr.data_ptr(), fp, nf, rows, cols, row, cn, 0, levels, grey.data_ptr(), pb,
                                                                arr, s))

                def replaced():
                    to_gray()
                    _capi.check(lib.micv_gaussian_pyramid_batch_dev(h, grey.data_ptr(), nf, pb, rows, cols, n4, levels, arr, None, None, s))

                cfg = dict(size=f"{rows}x{cols}", format=fmt, frames=nf, levels=levels, bytes_moved=moved)
                record("pyramid", cfg, "frame", measure({"(d) one launch": (kernel, nf), "(d) copy of its bytes": ((lambda: cb.copy_(ca)), nf),
                                                         "(d) F grey launches + build": (replaced, nf)}, a.rounds))

            # (e) the display driver, BGR and grey, F = 9
            nf = 9
            fr = all_frames[:nf]
            want = [ps5.denseLKDisplay(fr[p], fr[p + 1], "pyramidal", winSize=21, levels=4) for p in range(nf - 1)]
            got = ps5.denseLKDisplaySequence(fr, winSize=21, levels=4)
            for p in range(nf - 1):
                for k, e in zip(("u", "v", "arrows", "uColorMap", "vColorMap"), want[p]):
                    assert torch.equal(got[k][p], e), (k, p)
            del want, got
            cfg = dict(size=f"{rows}x{cols}", format=fmt, frames=nf, win=21, levels=4)
            record("display", cfg, "pair", measure({
                "(e) loop of micv_dense_lk_display_dev": ((lambda: [ps5.denseLKDisplay(fr[p], fr[p + 1], "pyramidal", winSize=21, levels=4)
                                                                   for p in range(nf - 1)]), nf - 1),
                "(e) micv_dense_lk_display_seq_async": ((lambda: ps5.denseLKDisplaySequence(fr, winSize=21, levels=4)), nf - 1)}, a.rounds))

    # (f) the host sequence entry against chunks through the device entry: a trial, measured only
    rows, cols = sizes[-1]
    for nf in (9, 27):
        host = make_frames(nf, rows, cols, 3)
        flist = [host[t] for t in range(nf)]
        out = (np.empty((nf - 1, rows, cols), np.float32), np.empty((nf - 1, rows, cols), np.float32))
        out2 = (np.empty_like(out[0]), np.empty_like(out[1]))
        pin = [torch.from_numpy(o) for o in out2]

        def seq_host():
            lk.calcOpticalFlowPyrSequence(flist, winSize=21, levels=4, out=out)

        def chunked():
            for f0, np_ in lk.sequencePlan(nf, 8):
                d = torch.from_numpy(host[f0:f0 + np_ + 1]).cuda()
                cu, cv = lk.calcOpticalFlowPyrSequenceDevice(d, winSize=21, levels=4, max_pairs=8)
                pin[0][f0:f0 + np_].copy_(cu)
                pin[1][f0:f0 + np_].copy_(cv)

        seq_host()
        chunked()
        assert np.array_equal(out[0], out2[0]) and np.array_equal(out[1], out2[1])
        cfg = dict(size=f"{rows}x{cols}", format="u8 bgr", frames=nf, win=21, levels=4)
        record("host", cfg, "pair", measure({"(f) micv_lk_flow_seq_host": (seq_host, nf - 1),
                                             "(f) chunks of 9 frames through micv_lk_flow_seq_async": (chunked, nf - 1)},
                                            min(a.rounds, 5), target_s=0.0))
    with open(os.path.join(a.out, "profile.jsonl"), "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_seq"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="480 x 640 and F = 3, 9 only")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if not a.no_resources:
        resources(a.out)
    if not a.no_timing:
        timing(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
