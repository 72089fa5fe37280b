#!/usr/bin/env python3
"""Times the colour frameDifference, the video batch and ps7.runProblem2 on one MI355X and writes
profiles/ps7_color/ps7_color_bench.jsonl (the method of tools/ps0_ps3_driver_profile.py).

(a) frame_difference, 480 x 640 and 1080 x 1920, blur 3 x 3 / sigma 1 and 31 x 31 / sigma 10, per call:
  color3 / color4        micv_mhi_frame_difference_c_dev on interleaved frames of 3 / 4 channels: two launches;
  three_planes           three calls of the single-channel micv_mhi_frame_difference_dev on planes of that size (what a
                         caller had to do before, short of the grey step): six launches;
  bytes_copy             a device copy of the bytes the colour call reads (both frames, three channels).
(b) batch, 27 videos of 480 x 640 with config/ps7.yaml's parameters and last frames:
  batch_c1 / batch_c3    micv_mhi_history_batch_dev, one and three channels: two launches per step;
  seq_loop_c1            27 calls of micv_mhi_history_seq_dev (the parent's way: three launches and a copy per update);
  seq_loop_c3            27 calls of micv_mhi_history_seq_c_dev on the colour videos.
(c) problem2, the same 27 one-channel videos from resident frames to the confusion matrices:
  run_problem2           ps7.runProblem2;
  separate_calls         the chain of tools/ps7_bench.py (one historySequence and one energyFromHistory per video).

Every form is warmed first; times are a host clock around `--calls` calls that end in a synchronise, the median of five
rounds with the forms alternating.  They are enqueue plus execution of back-to-back calls, not kernel times.  No GPU:
exits with an error, nothing is estimated.

    python tools/ps7_color_profile.py [--skip-batch]
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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps7_color", "ps7_color_bench.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("ps7_color_profile: no GPU")
    import _ps7_ref as ref
    from introtocomputervision_amd import config, matching, mhi, moments, ps7

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

    def measure(forms, launches, calls, **tags):
        for fn in forms.values():
            fn()
        got = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                got[k].append(wall(fn, calls))
        for k, v in got.items():
            emit(**tags, form=k, ms_per_call=round(float(np.median(v)), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                 library_launches=launches.get(k), calls=calls, clock="host, synchronised after the calls")

    # ---- (a)
    rng = np.random.default_rng(7)
    for rows, cols in ((480, 640), (1080, 1920)):
        f = [torch.from_numpy(rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)).cuda() for _ in range(2)]
        c3 = [x[..., :3].contiguous() for x in f]
        planes = [[x[..., c].contiguous() for c in range(3)] for x in f]
        src, dst = torch.cat([c3[0].view(-1), c3[1].view(-1)]), torch.empty(2 * rows * cols * 3, dtype=torch.uint8, device="cuda")
        for blur, sigma in ((3, 1.0), (31, 10.0)):
            measure({"color3": lambda: mhi.frameDifference(c3[0], c3[1], 20, blur, sigma),
                     "color4": lambda: mhi.frameDifference(f[0], f[1], 20, blur, sigma),
                     "three_planes": lambda: [mhi.frameDifference(planes[0][c], planes[1][c], 20, blur, sigma) for c in range(3)],
                     "bytes_copy": lambda: dst.copy_(src)},
                    {"color3": 2, "color4": 2, "three_planes": 6, "bytes_copy": 1}, args.calls, what="frame_difference",
                    size=f"{rows}x{cols}", blur=blur, bytes_read=2 * rows * cols * 3)
    if args.skip_batch:
        return write(args.out, out_rows)

    # ---- (b), (c)
    cfg = config.load(os.path.join(ROOT, "tests", "golden", "config", "ref", "ps7.yaml"))
    last = config.last_frames(cfg)
    vids, vids3, params = {}, {}, []
    for a in (1, 2, 3):
        p = config.mhi_params(cfg, f"mhi_action{a}")
        for person in (1, 2, 3):
            for trial in (1, 2, 3):
                name = f"PS7A{a}P{person}T{trial}"
                fr = ref.action_video(1000 * a + 10 * person + trial, a, last[name] + 1, 480, 640)
                vids[name] = torch.from_numpy(fr).cuda()
                # the blob at another place and brightness in the other two channels
                vids3[name] = torch.from_numpy(np.stack([fr, np.roll(fr, 40, 2), fr // 2], -1)).cuda()
                params.append((name, p, last[name], a, person))
    updates = sum(q[2] for q in params)

    def batch(v):
        return lambda: mhi.historyBatch([v[q[0]] for q in params], [q[1]["diff_threshold"] for q in params],
                                        params[0][1]["pre_blur_size"], params[0][1]["pre_blur_sigma"],
                                        [q[1]["tau"] for q in params], [q[2] for q in params])

    def loop(v):
        return lambda: [mhi.historySequence(v[n], p["diff_threshold"], p["pre_blur_size"], p["pre_blur_sigma"], p["tau"], [lf])
                        for n, p, lf, _, _ in params]

    steps = max(q[2] for q in params)
    measure({"batch_c1": batch(vids), "seq_loop_c1": loop(vids), "batch_c3": batch(vids3), "seq_loop_c3": loop(vids3)},
            {"batch_c1": 2 * steps, "seq_loop_c1": 3 * updates, "batch_c3": 2 * steps, "seq_loop_c3": 3 * updates},
            max(2, args.calls // 10), what="batch", videos=27, size="480x640", mhi_updates=updates)

    lab = torch.tensor([q[3] for q in params], dtype=torch.int32, device="cuda")
    grp = torch.tensor([q[4] for q in params], dtype=torch.int32, device="cuda")

    def chain():
        M = torch.stack([m[0] for m in loop(vids)()])
        E = torch.stack([mhi.energyFromHistory(m) for m in M])
        mu, eta, _ = moments.centralMomentsBatch(M, normInf=True)
        moments.centralMomentsBatch(E)
        matching.naiveConfusionMatrix(mu, lab)
        matching.naiveConfusionMatrix(eta, lab)
        return matching.confusionMatrix(mu, lab, grp, 3)

    measure({"run_problem2": lambda: ps7.runProblem2(vids, cfg), "separate_calls": chain}, {}, max(2, args.calls // 10),
            what="problem2", videos=27, size="480x640", mhi_updates=updates)
    write(args.out, out_rows)


def write(path, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
