"""ps7 second half on the device: moments of ps7's batch (27 MHIs with NORM_INF + 27 MEIs, 7 orders) at 480x640 and
1080p, knn_confusion at N = 27 and N = 20 000, and a whole synthetic problem 2 (27 videos -> MHIs -> MEIs -> moments ->
the three confusion results), through the _dev (device events around a stream) and _host (host clock, synchronous)
entry points, plus the numpy restatement's single-thread CPU time on the same inputs (measured in full, not scaled).
One JSON line per measurement.  --only moments runs the moments batch alone (for a counter run).

    python tools/ps7_bench.py [--reps 20] [--out FILE] [--only moments|knn|problem2] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dev_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_ms(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("moments", "knn", "problem2"), default=None)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    import torch

    import _ps7_ref as ref
    from introtocomputervision_amd import matching, moments
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    rng = np.random.default_rng(7)
    for rows, cols in ((480, 640), (1080, 1920)) if args.only in (None, "moments") else ():
        mh = np.zeros((27, rows, cols), np.uint8)
        for b in range(27):
            for _ in range(8):
                y, x = rng.integers(0, rows - rows // 5), rng.integers(0, cols - cols // 5)
                mh[b, y:y + rows // 5, x:x + cols // 5] = rng.integers(1, 26)
        me = (mh > 0).astype(np.uint8)
        dm, de = torch.from_numpy(mh).cuda(), torch.from_numpy(me).cuda()

        def dev():
            moments.centralMomentsBatch(dm, normInf=True)
            moments.centralMomentsBatch(de)

        def host():
            moments.centralMomentsBatch(mh, normInf=True)
            moments.centralMomentsBatch(me)
        cpu = None
        if not args.no_numpy:
            t0 = time.perf_counter()
            for b in range(27):
                ref.central_moments(mh[b], norm_inf=True)
                ref.central_moments(me[b])
            cpu = (time.perf_counter() - t0) * 1e3
        emit(what="moments_ps7_batch", rows=rows, cols=cols, images=54, orders=7, dev_ms=dev_ms(dev, args.reps),
             host_ms=host_ms(host, max(2, args.reps // 4)), numpy_ms=cpu)
    for n in (27, 20000) if args.only in (None, "knn") else ():
        centres = rng.standard_normal((3, 7)).astype(np.float32) * 3
        lab = rng.integers(1, 4, n).astype(np.int32)
        f = (centres[lab - 1] + rng.standard_normal((n, 7)).astype(np.float32) * 2).astype(np.float32)
        grp = rng.integers(1, 4, n).astype(np.int32)
        df, dl, dg = (torch.from_numpy(a).cuda() for a in (f, lab, grp))
        d_naive = dev_ms(lambda: matching.naiveConfusionMatrix(df, dl), args.reps)
        d_group = dev_ms(lambda: matching.confusionMatrix(df, dl, dg, 3), args.reps)
        h_naive = host_ms(lambda: matching.naiveConfusionMatrix(f, lab), max(2, args.reps // 4))
        cpu = None
        if not args.no_numpy:
            t0 = time.perf_counter()
            ref.naive_confusion(f, lab)
            cpu = (time.perf_counter() - t0) * 1e3
        emit(what="knn_confusion", n=n, dims=7, k=3, naive_dev_ms=d_naive, group_dev_ms=d_group, naive_host_ms=h_naive,
             numpy_naive_ms=cpu)
    if args.only in (None, "problem2"):
        problem2(args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for kw in lines:
                fh.write(json.dumps(kw) + "\n")


def problem2(args, emit):
    """runProblem2 on 27 synthetic 480 x 640 videos with ps7.yaml's parameters and last frames, all on the device:
    mhi.historySequence per video, energyFromHistory, the two moment batches, the naive mu / eta matrices and the
    per-person matrices.  Device events around the whole chain (frames already resident); the restatement (oracle MHI +
    numpy) once, on one thread."""
    import torch

    import _ps7_ref as ref
    from introtocomputervision_amd import config, matching, mhi, moments
    cfg = config.load(os.path.join(ROOT, "tests", "golden", "config", "ref", "ps7.yaml"))
    last = config.last_frames(cfg)
    vids = []
    for a in (1, 2, 3):
        p = config.mhi_params(cfg, f"mhi_action{a}")
        for person in (1, 2, 3):
            for trial in (1, 2, 3):
                lf = last[f"PS7A{a}P{person}T{trial}"]
                fr = ref.action_video(1000 * a + 10 * person + trial, a, lf + 1, 480, 640)
                vids.append((torch.from_numpy(fr).cuda(), fr, p, lf, a, person))
    lab = torch.tensor([v[4] for v in vids], dtype=torch.int32, device="cuda")
    grp = torch.tensor([v[5] for v in vids], dtype=torch.int32, device="cuda")

    def chain():
        M = torch.stack([mhi.historySequence(d, p["diff_threshold"], p["pre_blur_size"], p["pre_blur_sigma"], p["tau"],
                                             [lf])[0] for d, _, p, lf, _, _ in vids])
        E = torch.stack([mhi.energyFromHistory(m) for m in M])
        mu, eta, _ = moments.centralMomentsBatch(M, normInf=True)
        moments.centralMomentsBatch(E)
        matching.naiveConfusionMatrix(mu, lab)
        matching.naiveConfusionMatrix(eta, lab)
        return matching.confusionMatrix(mu, lab, grp, 3)
    frames = sum(v[3] for v in vids)
    cpu = None
    if not args.no_numpy:
        t0 = time.perf_counter()
        mhis = [ref.history_seq(fr, p["diff_threshold"], p["pre_blur_size"], p["pre_blur_sigma"], p["tau"], [lf])[0]
                for _, fr, p, lf, _, _ in vids]
        mom = [ref.central_moments(m, norm_inf=True) for m in mhis]
        mu, eta = np.stack([r[0] for r in mom]), np.stack([r[1] for r in mom])
        for m in mhis:
            ref.central_moments(ref.mhi_energy(m))
        acts, ppl = [v[4] for v in vids], [v[5] for v in vids]
        ref.naive_confusion(mu, acts)
        ref.naive_confusion(eta, acts)
        ref.group_confusion(mu, acts, ppl, 3)
        cpu = (time.perf_counter() - t0) * 1e3
    emit(what="problem2", videos=27, rows=480, cols=640, mhi_updates=frames, dev_ms=dev_ms(chain, max(2, args.reps // 4)),
         numpy_ms=cpu, numpy_note="CPU oracle MHI + numpy restatement, one thread")


if __name__ == "__main__":
    main()
