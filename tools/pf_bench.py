"""Time the ps6 particle filter (csrc/pf.hip) on 480 x 640 x 3 frames with the head model (129 x 104, pfconf1) and
the hand model (87 x 73, pfconf2 / pfconf3_hand): the device-resident tick (micv_pf_tick_dev, frames already on the
device), the sequence entry on host frames (micv_pf_track_seq_host, ms per frame, uploads included), and the exact
numpy restatement tests/_pf_ref.py on one CPU thread for scale.  Prints one JSON line per case.
    python tools/pf_bench.py [--ticks 200] [--ref-ticks 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frames_for(seed, count, obj):
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    tex = rng.integers(0, 256, obj + (3,), dtype=np.uint8)
    out = []
    for t in range(count):
        f = bg.copy()
        y, x = 150 + (t % 40), 250 + 2 * (t % 40)
        f[y:y + obj[0], x:x + obj[1]] = tex
        out.append(f)
    return out, tex, (250.0, 150.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--ref-ticks", type=int, default=2)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    import _pf_ref as ref
    from introtocomputervision_amd import pf
    cases = [("head", (129, 104), pf.MEAN_SQ_ERR, 300, 3.0, 6.5), ("hand", (87, 73), pf.MEAN_SQ_ERR, 700, 1.5, 28.0),
             ("head", (129, 104), pf.MEAN_SHIFT_LT, 300, 0.0, 4.7), ("hand", (87, 73), pf.MEAN_SHIFT_LT, 700, 0.0, 28.0)]
    for name, obj, mode, n, mse_sigma, dyn in cases:
        frames, tex, init = frames_for(7, 40, obj)
        dframes = [torch.from_numpy(f).cuda() for f in frames]
        g = pf.ParticleFilter(tex, (640, 480), n, mode, mse_sigma, dyn, init)
        for t in range(10):
            g.tick(dframes[t % len(dframes)])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(a.ticks):
            g.tick(dframes[t % len(dframes)])
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.ticks
        g2 = pf.ParticleFilter(tex, (640, 480), n, mode, mse_sigma, dyn, init)
        g2.track(frames[:4])
        t0 = time.perf_counter()
        g2.track(frames)
        seq_ms = (time.perf_counter() - t0) * 1e3 / len(frames)
        r = ref.PF(tex, 480, 640, n, mode, mse_sigma, dyn, init)
        t0 = time.perf_counter()
        for t in range(a.ref_ticks):
            r.tick(frames[t])
        ref_ms = (time.perf_counter() - t0) * 1e3 / a.ref_ticks
        print(json.dumps({"model": name, "patch": list(obj) + [3], "mode": "MSE" if mode == pf.MEAN_SQ_ERR else "HIST",
                          "n": n, "tick_dev_ms": round(dev_ms, 4), "seq_host_ms_per_frame": round(seq_ms, 4),
                          "cpu_numpy_ref_ms_per_tick": round(ref_ms, 1)}), flush=True)
        g.close()
        g2.close()


if __name__ == "__main__":
    main()
