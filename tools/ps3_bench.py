#!/usr/bin/env python3
"""ps3 calibration trials on the device: ms per call of micv_calib_ls_trials_dev (trial solve, residual and arg-min in one
call) for T = 30, 10 000 and 1 000 000 index subsets at k = 8 / 12 / 16 constraints on the 20 points of ps3 and at
k = 256 on 4096 synthetic points, float32 and float64 mode, device-resident (indices drawn by the device sampler), and
the numpy restatement (tests/_ps3_ref.py) on one CPU thread per trial.  Warm-up, then --reps timed groups of --inner
back-to-back calls between two device events, clock_ms = the median group / inner; one JSON line per case.
The T = 30 line is launch-bound: two launches and a 4-byte clear, a few tens of microseconds whatever the arithmetic.
  python tools/ps3_bench.py [--reps n] [--inner n] [--out file] [--no-numpy]"""
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

import _ps3_ref as R  # noqa: E402
from introtocomputervision_amd import geometry as g  # noqa: E402


def time_dev(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ms)), float(np.min(ms))


def direct_call(r2, r3, idx, k, j, T, f64):
    """micv_calib_ls_trials_dev on preallocated outputs: nothing but the library's own launches is timed."""
    from introtocomputervision_amd._capi import GEOM_F64, check, lib
    from introtocomputervision_amd.lk import _ctx_for
    dv = r2.device
    M = torch.empty((T, 12), dtype=torch.float32, device=dv)
    res = torch.empty(T, dtype=torch.float64, device=dv)
    bi = torch.empty(1, dtype=torch.int32, device=dv)
    br = torch.empty(1, dtype=torch.float64, device=dv)
    bm = torch.empty((1, 12), dtype=torch.float32, device=dv)
    st = torch.empty(1, dtype=torch.int32, device=dv)
    h = _ctx_for(r2, None).handle
    stream = torch.cuda.current_stream(dv).cuda_stream
    keep = (M, res, bi, br, bm, st)

    def fn():
        check(lib.micv_calib_ls_trials_dev(h, r2.data_ptr(), r3.data_ptr(), int(r2.shape[0]), idx.data_ptr(),
                                           int(idx.shape[1]), k, j, T, None, None, 0, GEOM_F64 if f64 else 0,
                                           M.data_ptr(), res.data_ptr(), bi.data_ptr(), br.data_ptr(), bm.data_ptr(),
                                           st.data_ptr(), stream))
    fn.keep = keep
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=0, help="calls per timed group (0: 50 for T <= 10 000, 3 above)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    P = R.load_all()
    big2, big3 = R.synth_camera(7, 4096, 0.5)
    sets = [("ps3 20 points", P["b"], P["p3"], (8, 12, 16)), ("4096 points", big2, big3, (256,))]
    lines = []
    for name, p2, p3, ks in sets:
        d2, d3 = torch.from_numpy(p2.T.copy()).cuda(), torch.from_numpy(p3.T.copy()).cuda()
        r2, r3 = g._rows(d2, 2, "pts2d"), g._rows(d3, 3, "pts3d")
        for k in ks:
            for T in (30, 10_000, 1_000_000):
                idx = g.sampleIndices(1234 + k, len(p2), k + 4, T)
                for f64 in (False, True):
                    inner = a.inner or (50 if T <= 10_000 else 3)
                    fn = direct_call(r2, r3, idx, k, 4, T, f64)
                    med, best = time_dev(fn, a.reps, inner)
                    rec = {"case": name, "k": k, "tests": 4, "T": T, "mode": "f64" if f64 else "f32",
                           "dev_ms_per_call": med, "dev_ms_min": best, "dev_us_per_trial": 1e3 * med / T,
                           "launch_bound": T == 30}
                    if not a.no_numpy:
                        Tn = min(T, 2000 if k <= 16 else 100)
                        sub = idx[:Tn].cpu().numpy()
                        t0 = time.perf_counter()
                        R.calib_ls_trials(p2, p3, sub, k, 4, f64=f64)
                        rec["numpy_trials_timed"] = Tn
                        rec["numpy_us_per_trial"] = 1e6 * (time.perf_counter() - t0) / Tn
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
                del idx
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
