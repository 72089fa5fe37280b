"""Time one RANSAC solve per call (micv_ransac_solve_dev / _host) at the reference's sizes and larger, with the
exact Python restatement's CPU time for scale.  Every iteration runs (min_ratio 1.0 is never reached), so the
work per call is fixed: iters hypotheses x N point tests.  Prints one JSON line per case.
    python tools/ransac_bench.py [--reps 20]"""
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
    a = ap.parse_args()
    import torch
    import _ransac_pin as pin
    import _ransac_ref as rr
    from introtocomputervision_amd import ransac
    from introtocomputervision_amd._capi import check, lib
    from introtocomputervision_amd.match import _host_ctx
    h = _host_ctx().handle
    stream = torch.cuda.current_stream().cuda_stream
    for tt, n, iters in [(1, 117, 2000), (2, 78, 2000), (3, 78, 2000), (1, 4096, 2000), (3, 4096, 2000),
                         (1, 65536, 2000), (3, 65536, 2000)]:
        src, dst, _, _ = pin.synth(tt, n, n // 2, 7)
        s = ransac.Generator(pin.PS4_SEED_WORDS).samples(n, tt, iters)
        ds, dd, dsm = (torch.from_numpy(x).cuda() for x in (src, dst, s))
        tr = torch.empty(12, device="cuda")
        mk = torch.empty(n, dtype=torch.uint8, device="cuda")
        st = torch.empty(3, dtype=torch.int32, device="cuda")

        def dev():
            check(lib.micv_ransac_solve_dev(h, ds.data_ptr(), dd.data_ptr(), n, dsm.data_ptr(), iters, tt, 6, 1.0,
                                            tr.data_ptr(), mk.data_ptr(), st.data_ptr(), stream))
        htr, hmk, hst = np.empty(12, np.float32), np.empty(n, np.uint8), np.empty(3, np.int32)

        def host():
            check(lib.micv_ransac_solve_host(h, src.ctypes.data, dst.ctypes.data, n, s.ctypes.data, iters, tt, 6, 1.0,
                                             htr.ctypes.data, hmk.ctypes.data, hst.ctypes.data))
        for _ in range(3):
            dev()
            host()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            dev()
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.reps
        t0 = time.perf_counter()
        for _ in range(a.reps):
            host()
        host_ms = (time.perf_counter() - t0) * 1e3 / a.reps
        ref_iters = iters if n * iters <= 1 << 24 else 100
        t0 = time.perf_counter()
        r = rr.solve_samples(src, dst, s[:ref_iters], tt, 6, ref_iters, 1.0)
        ref_ms = (time.perf_counter() - t0) * 1e3 * iters / ref_iters
        ok = hst.tolist() == [iters, r["best_iter"], r["best_count"]] if ref_iters == iters else None
        print(json.dumps(dict(type=tt, n=n, iters=iters, dev_ms=round(dev_ms, 4), host_ms=round(host_ms, 4),
                              python_ref_ms=round(ref_ms, 1), python_ref_scaled_from=ref_iters, agrees=ok)), flush=True)


if __name__ == "__main__":
    main()
