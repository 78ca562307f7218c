#!/usr/bin/env python
"""Wall and stage times of ONE greedy q-EHVI batch (bohip_gp_qehvi_batch) at S = 256, R = 4096, q = 8 over fronts of
n = 64 and n = 1024 points, two models of N = 1000, d = 4; beside it the draw stage alone (two sample_joint calls).  The stage split
is enable_timing's on the first objective's handle, summed per launch family.  BOHIP_QEHVI_NARROW=0 / 1 (read once per process)
selects the full walk or the wave-union walk of k_qehvi_gain: run the script once with each to compare; the picks must agree.

    BOHIP_QEHVI_NARROW=1 python tools/time_qehvi.py [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, R, S, Q = 1000, 4, 4096, 256, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    reps = ap.parse_args().reps
    import bohip
    from bohip import _lib

    lib = _lib.load()
    rng = np.random.default_rng(3)
    X = rng.random((D, N))
    ys = [np.sin(3 * X).sum(0) + 0.1 * rng.standard_normal(N), np.cos(3 * X).sum(0) + 0.1 * rng.standard_normal(N)]
    ms = []
    for y in ys:
        m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
        m.append_(X, y)
        ms.append(m)
    xs = np.asfortranarray(np.random.default_rng(4).random((D, R)))
    dp, ref = C.POINTER(C.c_double), np.array([-4.0, -4.0])
    idx, gain = np.zeros(Q, dtype=np.int64), np.zeros(Q)

    def med(fn):
        fn()
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    draw_ms = med(lambda: [m.sample_joint(xs, S, 5 + i, want_samples=False) for i, m in enumerate(ms)])
    for n in (64, 1024):
        t = (np.arange(n) + 0.5) / n                                             # a front through the cloud of the draws
        front = np.ascontiguousarray(np.stack([-3.0 + 5.0 * t, 2.0 - 5.0 * t ** 1.5]))

        def batch():
            _lib.check(lib.bohip_gp_qehvi_batch(ms[0]._h, ms[1]._h, front.ctypes.data_as(dp), n, ref.ctypes.data_as(dp),
                                                xs.ctypes.data_as(dp), R, S, 5, 1e-12, 40, Q, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                gain.ctypes.data_as(dp), None, None, None))

        wall = med(batch)
        ms[0].enable_timing(True)
        batch()
        rows = []
        for _ in range(reps):
            batch()
            rows.append(ms[0].timing(256))
        ms[0].enable_timing(False)
        names = list(dict.fromkeys(k for k, _ in rows[0]))
        stages = {k: float(np.median([sum(v for kk, v in r if kk == k) for r in rows])) for k in names}
        print(json.dumps(dict(narrow=os.environ.get("BOHIP_QEHVI_NARROW", "default"), n_front=n, S=S, R=R, q=Q, wall_ms=wall,
                              two_sample_joint_ms=draw_ms, stages_ms=stages, idx=idx.tolist(), gain_sum=float(gain.sum()))), flush=True)


if __name__ == "__main__":
    main()
