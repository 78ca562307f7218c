#!/usr/bin/env python
"""Median wall time of value-only bohip_gp_score calls (host entry, one synchronisation per call) on problems that prune and on
problems that do not.  BOHIP_LIB selects the library build, so two builds can be compared A/B on one box.

    python tools/time_value_calls.py [--reps 60]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402

PROBLEMS = [  # name, N, d, log length scale, tau offset above max(y)
    ("bench shape (prunes)", 3000, 8, np.log(0.5), 0.0),
    ("d = 16, unit length scales", 3000, 16, 0.0, 0.0),
    ("tau = max(y) + 2 (EI ~ 0)", 3000, 8, np.log(0.5), 2.0),
    ("tau = max(y) + 100 (EI == 0: prunes nothing)", 3000, 8, np.log(0.5), 100.0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    a = ap.parse_args()
    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    for name, N, d, ll, off in PROBLEMS:
        rng = np.random.default_rng(3)
        X = rng.random((N, d))
        y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
        m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, ll), 0.0), logNoise=-2.0, capacity=N)
        m.append_(X.T, y)
        Xs = np.random.default_rng(4).random((4096, d)).T
        tau = [y.max() + off]
        for _ in range(40):
            m.score("EI", tau, Xs, want_scores=False)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, v, i = m.score("EI", tau, Xs, want_scores=False)
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts) * 1e3
        print(f"{lib:24s} {name:46s} median {np.median(ts):.3f} ms  mean {ts.mean():.3f} ms  best {v!r} @ {i}", flush=True)


if __name__ == "__main__":
    main()
