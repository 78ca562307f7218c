#!/usr/bin/env python
"""Median wall time of leave-one-out cross-validation on the resident model beside the marginal likelihood's
gradient of the same build: loo(), loo_grad() and mll_grad() at N = 256, 3000 and 10^4 (d = 8, SEArd).  Every call is blocking
(it ends in a stream synchronisation), so a host clock around it is the call's time.  The three calls alternate inside one loop,
after a warm-up of each; then one loo_grad with the stage events on gives its split by stage.

    python tools/time_loo.py [--reps 30] > profiles/loo_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402,F401
from time_joint_draw import model, problem  # noqa: E402

SIZES, D = (256, 3000, 10000), 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    for N in SIZES:
        X, y, _ = problem(N, D, 1)
        m = model(X, y)
        calls = (("loo", m.loo), ("loo_grad", m.loo_grad), ("mll_grad", m.mll_grad))
        for _, fn in calls:
            for _ in range(3):
                fn()
        ts = {name: [] for name, _ in calls}
        for _ in range(a.reps):
            for name, fn in calls:
                t0 = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        base = np.median(ts["mll_grad"])
        for name, _ in calls:
            v = np.array(ts[name])
            print(f"N={N:6d} {name:9s} median {np.median(v):9.3f} ms  min {v.min():9.3f} ms  max {v.max():9.3f} ms  = {np.median(v) / base:5.2f} x mll_grad", flush=True)
        m.enable_timing(True)
        m.loo_grad()                                              # ("kinv" is the launch mll_grad pays too)
        print(f"N={N:6d} loo_grad  stages: " + ", ".join(f"{s} {ms:.3f} ms" for s, ms in m.timing()), flush=True)
        m.enable_timing(False)
        m.close()


if __name__ == "__main__":
    main()
