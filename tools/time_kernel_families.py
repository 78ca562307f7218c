#!/usr/bin/env python
"""Median wall time of the main entry points by covariance kernel (DESIGN.md "Matérn kernels"): N = 3000 observations, d = 8.
Each number is a host clock around one blocking call, after warm-up.  BOHIP_LIB selects the library build.

    python tools/time_kernel_families.py [--reps 25]

Columns: refit (kernel matrix + factorisation + alpha), value-only score of 4096 candidates (arg-max record only), one
small-batch value + gradient pass (R = 10), acquire_max (UCB, 10 starts)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402

KERNELS = ["SEArd", "Mat52Ard", "Mat32Ard", "Mat12Ard"]


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    N, d = 3000, 8
    rng = np.random.default_rng(3)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    Xs = np.random.default_rng(4).random((4096, d)).T
    X10 = np.random.default_rng(5).random((10, d)).T
    lb, ub = np.zeros(d), np.ones(d)
    starts = bohip.latin_hypercube_sampling(lb, ub, 10, np.random.default_rng(6))
    tau = [float(y.max())]
    print(f"{'kernel':10s} {'refit ms':>9s} {'score4096 ms':>13s} {'small pass ms':>14s} {'acquire_max ms':>15s}")
    for kern in KERNELS:
        m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=getattr(bohip, kern)(np.full(d, np.log(0.5)), 0.0),
                             logNoise=-2.0, capacity=N)
        m.append_(X.T, y)
        refit = median_ms(m.fit_, a.reps, 3)
        score = median_ms(lambda: m.score("EI", tau, Xs, want_scores=False), a.reps, 40)
        small = median_ms(lambda: m.score_grad("UCB", [2.0], X10), a.reps, 20)
        asc = median_ms(lambda: m.ascend("UCB", [2.0], lb, ub, starts), a.reps, 3)
        print(f"{kern:10s} {refit:9.3f} {score:13.3f} {small:14.3f} {asc:15.3f}", flush=True)
        m.close()


if __name__ == "__main__":
    main()
