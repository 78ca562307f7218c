#!/usr/bin/env python
"""Passes and wall time of the device ascent (model.ascend = bohip_gp_acquire_max) under ExpectedImprovement and under
LogExpectedImprovement from the SAME ten starts, and the textbook EI (= exp(LogEI), from the host functor on predict_f) at the
point each returns.  Two workloads:

    flank   the N = 600, d = 3 model of tools/ascent_kkt_margin.py (profiles/r06_ascent_kkt_margin.txt), tau = median y, where EI
            crawls down exponential flanks for some start seeds; seeds 41 .. 52, tolerances 1e-13 as there
    bench   the bench model (N = 3000, d = 8, SEArd, length 0.5) at tau = max y, default tolerances; seeds 1 .. 6

Numbers are recorded (profiles/logei_ascent.txt), not asserted.

    python tools/time_logei_ascent.py [--reps 3] > profiles/logei_ascent.txt
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synth(N, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    return X, y


def run(bohip, name, m, d, tau, seeds, reps, tol):
    lb, ub = np.zeros(d), np.ones(d)
    le = bohip.LogExpectedImprovement(tau)
    print(f"== {name}: tau = {tau:.6g}, ten starts per seed, best of {reps} timings")
    print(f"{'seed':>4s} | {'EI passes':>9s} {'ms':>8s} {'textbook EI at x*':>18s} | {'LogEI passes':>12s} {'ms':>8s} {'textbook EI at x*':>18s}")
    tot = {"EI": [0, 0.0], "LogEI": [0, 0.0]}
    for seed in seeds:
        starts = np.asfortranarray(np.random.default_rng(seed).random((d, 10)))
        cells = []
        for acq in ("EI", "LogEI"):
            best_t = math.inf
            for _ in range(reps):
                t0 = time.perf_counter()
                f, X, bf, bi, bx, ev = m.ascend(acq, [tau], lb, ub, starts, maxeval=2000, ftol_rel=tol, xtol_abs=tol)
                best_t = min(best_t, time.perf_counter() - t0)
            mu, var = m.predict_f(bx)
            ei = math.exp(le(float(mu[0]), float(var[0]))) if bi >= 0 else float("nan")
            tot[acq][0] += ev
            tot[acq][1] += best_t
            cells.append(f"{ev:{9 if acq == 'EI' else 12}d} {best_t * 1e3:8.2f} {ei:18.10e}")
        print(f"{seed:4d} | " + " | ".join(cells))
    print(f"sum  | EI {tot['EI'][0]} passes, {tot['EI'][1] * 1e3:.1f} ms | LogEI {tot['LogEI'][0]} passes, {tot['LogEI'][1] * 1e3:.1f} ms"
          f" | passes LogEI / EI = {tot['LogEI'][0] / max(tot['EI'][0], 1):.3f}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import bohip

    X, y = synth(600, 3, 40)
    m = bohip.ElasticGPE(3, mean=bohip.MeanConst(0.2), kernel=bohip.SEArd(np.array([-0.9, -0.6, -0.75]), 0.1), logNoise=-2.0, capacity=600)
    m.append_(X.T, y)
    run(bohip, "flank (N = 600, d = 3)", m, 3, float(np.median(y)), range(41, 53), args.reps, 1e-13)
    m.close()
    X, y = synth(3000, 8, 0)
    m = bohip.ElasticGPE(8, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(8, math.log(0.5)), 0.0), logNoise=-2.0, capacity=3000)
    m.append_(X.T, y)
    run(bohip, "bench model (N = 3000, d = 8)", m, 8, float(y.max()), range(1, 7), args.reps, 1e-10)
    m.close()


if __name__ == "__main__":
    main()
