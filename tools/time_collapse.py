#!/usr/bin/env python
"""Median wall time of the calls a Bayesian-optimisation loop makes, on a model that holds 600 positions evaluated 5 times each as
600 weighted sites (ElasticGPE(collapse=True)) beside the same model with its 3000 evaluations as rows of their own
(the route of every earlier build: the baseline).  d = 8, SEArd, R = 4096 candidates, EI.  Per model: fit_(), one score pass, one
mll_grad, and the append of one new position evaluated 5 times (5 rows on the expanded model, one site on the collapsed one), 30 calls
each.  Every call is blocking (it ends in a stream synchronisation), so a host clock around it is the call's time.  The two models
alternate three times in one process, each round on fresh handles; a figure's spread is the range of its three round medians.  The
stage events of one call of each kind follow.

    python tools/time_collapse.py [--reps 30] [--rounds 3] > profiles/rep_collapse.txt
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402

SITES, REPS, D, R = 600, 5, 8, 4096
CALLS = ("fit_", "score", "mll_grad", "append")


def problem(reps_append):
    rng = np.random.default_rng(0)
    pos = rng.random((SITES + reps_append, D))
    X = np.repeat(pos, REPS, axis=0)
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(len(X))
    return X, y, np.asfortranarray(rng.random((D, R)))


def make(collapse, X, y):
    m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0,
                         capacity=1024 if collapse else 4096, collapse=collapse)   # (each sized for what it holds)
    n0 = SITES * REPS
    bohip.update_(m, X[:n0].T, y[:n0])
    return m


def one_round(collapse, X, y, xs, reps, stages):
    m = make(collapse, X, y)
    n0, tau = SITES * REPS, [float(y[:SITES * REPS].max())]
    assert (m.nobs, m.nevals) == ((SITES, n0) if collapse else (n0, n0))
    k = [0]

    def append():
        lo = n0 + REPS * k[0]
        k[0] += 1
        bohip.update_(m, X[lo:lo + REPS].T, y[lo:lo + REPS])

    calls = dict(fit_=m.fit_, score=lambda: m.score("EI", tau, xs, want_scores=False), mll_grad=m.mll_grad, append=append)
    out = {}
    for name in CALLS[:3]:
        fn = calls[name]
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = float(np.median(ts))
    ts = []
    for _ in range(reps):                                         # (no warm-up: every append is a new row; the first pays what the others pay)
        t0 = time.perf_counter()
        append()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["append"] = float(np.median(ts))
    if stages is not None:
        m.enable_timing(True)
        for name in CALLS:
            calls[name]()
            if name != "mll_grad":                                # (mll_grad does not publish its stage events)
                stages[name] = ", ".join(f"{s} {ms:.3f}" for s, ms in m.timing())
        m.enable_timing(False)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    X, y, xs = problem(a.reps + len(CALLS))
    res = {True: [], False: []}
    stages = {True: {}, False: {}}
    for r in range(a.rounds):
        for collapse in (True, False):
            res[collapse].append(one_round(collapse, X, y, xs, a.reps, stages[collapse] if r == a.rounds - 1 else None))
            print(f"round {r + 1} {'collapsed' if collapse else 'expanded '}: " +
                  "  ".join(f"{n} {res[collapse][-1][n]:8.3f} ms" for n in CALLS), flush=True)
    print(f"\n{SITES} sites x {REPS} = {SITES * REPS} evaluations, d = {D}, R = {R}, EI; medians of {a.reps} calls, {a.rounds} rounds: "
          "median of the round medians [their range]")
    for n in CALLS:
        c, e = np.array([x[n] for x in res[True]]), np.array([x[n] for x in res[False]])
        sc, se = c.max() - c.min(), e.max() - e.min()
        verdict = "faster" if np.median(c) <= np.median(e) else ("within the spread" if np.median(c) - np.median(e) <= max(sc, se) else "SLOWER")
        print(f"{n:9s} collapsed {np.median(c):8.3f} ms [{sc:6.3f}]   expanded {np.median(e):8.3f} ms [{se:6.3f}]   "
              f"expanded / collapsed = {np.median(e) / np.median(c):6.2f}   collapsed is {verdict}")
    for collapse in (True, False):
        for n, s in stages[collapse].items():
            print(f"stages ({'collapsed' if collapse else 'expanded'}) {n}: {s} ms")


if __name__ == "__main__":
    main()
