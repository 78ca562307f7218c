#!/usr/bin/env python
"""Median wall time of choosing q points to evaluate in parallel, two ways:

    --mode batch   ONE bohip_gp_select_batch call (constant liar = max y)
    --mode loop    what a caller had to do before: q rounds of value-only bohip_gp_score + bohip_gp_append of the fantasised
                   observation on a SCRATCH handle (its construction is not timed) -- works with any library build.  (Nothing
                   keeps such a loop from proposing the same candidate again; masking earlier picks would need all R scores
                   on the host every round.  The time is what is compared.)
    --mode score   the value-only bohip_gp_score call alone, the yardstick of q = 1 -- any library build

BOHIP_LIB selects the library build, so the loop of an older build and the batch call of this one can be alternated A/B on one
box.  Shapes: the bench shape (N = 3000, d = 8, R = 4096) at q = 1, 2, 8, 32 and C4 (N = 10000, d = 16, R = 4096) at q = 8;
--big adds one batch call at C4 with R = 32768 (2.7 GB of V').

    python tools/time_batch_select.py --mode batch [--reps 30] [--once]     (--once: one call per shape, for a kernel trace)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402

SHAPES = [("bench", 3000, 8, 4096, (1, 2, 8, 32)), ("C4", 10000, 16, 4096, (8,))]


def problem(N, d, R):
    rng = np.random.default_rng(3)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    Xs = np.asfortranarray(np.random.default_rng(4).random((R, d)).T)
    return X, y, Xs


def model(X, y, extra=0):
    N, d = X.shape
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0,
                         capacity=N + extra)
    m.append_(X.T, y)
    return m


def time_batch(m, tau, Xs, q, liar, reps):
    for _ in range(0 if reps == 1 else 5):
        m.select_batch("EI", tau, Xs, q, fantasy=liar)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx, val, _, _ = m.select_batch("EI", tau, Xs, q, fantasy=liar)
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3, idx


def time_loop(X, y, tau, Xs, q, liar, reps):
    ts = []
    for rep in range(reps + 1):                       # (the first repetition warms the library up and is dropped)
        m = model(X, y, extra=q)
        m.score("EI", tau, Xs, want_scores=False)     # buffers of the scoring pass exist before the clock starts
        picks = []
        t0 = time.perf_counter()
        for _ in range(q):
            _, _, i = m.score("EI", tau, Xs, want_scores=False)
            m.append_(Xs[:, i], [liar])
            picks.append(i)
        if rep:
            ts.append(time.perf_counter() - t0)
        m.close()
    return np.array(ts) * 1e3, np.array(picks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batch", "loop", "score"), required=True)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--shapes", default="bench,C4")
    a = ap.parse_args()
    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    if a.mode != "batch":   # an older build has no bohip_gp_select_batch: bind what it exports (the loop needs score and append only)
        import ctypes
        from bohip import _lib
        have = ctypes.CDLL(_lib.LIB_PATH)
        for sym in [k for k in _lib.SIGNATURES if not hasattr(have, k)]:
            del _lib.SIGNATURES[sym]
    for name, N, d, R, qs in SHAPES:
        if name not in a.shapes.split(","):
            continue
        X, y, Xs = problem(N, d, R)
        tau, liar = [float(y.max())], float(y.max())
        reps = 1 if a.once else (a.reps if N <= 3000 else max(3, a.reps // 6))
        m = model(X, y) if a.mode != "loop" else None
        if a.mode == "score":
            for _ in range(40):
                m.score("EI", tau, Xs, want_scores=False)
            ts = []
            for _ in range(2 * reps):
                t0 = time.perf_counter()
                _, v, i = m.score("EI", tau, Xs, want_scores=False)
                ts.append(time.perf_counter() - t0)
            ts = np.array(ts) * 1e3
            print(f"{lib:22s} score {name:5s} N={N} R={R}       median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  pick {i}", flush=True)
            m.close()
            continue
        for q in qs:
            ts, picks = time_batch(m, tau, Xs, q, liar, reps) if a.mode == "batch" else time_loop(X, y, tau, Xs, q, liar, reps)
            print(f"{lib:22s} {a.mode:5s} {name:5s} N={N} R={R} q={q:2d}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  "
                  f"picks {picks[:4].tolist()}", flush=True)
        if a.big and a.mode == "batch" and name == "C4":
            _, _, Xb = problem(N, d, 32768)
            ts, picks = time_batch(m, tau, Xb, 8, liar, 1 if a.once else 3)
            print(f"{lib:22s} batch {name:5s} N={N} R=32768 q= 8  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  "
                  f"picks {picks[:4].tolist()}  launches {m.info(8)}", flush=True)
        if m is not None:
            m.close()


if __name__ == "__main__":
    main()
