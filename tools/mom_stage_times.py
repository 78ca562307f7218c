#!/usr/bin/env python
"""Times of a score with three and four objectives from the handles' stage timers: bohip_gp_score_mom at N = 3000,
d = 8, R = 4096 and R = 10 (the ascent's case), for M = 3 over fronts of 16, 64 and 256 points and M = 4 over fronts of 16 and 48
points -- the box count, the mom_ehvi stage in its value and gradient forms, and the whole call beside M bohip_gp_predict (value
form) or bohip_gp_predict_grad (gradient form) calls made one after the other in the same process.

    python tools/mom_stage_times.py [--reps 20] [--out FILE]

One process, every case in turn; whole-call times are host clocks around calls that end in a device synchronise, medians of `reps`
calls after 3 warm-up calls; stage times are medians of the handles' event timers over `reps` further calls."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 3000, 8
CASES = ((3, 16), (3, 64), (3, 256), (4, 16), (4, 48))


def members(bohip, M):
    ms = []
    for i, kern in enumerate((bohip.SEArd, bohip.Mat52Ard, bohip.Mat32Ard, bohip.SEArd)[:M]):
        rng = np.random.default_rng(3 + i)
        X = rng.random((N, D))
        y = np.sin(3 * X + i).sum(1) + 0.1 * rng.standard_normal(N)
        m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=kern(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
        m.append_(X.T, y)
        ms.append(m)
    return ms


def a_front(M, n, lo, hi, seed=0):
    """n mutually non-dominated points inside [lo, hi] of each objective (lo + (hi - lo) u, u on the unit sphere's positive orthant);
    ref below lo."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.2, 1.0, (n, M))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    lo, hi = np.asarray(lo), np.asarray(hi)
    return np.ascontiguousarray((lo + (hi - lo) * u).T), lo - 0.5


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3


def stages(ms, fn, reps):
    for m in ms:
        m.enable_timing(True)
    fn()
    rows = []
    for _ in range(reps):
        fn()
        rows.append([(f"{i}:{n}", t) for i, m in enumerate(ms) for n, t in m.timing()])
    for m in ms:
        m.enable_timing(False)
    names = []
    for n, _ in rows[0]:
        if n not in names:
            names.append(n)
    return [(n, float(np.median([sum(t for k, t in r if k == n) for r in rows]))) for n in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bohip

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    all_ms = members(bohip, 4)
    say(f"score with M objectives, N = {N}, d = {D}, members SEArd, Mat52Ard, Mat32Ard, SEArd, medians of {a.reps} calls, ms")
    for R in (4096, 10):
        Xs = np.asfortranarray(np.random.default_rng(4).random((D, R)))
        for M in (3, 4):
            ms = all_ms[:M]
            pg = timed(lambda: [m.predict_grad(Xs) for m in ms], a.reps)
            pf = timed(lambda: [m.predict_f(Xs) for m in ms], a.reps)
            say(f"R = {R} M = {M}: {M} predict_grad calls one after the other {np.median(pg):.3f} (min {pg.min():.3f}); {M} predict_f calls "
                f"{np.median(pf):.3f} (min {pf.min():.3f})")
            ys = [np.asarray(m.y) for m in ms]
            lo, hi = [float(np.quantile(y, 0.5)) for y in ys], [float(y.max()) for y in ys]
            for n_front in [n for mm, n in CASES if mm == M]:
                fr, ref = a_front(M, n_front, lo, hi, seed=n_front)
                nbox = bohip.mom_boxes(fr, ref)[1].shape[1]
                for name, g in (("value", False), ("gradient", True)):
                    call = lambda: bohip.score_mom(ms, fr, ref, Xs, want_grad=g, want_moments=False)   # noqa: E731
                    whole = timed(call, a.reps)
                    st = stages(ms, call, a.reps)
                    ehvi = sum(t for n, t in st if n.endswith(":mom_ehvi"))
                    post = [sum(t for n, t in st if n.startswith(f"{i}:") and not n.endswith(":mom_ehvi")) for i in range(M)]
                    say(f"R = {R} M = {M} n_front = {n_front:3d} boxes = {nbox:5d} {name:8s} call: whole {np.median(whole):.3f} "
                        f"(min {whole.min():.3f}); mom_ehvi {ehvi:.3f}; posterior stages per member " + ", ".join(f"{p:.3f}" for p in post))
    for m in all_ms:
        m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
