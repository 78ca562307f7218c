#!/usr/bin/env python
"""Times of a two-objective score from the handles' stage timers: bohip_gp_score_mo at N = 3000, d = 8, R = 4096 over
fronts of 16, 128 and 1024 points -- the mo_ehvi stage, the two members' posterior stages in the same call, and the whole call
against two bohip_gp_predict_grad calls made one after the other (what the second stream buys) -- and the mo_ehvi stage at R = 10,
the ascent's case.

    python tools/mo_stage_times.py [--reps 20] [--out FILE]

One process, every case in turn; whole-call times are host clocks around calls that end in a device synchronise, medians of `reps`
calls after 3 warm-up calls; stage times are medians of the handles' event timers over `reps` further calls."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 3000, 8


def members(bohip):
    ms = []
    for i, kern in enumerate((bohip.SEArd, bohip.Mat52Ard)):
        rng = np.random.default_rng(3 + i)
        X = rng.random((N, D))
        y = np.sin(3 * X + i).sum(1) + 0.1 * rng.standard_normal(N)
        m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=kern(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
        m.append_(X.T, y)
        ms.append(m)
    return ms


def a_front(n, lo, hi, seed=0):
    """n points ascending in f1 and descending in f2 inside [lo, hi] of each objective; ref below lo."""
    rng = np.random.default_rng(seed)
    f1 = np.sort(rng.uniform(lo[0], hi[0], n))
    f2 = -np.sort(-rng.uniform(lo[1], hi[1], n))
    return np.stack([f1, f2]), np.array([lo[0] - 0.5, lo[1] - 0.5])


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
    from bohip.model import score_mo

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ms = members(bohip)
    ys = [np.asarray(m.y) for m in ms]
    lo, hi = [float(np.quantile(y, 0.5)) for y in ys], [float(y.max()) for y in ys]
    say(f"two-objective score, N = {N}, d = {D}, members SEArd and Mat52Ard, medians of {a.reps} calls, ms")
    for R in (4096, 10):
        Xs = np.asfortranarray(np.random.default_rng(4).random((D, R)))
        pg = timed(lambda: [m.predict_grad(Xs) for m in ms], a.reps)
        pf = timed(lambda: [m.predict_f(Xs) for m in ms], a.reps)
        say(f"R = {R}: two predict_grad calls one after the other {np.median(pg):.3f} (min {pg.min():.3f}); two predict_f calls "
            f"{np.median(pf):.3f} (min {pf.min():.3f})")
        for n_front in (16, 128, 1024):
            fr, ref = a_front(n_front, lo, hi, seed=n_front)
            for name, g in (("value", False), ("gradient", True)):
                call = lambda: score_mo(ms[0], ms[1], fr, ref, Xs, want_grad=g, want_moments=False)   # noqa: E731
                whole = timed(call, a.reps)
                st = stages(ms, call, a.reps)
                ehvi = sum(t for n, t in st if n.endswith(":mo_ehvi"))
                post = [sum(t for n, t in st if n.startswith(f"{i}:") and not n.endswith(":mo_ehvi")) for i in range(2)]
                say(f"R = {R} n_front = {n_front:4d} {name:8s} call: whole {np.median(whole):.3f} (min {whole.min():.3f}); mo_ehvi {ehvi:.3f}; "
                    f"posterior stages member 0 {post[0]:.3f}, member 1 {post[1]:.3f}")
                say("    stages (member:stage) " + "  ".join(f"{n} {t:.3f}" for n, t in st))
    for m in ms:
        m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
