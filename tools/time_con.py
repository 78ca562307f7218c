#!/usr/bin/env python
"""Times of a constrained score: ConstrainedGPE.score at N = 3000, d = 8, C = 2, R = 1024 and 4096 -- the value call and
the gradient call with their stage times -- against what a caller had before it: (C + 1) x predict_f plus the NumPy combine, and
(C + 1) x score_grad.

    python tools/time_con.py [--reps 20] [--rounds 3] [--parent DIR]   every case, each in a child process of its own under a time
                                                                        limit, "con" and "base" alternating; the first child that
                                                                        fails ends the run.  --parent: a checkout of the parent
                                                                        commit (built) to take the base figures from; default: this tree
    python tools/time_con.py --case con:4096 [--reps 20]                one case, in this process
    python tools/time_con.py --case base:4096 --tree DIR                the base case importing bohip from DIR

The value call should cost no more than 1.1 x the (C + 1) predict calls: it runs the same posterior launches, on (C + 1) streams, and
the combine streams (C + 1) x 16 bytes a candidate."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, C_ = 3000, 8, 2
THR, SENSES = [0.2, 0.6], [1, -1]


def members(bohip):
    ms = []
    for i in range(C_ + 1):
        rng = np.random.default_rng(3 + i)
        X = rng.random((N, D))
        y = np.sin(3 * X + i).sum(1) + 0.1 * rng.standard_normal(N)
        m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
        m.append_(X.T, y - (np.median(y) if i else 0.0))
        ms.append(m)
    return ms


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


def one_case(case, reps, tree):
    sys.path.insert(0, tree)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import bohip

    kind, R = case.split(":")
    R = int(R)
    Xs = np.asfortranarray(np.random.default_rng(4).random((D, R)))
    ms = members(bohip)
    tau = float(np.median(ms[0].y))
    if kind == "con":
        cm = bohip.ConstrainedGPE(ms[0], ms[1:], THR, SENSES)
        val = timed(lambda: cm.score("LogEI", [tau], Xs, want_moments=False), reps)
        grd = timed(lambda: cm.score("LogEI", [tau], Xs, want_grad=True, want_moments=False), reps)
        print(f"con  N={N} d={D} C={C_} R={R:4d}  value call median {np.median(val):7.3f} ms  min {val.min():7.3f}   "
              f"gradient call median {np.median(grd):7.3f} ms  min {grd.min():7.3f}", flush=True)
        for name, g in (("value", False), ("gradient", True)):
            st = stages(ms, lambda: cm.score("LogEI", [tau], Xs, want_grad=g, want_moments=False), reps)
            print(f"    {name} stages (model:stage, ms)  " + "  ".join(f"{n} {t:.3f}" for n, t in st), flush=True)
    else:
        import con_reference as cr

        def predicts():
            mv = [m.predict_f(Xs) for m in ms]
            return np.array([a for a, _ in mv]), np.array([b for _, b in mv])

        def with_twin():
            mu, var = predicts()
            return cr.combine("LogEI", [tau], THR, SENSES, mu, var)

        pr = timed(predicts, reps)
        tw = timed(with_twin, reps)
        sg = timed(lambda: [m.score_grad("LogEI", [tau], Xs) for m in ms], reps)
        print(f"base N={N} d={D} C={C_} R={R:4d}  {C_ + 1} x predict_f median {np.median(pr):7.3f} ms  min {pr.min():7.3f}   "
              f"+ NumPy combine median {np.median(tw):7.3f} ms   {C_ + 1} x score_grad median {np.median(sg):7.3f} ms  min {sg.min():7.3f}"
              f"   [{os.path.relpath(tree, ROOT)}]", flush=True)
    for m in ms:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=ROOT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a case's child process may take")
    a = ap.parse_args()
    if a.case:
        one_case(a.case, a.reps, os.path.abspath(a.tree))
        return 0
    for _ in range(a.rounds):
        for R in (1024, 4096):
            for case, tree in ((f"con:{R}", ROOT), (f"base:{R}", os.path.abspath(a.parent))):
                rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case,
                                      "--tree", tree, "--reps", str(a.reps)])
                if rc != 0:
                    print(f"case {case} ended with status {rc}; nothing more is started", flush=True)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
