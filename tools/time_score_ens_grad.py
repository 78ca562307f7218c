#!/usr/bin/env python
"""Median wall time of the gradient of one acquisition averaged over H hyper-parameter settings, three ways on the
same model, alternated call by call in one process:

    cold    model.score_ensemble_grad("EI", tau, Xs, Theta) with a Theta the handle has not just factored (two Thetas that differ in
            one entry by 1e-9 take turns): bohip_gp_score_ens_grad with its factor and alpha stages
    reused  the same call again with the same Theta: the factors left on the handle serve it (what every step of an ascent but the
            first costs)
    loop    H times set_params_ + score_grad on the resident model, then the model's own parameters again -- the only thing a user
            could do before: H refits per gradient

and the stage times of the cold and the reused call from the handle's timing facility (ens_factor, ens_alpha, ens_grad, ens_reduce:
medians of the per-call sums over a second set of calls, so the events do not sit inside the wall-clock figures).

Shapes (N, H, R): (64, 16, 16), (256, 32, 16), (512, 32, 16), (512, 32, 1024); d = 8, SEArd; settings within +-0.5 of the model's own.

    python tools/time_score_ens_grad.py [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_joint_draw import model, problem  # noqa: E402
from time_score_ens import settings, spread  # noqa: E402

SHAPES, D = ((64, 16, 16), (256, 32, 16), (512, 32, 16), (512, 32, 1024)), 8


def loop(m, Theta, p, Xs):
    own = (m.kernel.ll.copy(), m.kernel.lsigma, m.logNoise, m.mean.beta)
    acc = np.zeros(Xs.shape)
    for t in Theta:
        m.set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
        acc += m.score_grad("EI", p, Xs)[1] / len(Theta)
    m.set_params_(ll=own[0], lsigma=own[1], logNoise=own[2], beta=own[3])
    return acc


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stage_sums(m):
    call = {}
    for name, ms in m.timing():
        call[name] = call.get(name, 0.0) + ms
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for N, H, R in SHAPES:
        X, y, Xs = problem(N, D, R)
        m = model(X, y)
        p = [float(np.median(y))]
        two = [settings(H), settings(H)]
        two[1][0, 0] += 1e-9
        rows = {"cold": [], "reused": [], "loop": []}
        for i in range(3 + a.reps):                                 # 3 warm-up rounds, then the timed ones: cold, reused, loop in turn
            T = two[i % 2]
            tc, (_, g_cold) = clock(lambda: m.score_ensemble_grad("EI", p, Xs, T))
            tr, (_, g_reuse) = clock(lambda: m.score_ensemble_grad("EI", p, Xs, T))
            tl, g_loop = clock(lambda: loop(m, T, p, Xs))
            assert np.array_equal(g_cold, g_reuse)
            if i >= 3:
                rows["cold"].append(tc)
                rows["reused"].append(tr)
                rows["loop"].append(tl)
        err = np.max(np.abs(g_cold - g_loop)) / np.max(np.abs(g_loop))
        med = {k: np.median(v) for k, v in rows.items()}
        for k in ("cold", "reused", "loop"):
            print(f"N={N:4d} H={H:3d} R={R:5d}  {k:6s} {spread(np.array(rows[k]))}", flush=True)
        print(f"N={N:4d} H={H:3d} R={R:5d}  ratios of medians: reused / cold {med['reused'] / med['cold']:6.3f}   loop / cold {med['loop'] / med['cold']:6.2f}   "
              f"loop / reused {med['loop'] / med['reused']:6.2f}   max |difference| of the two routes' gradients / max |gradient| {err:.1e}", flush=True)
        m.enable_timing(True)
        st = {"cold": {}, "reused": {}}
        for i in range(a.reps):
            T = two[i % 2]
            for k in ("cold", "reused"):
                m.score_ensemble_grad("EI", p, Xs, T)
                for name, ms in stage_sums(m).items():
                    st[k].setdefault(name, []).append(ms)
        m.enable_timing(False)
        for k in ("cold", "reused"):
            print(f"N={N:4d} H={H:3d} R={R:5d}  stages {k:6s} " + "  ".join(f"{n} {np.median(v):8.3f} ms" for n, v in sorted(st[k].items())), flush=True)
        m.close()


if __name__ == "__main__":
    main()
