#!/usr/bin/env python
"""Median wall time of one acquisition averaged over H hyper-parameter settings, two ways on the same model:

    ensemble   model.score_ensemble("EI", tau, Xs, Theta): bohip_gp_score_ens, all settings in one call, the model untouched
    loop       H times set_params_ + score on the resident model, then the model's own parameters again -- the only thing a user
               could do before: H refits, and a model that is left changed unless restored

and the stage times of the ensemble call from the handle's timing facility (ens_factor, ens_score, ens_reduce: medians of the
per-call sums over a second set of calls, so the events do not sit inside the wall-clock figures).

Shapes (N, H, R): (64, 16, 1024), (256, 32, 4096), (512, 32, 4096); d = 8, SEArd; settings within +-0.5 of the model's own.

    python tools/time_score_ens.py [--reps 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_joint_draw import model, problem, timed  # noqa: E402

SHAPES, D = ((64, 16, 1024), (256, 32, 4096), (512, 32, 4096)), 8


def settings(H):
    c = np.concatenate([[-2.0, 0.0], np.full(D, np.log(0.5)), [0.0]])
    return c + np.random.default_rng(H).uniform(-0.5, 0.5, (H, c.size))


def loop(m, Theta, p, Xs):
    own = (m.kernel.ll.copy(), m.kernel.lsigma, m.logNoise, m.mean.beta)
    acc = np.zeros(Xs.shape[1])
    for t in Theta:
        m.set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
        acc += m.score("EI", p, Xs)[0] / len(Theta)
    m.set_params_(ll=own[0], lsigma=own[1], logNoise=own[2], beta=own[3])
    return acc


def spread(ts):
    return f"median {np.median(ts):9.3f} ms  min {ts.min():9.3f}  p90 {np.percentile(ts, 90):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for N, H, R in SHAPES:
        X, y, Xs = problem(N, D, R)
        m = model(X, y)
        Theta, p = settings(H), [float(np.median(y))]
        te = timed(lambda: m.score_ensemble("EI", p, Xs, Theta), a.reps)
        tl = timed(lambda: loop(m, Theta, p, Xs), a.reps)
        res, ref = m.score_ensemble("EI", p, Xs, Theta), loop(m, Theta, p, Xs)
        err = np.max(np.abs(res.scores - ref) / np.maximum(np.abs(ref), 1e-12))
        print(f"N={N:4d} H={H:3d} R={R:5d}  ensemble {spread(te)}", flush=True)
        print(f"N={N:4d} H={H:3d} R={R:5d}  loop     {spread(tl)}   ratio of medians loop / ensemble {np.median(tl) / np.median(te):6.2f}   "
              f"max rel difference of the averages {err:.1e}", flush=True)
        m.enable_timing(True)
        rows = {}
        for _ in range(a.reps):
            m.score_ensemble("EI", p, Xs, Theta)
            call = {}
            for name, ms in m.timing():
                call[name] = call.get(name, 0.0) + ms
            for name, ms in call.items():
                rows.setdefault(name, []).append(ms)
        m.enable_timing(False)
        print(f"N={N:4d} H={H:3d} R={R:5d}  stages   " + "  ".join(f"{k} {np.median(v):8.3f} ms" for k, v in sorted(rows.items())), flush=True)
        m.close()


if __name__ == "__main__":
    main()
