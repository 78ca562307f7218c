"""Warm times of bohip_gp_score_pending_grad beside bohip_gp_score_pending and bohip_gp_score_grad on one model:
N = 3000, d = 8, R = 4096 and R = 10, (p, S) = (8, 0), (8, 64), (32, 1024).  The three calls ALTERNATE in one process: 5 warm-up
rounds, then the median (min) of 30 rounds of blocking calls; then the stage split of one call through the handle's timing, where
pend_weights (the fantasies over the lanes of a wave) stands beside pend_score (the same fantasies, a thread per candidate).
Usage: python tools/pending_grad_ab.py [out.txt]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bohip   # noqa: E402

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
N, d = 3000, 8
rng = np.random.default_rng(0)
X = rng.random((d, N))
y = np.sin(3 * X).sum(0) + 0.1 * rng.standard_normal(N)
m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
m.append_(X, y)
prm = [float(y.max())]


def split(fn):
    m.enable_timing(True)
    fn()
    rows = m.timing()
    m.enable_timing(False)
    agg = {}
    for name, ms in rows:
        agg[name] = agg.get(name, 0.0) + ms
    return ", ".join(f"{k} {v:.3f}" for k, v in agg.items())


print(f"N = {N}, d = {d}, EI; ms, median (min) of 30 alternated blocking calls from host arrays", file=out)
for R in (4096, 10):
    xs = np.asfortranarray(rng.random((d, R)))
    for p, S in ((8, 0), (8, 64), (32, 1024)):
        m.set_pending(rng.random((d, p)))
        kw = dict(fantasies=S, seed=1, raise_tau=True)
        calls = {"score_pending": lambda: m.score_pending("EI", prm, xs, **kw),
                 "score_pending_grad": lambda: m.score_pending_grad("EI", prm, xs, **kw),
                 "score_grad": lambda: m.score_grad("EI", prm, xs)}
        ts = {k: [] for k in calls}
        for rep in range(35):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                if rep >= 5:
                    ts[name].append(time.perf_counter() - t0)
        for name, fn in calls.items():
            print(f"R = {R:5d} p = {p:2d} S = {S:4d}  {name:18s} {1e3 * np.median(ts[name]):8.3f} ({1e3 * np.min(ts[name]):.3f})   "
                  f"stages [ms]: {split(fn)}", file=out)
m.close()
