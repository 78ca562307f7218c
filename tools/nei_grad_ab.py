"""Warm times of bohip_gp_score_nei_grad beside bohip_gp_score_nei and bohip_gp_score_grad on one model:
N = 3000, d = 8, S = 64, R = 4096 and R = 10.  Median of 30 blocking calls after 5 warm-up calls, then the stage split of one call
through the handle's timing.  Usage: python tools/nei_grad_ab.py [out.txt]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bohip   # noqa: E402

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
N, d, S = 3000, 8, 64
rng = np.random.default_rng(0)
X = rng.random((d, N))
y = np.sin(3 * X).sum(0) + 0.1 * rng.standard_normal(N)
m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
m.append_(X, y)
kw = dict(S=S, seed=1, acq="ei", jitter_rel=1e-6)


def warm(fn, reps=30):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def split(fn):
    m.enable_timing(True)
    fn()
    rows = m.timing()
    m.enable_timing(False)
    agg = {}
    for name, ms in rows:
        agg[name] = agg.get(name, 0.0) + ms
    return ", ".join(f"{k} {v:.3f}" for k, v in agg.items())


print(f"N = {N}, d = {d}, S = {S}; ms, median (min) of 30 blocking calls from host arrays", file=out)
for R in (4096, 10):
    xs = np.asfortranarray(rng.random((d, R)))
    calls = {"score_nei": lambda: m.nei(xs, **kw), "score_nei_grad": lambda: m.nei_grad(xs, **kw),
             "score_grad": lambda: m.score_grad("EI", [float(y.max())], xs)}
    for name, fn in calls.items():
        med, mn = warm(fn)
        print(f"R = {R:5d}  {name:15s} {med:8.3f} ({mn:.3f})   stages [ms]: {split(fn)}", file=out)
m.close()
