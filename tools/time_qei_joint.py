"""Warm times of bohip_gp_qei_joint beside bohip_gp_score_grad of the same B q rows on one model: N = 3000, d = 8,
q = 8, S = 256, B = 1, 16, 64.  The value call, the value + gradient call and score_grad ALTERNATE in one process: 5 warm-up rounds,
then the median (min) of 30 rounds of blocking calls; then the stage split of one call through the handle's timing.
Usage: python tools/time_qei_joint.py [out.txt]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bohip   # noqa: E402

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
N, d, q, S = 3000, 8, 8, 256
rng = np.random.default_rng(0)
X = rng.random((d, N))
y = np.sin(3 * X).sum(0) + 0.1 * rng.standard_normal(N)
m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
m.append_(X, y)
tau = float(np.median(y))


def split(fn):
    m.enable_timing(True)
    fn()
    rows = m.timing()
    m.enable_timing(False)
    agg = {}
    for name, ms in rows:
        agg[name] = agg.get(name, 0.0) + ms
    return ", ".join(f"{k} {v:.3f}" for k, v in agg.items())


print(f"N = {N}, d = {d}, q = {q}, S = {S}; ms, median (min) of 30 alternated blocking calls from host arrays", file=out)
for B in (1, 16, 64):
    xs = np.asfortranarray(rng.random((d, B * q)))
    calls = {"qei_joint value": lambda: m.qei_joint(xs, q, S, 1, tau=tau, grad=False),
             "qei_joint value+grad": lambda: m.qei_joint(xs, q, S, 1, tau=tau),
             "score_grad": lambda: m.score_grad("EI", [tau], xs)}
    ts = {k: [] for k in calls}
    for rep in range(35):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep >= 5:
                ts[name].append(time.perf_counter() - t0)
    for name, fn in calls.items():
        print(f"B = {B:3d} (B q = {B * q:4d})  {name:21s} {1e3 * np.median(ts[name]):8.3f} ({1e3 * np.min(ts[name]):.3f})   "
              f"stages [ms]: {split(fn)}", file=out)
m.close()
