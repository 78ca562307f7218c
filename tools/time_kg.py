#!/usr/bin/env python
"""Stage times of the knowledge gradient over a candidate set: model.kg(X) with E = R at N = 3000, d = 8,
R = 1024 and 4096.

    python tools/time_kg.py [--reps 20]              every shape, each in a child process of its own under a time limit; the first
                                                     child that fails ends the run
    python tools/time_kg.py --shape 4096 [--reps 20] one shape, in this process

Per shape: the wall time of model.kg and of model.predict_cov (the same posterior stages, plus the R x R copy to the host), the
stage split of enable_timing / timing() -- kstar, trigemm_sq+V, gemm_VV, post_cov, kg -- and the `kg` stage against the sum of the
stages that build Sigma; the segments per evaluation point; and the host reference tests/kg_reference.py kg_hull on the same
(mu, Sigma) -- over --hull-points evaluation points, scaled to E (it is a Python loop over the R lines of every point).
BOHIP_LIB selects the library build."""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = (1024, 4096)
N, D = 3000, 8
LNOISE = -2.0


def one_shape(R, reps, hull_points):
    import bohip
    import kg_reference as kr
    from time_joint_draw import model, problem, stage_medians, timed

    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    X, y, Xs = problem(N, D, R)
    m = model(X, y)
    wall = timed(lambda: m.kg(Xs), reps)
    cov_wall = timed(lambda: m.predict_cov(Xs), max(3, reps // 4))
    st = stage_medians(m, lambda: m.kg(Xs), reps)
    res = m.kg(Xs)
    print(f"{lib:18s} kg N={N} d={D} R=E={R:4d}  median {np.median(wall):8.3f} ms  min {wall.min():8.3f} ms   "
          f"(predict_cov with its R x R copy: median {np.median(cov_wall):8.3f} ms)", flush=True)
    print("    " + "  ".join(f"{n} {ms:.3f}" for n, ms in st), flush=True)
    d = dict(st)
    build = sum(ms for n, ms in st if n != "kg")
    print(f"    kg stage {d['kg']:.3f} ms against {build:.3f} ms for the stages that build Sigma: {d['kg'] / build:.2f}x", flush=True)
    print(f"    segments per point: min {res.nseg.min()}  mean {res.nseg.mean():.1f}  max {res.nseg.max()};  "
          f"KG max {res.values.max():.3e} at {res.best_idx}", flush=True)
    mu, cov = m.predict_cov(Xs)
    nu = math.exp(2.0 * LNOISE) + np.finfo(np.float64).eps
    pts = min(hull_points, R)
    t0 = time.perf_counter()
    hull = np.array([kr.kg_hull(mu, cov[e] / math.sqrt(cov[e, e] + nu))[0] for e in range(pts)])
    dt = time.perf_counter() - t0
    err = np.abs(res.values[:pts] - hull).max()
    print(f"    host kg_hull: {dt:.2f} s for {pts} points = {dt * R / pts:.1f} s for all {R};  worst |device - hull| {err:.2e}", flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hull-points", type=int, default=64)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if a.shape:
        one_shape(a.shape, a.reps, a.hull_points)
        return 0
    for R in SHAPES:
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--shape", str(R),
                              "--reps", str(a.reps), "--hull-points", str(a.hull_points)])
        if rc != 0:
            print(f"shape R = {R} ended with status {rc}; nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
