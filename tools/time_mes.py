#!/usr/bin/env python
"""Stage times of max-value entropy search over a candidate set: model.mes(X, samples = 16) at N = 3000, d = 8 --
Gumbel mode at R = 1024 and 4096, joint mode at R = 1024.

    python tools/time_mes.py [--reps 20]                          every case, each in a child process of its own under a time
                                                                  limit; the first child that fails ends the run
    python tools/time_mes.py --case gumbel:4096 [--reps 20]       one case, in this process

Per case: the wall time of model.mes and of model.predict_f on the same candidates, the stage split of enable_timing / timing() --
the stages of bohip_gp_predict (or of bohip_gp_sample_joint), then mes_bracket, mes_probe, mes_draw, mes_rowmax, mes_values -- and
the sum of the mes_* stages against the posterior stages of the same call, the yardstick: a few hundred thousand transcendental
evaluations against the posterior's contraction.  BOHIP_LIB selects the library build."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("gumbel:1024", "gumbel:4096", "joint:1024")
N, D, K = 3000, 8, 16


def one_case(case, reps):
    from time_joint_draw import model, problem, stage_medians, timed

    mode, R = case.split(":")
    R = int(R)
    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    X, y, Xs = problem(N, D, R)
    m = model(X, y)
    call = lambda: m.mes(Xs, samples=K, mode=mode, seed=1)   # noqa: E731
    wall = timed(call, reps)
    pred = timed(lambda: m.predict_f(Xs), reps)
    st = stage_medians(m, call, reps)
    res = call()
    print(f"{lib:18s} mes {mode:6s} N={N} d={D} R={R:4d} K={K}  median {np.median(wall):8.3f} ms  min {wall.min():8.3f} ms   "
          f"(predict_f: median {np.median(pred):8.3f} ms)", flush=True)
    print("    " + "  ".join(f"{n} {ms:.3f}" for n, ms in st), flush=True)
    mes = sum(ms for n, ms in st if n.startswith("mes_"))
    post = sum(ms for n, ms in st if not n.startswith("mes_"))
    print(f"    mes_* stages {mes:.3f} ms against {post:.3f} ms for the posterior stages of the same call: {mes / post:.2f}x", flush=True)
    print(f"    max values {res.maxvals.min():.4f} .. {res.maxvals.max():.4f}, quantiles {res.quantiles};  MES max {res.best_val:.3e} "
          f"at {res.best_idx}", flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120, help="seconds a case's child process may take")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if a.case:
        one_case(a.case, a.reps)
        return 0
    for case in CASES:
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case,
                              "--reps", str(a.reps)])
        if rc != 0:
            print(f"case {case} ended with status {rc}; nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
