#!/usr/bin/env python
"""Median wall time of the leave-one-out objective and its gradient at H hyper-parameter settings, two ways:

    --mode loop     H times set_params_ + loo_grad on the resident model: what a lock-step multi-start fit with objective="loo" paid
                    before loo_grad_batch existed.  Works with an older library build too (BOHIP_LIB selects it; symbols it lacks
                    are not bound)
    --mode batch    loo_grad_batch(Theta) -- ONE launch, one workgroup per setting -- on the same settings, and the value-only call
    --mode stages   the stage split of the kernel's first workgroup (BOHIP_FIT_TRACE: wall-clock stamps inside the kernel) at
                    N = 256 for H = 2, 8, 32

Shapes: N in {64, 128, 256, 512}, d = 8, H in {2, 8, 32}; settings within +-0.5 of the model's own.  Every call ends in the
library's own stream synchronise, so the host clock around it is the call's time.  One line per cell: median, min and max of
--reps calls after three warm-up calls.  tools/loo_batch_table.py turns alternating loop / batch runs into the table of
profiles/loo_batch_ab.txt and into bopt._LOO_BATCH_MIN_H.

    python tools/time_loo_batch.py --mode batch [--reps 20]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402,F401
from time_joint_draw import model, problem, timed  # noqa: E402

SIZES, HS, D = (64, 128, 256, 512), (2, 8, 32), 8


def settings(H):
    c = np.concatenate([[-2.0, 0.0], np.full(D, np.log(0.5)), [0.0]])
    return c + np.random.default_rng(H).uniform(-0.5, 0.5, (H, c.size))


def loop(m, Theta):
    for t in Theta:
        m.set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
        m.loo_grad()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loop", "batch", "stages"), required=True)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    if a.mode == "loop":   # an older build lacks the newer symbols: bind what it exports
        import ctypes
        from bohip import _lib
        have = ctypes.CDLL(_lib.LIB_PATH)
        for table in [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES")]:
            for sym in [k for k in table if not hasattr(have, k)]:
                del table[sym]
    if a.mode == "stages":
        if os.environ.get("BOHIP_FIT_TRACE") is None:   # the library prints the stamps on stderr: run this mode in a child and keep them
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "stages"], env={**os.environ, "BOHIP_FIT_TRACE": "1"},
                                 stderr=subprocess.PIPE, text=True).stderr
            rows = [l for l in out.splitlines() if l.startswith("bohip loo stages")]
            for H in HS:
                mine = [l for l in rows if f" H={H} " in l]
                print(f"{lib:22s} stages (last of {len(mine)} calls) " + mine[-1][len("bohip loo stages "):], flush=True)
            return
        X, y, _ = problem(256, D, 1)
        m = model(X, y)
        for H in HS:
            for _ in range(5):
                m.loo_grad_batch(settings(H))
        return
    for N in SIZES:
        X, y, _ = problem(N, D, 1)
        m = model(X, y)
        for H in HS:
            Theta = settings(H)
            if a.mode == "loop":
                ts = timed(lambda: loop(m, Theta), a.reps)
                print(f"{lib:22s} loop   N={N:4d} H={H:3d}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  max {ts.max():8.3f} ms  "
                      f"per setting {np.median(ts) / H:7.3f} ms", flush=True)
            else:
                ts = timed(lambda: m.loo_grad_batch(Theta), a.reps)
                tv = timed(lambda: m.loo_grad_batch(Theta, want_grad=False), a.reps)
                print(f"{lib:22s} batch  N={N:4d} H={H:3d}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  max {ts.max():8.3f} ms  "
                      f"per setting {np.median(ts) / H:7.3f} ms;  value only: median {np.median(tv):8.3f} ms", flush=True)
        m.close()


if __name__ == "__main__":
    main()
