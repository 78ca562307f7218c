#!/usr/bin/env python
"""Median wall time of the marginal likelihood and its gradient at H hyper-parameter settings, two ways:

    --mode loop     H times set_params_ + mll_grad on the resident model: what a sequential multi-start fit pays.  Works with an
                    older library build too (BOHIP_LIB selects it; symbols it lacks are not bound) -- the baseline is the PARENT
                    build's library, not the build under test
    --mode batch    this build's mll_grad_batch(Theta) -- ONE launch, one workgroup per setting -- on the same settings, and the
                    value-only call
    --mode stages   the stage split of the kernel's first workgroup (BOHIP_FIT_TRACE: wall-clock stamps inside the kernel) at
                    N = 256 for H = 1, 8, 64
    --mode fit      wall time of MAPGPOptimizer(restarts=8, maxeval=60) through optimizemodel_ at N = 64, 128, 256, batched and with
                    the looping fallback forced, and of the single search (restarts=1)

Shapes: N in {64, 128, 256, 512}, d = 8, H in {1, 8, 64}; settings within +-0.5 of the model's own.

    python tools/time_mll_batch.py --mode batch [--reps 20]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402
from time_joint_draw import model, problem, timed  # noqa: E402

SIZES, HS, D = (64, 128, 256, 512), (1, 8, 64), 8


def settings(H):
    c = np.concatenate([[-2.0, 0.0], np.full(D, np.log(0.5)), [0.0]])
    return c + np.random.default_rng(H).uniform(-0.5, 0.5, (H, c.size))


def loop(m, Theta):
    for t in Theta:
        m.set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
        m.mll_grad()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loop", "batch", "stages", "fit"), required=True)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    if a.mode == "loop":   # an older build lacks the newer symbols: bind what it exports
        import ctypes
        from bohip import _lib
        have = ctypes.CDLL(_lib.LIB_PATH)
        for table in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES):
            for sym in [k for k in table if not hasattr(have, k)]:
                del table[sym]
    if a.mode == "stages":
        if os.environ.get("BOHIP_FIT_TRACE") is None:   # the library prints the stamps on stderr: run this mode in a child and keep them
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "stages"], env={**os.environ, "BOHIP_FIT_TRACE": "1"},
                                 stderr=subprocess.PIPE, text=True).stderr
            rows = [l for l in out.splitlines() if l.startswith("bohip fit stages")]
            for H in HS:
                mine = [l for l in rows if f" H={H} " in l]
                print(f"{lib:22s} stages (last of {len(mine)} calls) " + mine[-1][len("bohip fit stages "):], flush=True)
            return
        X, y, _ = problem(256, D, 1)
        m = model(X, y)
        for H in HS:
            for _ in range(5):
                m.mll_grad_batch(settings(H))
        return
    if a.mode == "fit":
        from bohip import bopt

        for N in (64, 128, 256):
            X, y, _ = problem(N, D, 1)
            kw = dict(every=1, maxeval=60, seed=1, noisebounds=[-6, 2], meanbounds=[[-2], [2]], kernbounds=[[-4] * (D + 1), [4] * (D + 1)])
            table = bopt._FIT_BATCH_MIN_H
            for name, restarts, rule in (("restarts=8 batched", 8, ((512, 1),)), ("restarts=8 looping", 8, ((512, 10 ** 9),)), ("restarts=1", 1, table)):
                bopt._FIT_BATCH_MIN_H = rule
                ts, end = [], 0.0
                for _ in range(3):
                    m = model(X, y)
                    t0 = time.perf_counter()
                    bopt.optimizemodel_(bopt.MAPGPOptimizer(restarts=restarts, **kw), m)
                    ts.append(time.perf_counter() - t0)
                    end = m.mll()
                    m.close()
                print(f"{lib:22s} fit    N={N:4d} {name:20s} median {np.median(ts) * 1e3:9.2f} ms  end mll {end:.4f}", flush=True)
            bopt._FIT_BATCH_MIN_H = table
        return
    for N in SIZES:
        X, y, _ = problem(N, D, 1)
        m = model(X, y)
        for H in HS:
            Theta = settings(H)
            if a.mode == "loop":
                ts = timed(lambda: loop(m, Theta), a.reps)
                print(f"{lib:22s} loop   N={N:4d} H={H:3d}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  per setting {np.median(ts) / H:7.3f} ms", flush=True)
            else:
                ts = timed(lambda: m.mll_grad_batch(Theta), a.reps)
                tv = timed(lambda: m.mll_grad_batch(Theta, want_grad=False), a.reps)
                print(f"{lib:22s} batch  N={N:4d} H={H:3d}  median {np.median(ts):8.3f} ms  min {ts.min():8.3f} ms  per setting {np.median(ts) / H:7.3f} ms;  "
                      f"value only: median {np.median(tv):8.3f} ms", flush=True)
        m.close()


if __name__ == "__main__":
    main()
