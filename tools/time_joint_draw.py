#!/usr/bin/env python
"""Median wall time of ONE joint posterior draw over R candidates, two ways:

    --mode host     myrand(model, X, rng): bohip_gp_predict_cov on the device, the R x R covariance copied to the host and
                    factorised there with LAPACK -- the only joint draw before bohip_gp_sample_joint; works with any library build
    --mode device   myrand(model, X, seed=k) = model.sample_joint(X, 1, k): everything on the device, the draw (R values) returned
    --mode stages   this build's sample_joint alone at R = 4096, S = 1, 8, 64, 1024: wall time (winners only / with the S x R
                    samples) and the stage split of enable_timing / timing(); for S = 1 the bytes/s of the pass over C
    --mode forms    the `sample_draw` stage alone over S = 1 .. 1024 at R = 4096; run once with BOHIP_SAMPLE_MFMA_MIN=1 (every S on
                    the MFMA kernel) and once with BOHIP_SAMPLE_MFMA_MIN=1000000 (every S on the row-panel kernel): where the
                    two cross is where the library switches

BOHIP_LIB selects the library build, so the host path of an older build and the device call of this one can be alternated A/B
on one box.  Shapes: N = 3000, d = 8, R = 1024 and 4096; N = 10000, d = 8, R = 2048.

    python tools/time_joint_draw.py --mode device [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402

SHAPES = [(3000, 8, 1024), (3000, 8, 4096), (10000, 8, 2048)]


def problem(N, d, R):
    rng = np.random.default_rng(3)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    Xs = np.asfortranarray(np.random.default_rng(4).random((R, d)).T)
    return X, y, Xs


def model(X, y):
    N, d = X.shape
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
    m.append_(X.T, y)
    return m


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts) * 1e3


def stage_medians(m, fn, reps):
    m.enable_timing(True)
    fn()
    rows = []
    for _ in range(reps):
        fn()
        rows.append(m.timing())
    m.enable_timing(False)
    names = []
    for n, _ in rows[0]:
        if n not in names:
            names.append(n)
    return [(n, float(np.median([sum(ms for k, ms in r if k == n) for r in rows]))) for n in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("host", "device", "stages", "forms"), required=True)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lib = os.path.basename(os.environ.get("BOHIP_LIB", "") or "libbohip.so")
    if a.mode == "host":   # an older build has no bohip_gp_sample_joint: bind what it exports (the host path needs predict_cov only)
        import ctypes
        from bohip import _lib
        have = ctypes.CDLL(_lib.LIB_PATH)
        for sym in [k for k in _lib.SIGNATURES if not hasattr(have, k)]:
            del _lib.SIGNATURES[sym]
    if a.mode in ("host", "device"):
        for N, d, R in SHAPES:
            X, y, Xs = problem(N, d, R)
            m = model(X, y)
            rng = np.random.default_rng(0)
            k = [0]

            def host():
                return bohip.myrand(m, Xs, rng)

            def device():
                k[0] += 1
                return bohip.myrand(m, Xs, seed=k[0])

            ts = timed(host if a.mode == "host" else device, a.reps)
            extra = ""
            if a.mode == "device":
                js = m.sample_joint(Xs, 1, 1, want_samples=False)
                extra = f"  jitter tries {js.tries}"
            print(f"{lib:22s} {a.mode:6s} N={N:5d} R={R:4d}  median {np.median(ts):9.3f} ms  min {ts.min():9.3f} ms{extra}", flush=True)
            m.close()
        return
    N, d, R = 3000, 8, 4096
    X, y, Xs = problem(N, d, R)
    m = model(X, y)
    cbytes = 8.0 * R * (R + 1) / 2
    if a.mode == "stages":
        for S in (1, 8, 64, 1024):
            best = timed(lambda: m.sample_joint(Xs, S, 5, want_samples=False), a.reps)
            full = timed(lambda: m.sample_joint(Xs, S, 5), a.reps)
            st = stage_medians(m, lambda: m.sample_joint(Xs, S, 5, want_samples=False), a.reps)
            print(f"{lib:22s} stages N={N} R={R} S={S:4d}  winners only: median {np.median(best):8.3f} ms  min {best.min():8.3f} ms;  "
                  f"with samples: median {np.median(full):8.3f} ms", flush=True)
            print("    " + "  ".join(f"{n} {ms:.3f}" for n, ms in st), flush=True)
            if S == 1:
                draw = dict(st)["sample_draw"]
                print(f"    sample_draw at S = 1 reads C once: {cbytes / 1e6:.1f} MB in {draw:.3f} ms = {cbytes / draw / 1e9:.2f} TB/s "
                      "(includes the arg-max finish kernel)", flush=True)
    else:
        knob = os.environ.get("BOHIP_SAMPLE_MFMA_MIN", "(default)")
        for S in (1, 2, 4, 8, 16, 32, 64, 128, 192, 256, 384, 512, 1024):
            st = dict(stage_medians(m, lambda: m.sample_joint(Xs, S, 5, want_samples=False), a.reps))
            print(f"{lib:22s} forms  BOHIP_SAMPLE_MFMA_MIN={knob:8s} R={R} S={S:3d}  sample_draw {st['sample_draw']:8.3f} ms", flush=True)
    m.close()


if __name__ == "__main__":
    main()
