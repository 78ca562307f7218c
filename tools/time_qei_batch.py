#!/usr/bin/env python
"""Wall time of ONE greedy q-EI batch over R candidates from S joint draws, two routes to the same (idx, gain):

    --mode a    the route before bohip_gp_qei_batch: model.sample_joint(want_samples=True) -- the S x R matrix crosses to the host --
                plus the NumPy twin of the selection (tests/qei_reference.py).  Works with any library build that has
                bohip_gp_sample_joint; BOHIP_LIB selects it.
    --mode b    model.qei_batch: the draws stay on the device, idx / gain come back.  Also prints the stage split of enable_timing
                (the draw stages and `qei_select`) and the selection's rate against the bytes of F it reads (q passes over S x R).
    --mode ab   alternates a (library BOHIP_LIB_A) and b (this build) as fresh child processes, --rounds times each (default 3), and
                prints per shape the medians, the spread of each route's per-round medians, the gain a - b and whether the gain
                exceeds five times the larger spread.

Shapes: N = 3000, d = 8, R = 4096 at (S, q) = (256, 8) and (1024, 32); N = 10000, d = 8, R = 2048 at (256, 8).

    BOHIP_LIB_A=/path/to/older/libbohip.so python tools/time_qei_batch.py --mode ab [--reps 10] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(3000, 8, 4096, 256, 8), (3000, 8, 4096, 1024, 32), (10000, 8, 2048, 256, 8)]


def problem(N, d, R):
    rng = np.random.default_rng(3)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    Xs = np.asfortranarray(np.random.default_rng(4).random((R, d)).T)
    return X, y, Xs


def timed(fn, reps, warm=2):
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


def run_route(mode, reps):
    """One process, one library: a JSON line per shape."""
    import ctypes

    import qei_reference as qr
    from bohip import _lib

    have = ctypes.CDLL(_lib.LIB_PATH)                # an older build lacks the newer symbols: bind what it exports
    for table in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES):
        for sym in [k for k in table if not hasattr(have, k)]:
            del table[sym]
    import bohip

    for N, d, R, S, q in SHAPES:
        X, y, Xs = problem(N, d, R)
        m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
        m.append_(X.T, y)
        tau = float(y.max())
        out = {}

        def route_a():
            F = m.sample_joint(Xs, S, 5).samples
            out["r"] = qr.qei_greedy(F, tau, q)

        def route_b():
            r = m.qei_batch(Xs, q, S, 5, tau=tau)
            out["r"] = (r.idx, r.gain)

        fn = route_a if mode == "a" else route_b
        ts = timed(fn, reps)
        rec = dict(mode=mode, lib=os.path.basename(_lib.LIB_PATH), N=N, R=R, S=S, q=q, median_ms=float(np.median(ts)), min_ms=float(ts.min()),
                   idx=[int(i) for i in out["r"][0]], gain_sum=float(np.sum(out["r"][1])))
        if mode == "b":
            st = stage_medians(m, route_b, reps)
            rec["stages_ms"] = st
            sel = dict(st).get("qei_select")
            if sel:
                rec["select_GBps_over_F"] = q * S * R * 8.0 / sel / 1e6
        print(json.dumps(rec), flush=True)
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("a", "b", "ab"), required=True)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.mode != "ab":
        run_route(a.mode, a.reps)
        return
    lib_a = os.environ.get("BOHIP_LIB_A")
    if not lib_a or not os.path.exists(lib_a):
        sys.exit("--mode ab needs BOHIP_LIB_A=<library of the build to compare with>")
    rows = {"a": [], "b": []}
    for rnd in range(max(3, a.rounds)):
        for mode in ("a", "b"):                      # a fresh process per visit: one library per process, one process on the device at a time
            env = dict(os.environ)
            env.pop("BOHIP_LIB", None)
            if mode == "a":
                env["BOHIP_LIB"] = lib_a
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--reps", str(a.reps)], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"route {mode} failed (exit {p.returncode}):\n{p.stdout}\n{p.stderr}")
            recs = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
            rows[mode].append(recs)
            for r in recs:
                print(f"round {rnd} {mode} {r['lib']:24s} N={r['N']:5d} R={r['R']:4d} S={r['S']:4d} q={r['q']:2d}  median {r['median_ms']:10.3f} ms  "
                      f"min {r['min_ms']:10.3f} ms", flush=True)
    print()
    for i, (N, d, R, S, q) in enumerate(SHAPES):
        ma = np.array([r[i]["median_ms"] for r in rows["a"]])
        mb = np.array([r[i]["median_ms"] for r in rows["b"]])
        spread = max(np.ptp(ma), np.ptp(mb))
        gain = float(np.median(ma) - np.median(mb))
        same = all(r[i]["idx"] == rows["b"][0][i]["idx"] for r in rows["a"] + rows["b"])
        print(f"N={N} R={R} S={S} q={q}:  a {np.median(ma):.3f} ms (spread {np.ptp(ma):.3f})  b {np.median(mb):.3f} ms (spread {np.ptp(mb):.3f})  "
              f"gain {gain:.3f} ms = {gain / spread if spread > 0 else float('inf'):.1f} x the larger spread "
              f"({'above' if gain > 5 * spread else 'NOT above'} 5 x);  same picks on both routes: {same}")
        last = rows["b"][-1][i]
        print("    b stages (ms): " + "  ".join(f"{n} {ms:.3f}" for n, ms in last["stages_ms"]))
        if "select_GBps_over_F" in last:
            print(f"    qei_select reads F {q} times: {q * S * R * 8 / 1e6:.1f} MB in {dict(last['stages_ms'])['qei_select']:.3f} ms = "
                  f"{last['select_GBps_over_F']:.0f} GB/s ({2 * q} launches + 1)")


if __name__ == "__main__":
    main()
