"""Warm times of the two ways to evaluate the knowledge gradient off the grid: N = 3000, d = 8, R = 1024, E = 16, 256.
  --mode a   bohip_gp_kg on [Xe; A] (value only: every call rebuilds V' and Sigma of the whole set)
  --mode b   bohip_gp_kg_grad on Xe over the resident A (value and gradient), with the stage split of one call
  --mode ab  both alternated as fresh child processes, three times; the ratio of the medians with both routes' spreads
Each process: 5 warm-up calls, then the median (min .. max) of 30 blocking calls from host arrays.
Usage: python tools/time_kg_grad.py --mode ab [out.txt]"""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N, d, R = 3000, 8, 1024


def one(mode):
    sys.path.insert(0, os.path.join(HERE, ".."))
    import bohip

    rng = np.random.default_rng(0)
    X = rng.random((d, N))
    y = np.sin(3 * X).sum(0) + 0.1 * rng.standard_normal(N)
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
    m.append_(X, y)
    A = np.asfortranarray(rng.random((d, R)))
    for E in (16, 256):
        Xe = np.asfortranarray(rng.random((d, E)))
        both = np.asfortranarray(np.concatenate([Xe, A], axis=1))
        m.kg_set_points(A)
        fn = (lambda: m.kg(both, E)) if mode == "a" else (lambda: m.kg_grad(Xe))
        ts = []
        for rep in range(35):
            t0 = time.perf_counter()
            fn()
            if rep >= 5:
                ts.append(1e3 * (time.perf_counter() - t0))
        m.enable_timing(True)
        fn()
        agg = {}
        for name, ms in m.timing():
            agg[name] = agg.get(name, 0.0) + ms
        m.enable_timing(False)
        print(f"{mode} E = {E:3d}  {np.median(ts):8.3f} ({np.min(ts):.3f} .. {np.max(ts):.3f})  stages [ms]: "
              + ", ".join(f"{k} {v:.3f}" for k, v in agg.items()), flush=True)
    m.close()


if __name__ == "__main__":
    mode = sys.argv[sys.argv.index("--mode") + 1]
    if mode in ("a", "b"):
        one(mode)
        sys.exit(0)
    rest = [a for a in sys.argv[1:] if a not in ("--mode", mode)]
    out = open(rest[0], "w") if rest else sys.stdout
    print(f"N = {N}, d = {d}, R = {R}; ms, median (min .. max) of 30 blocking calls; a = kg on [Xe; A], b = kg_grad; fresh processes, alternated",
          file=out)
    med = {}
    for rep in range(3):
        for md in ("a", "b"):
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", md], check=True, capture_output=True, text=True,
                                 timeout=60).stdout
            out.write(txt)
            for line in txt.splitlines():
                med.setdefault((md, int(line.split()[3])), []).append(float(line.split()[4]))
    for E in (16, 256):
        a, b = med[("a", E)], med[("b", E)]
        print(f"E = {E}: a {np.median(a):.3f} ({min(a):.3f} .. {max(a):.3f}), b {np.median(b):.3f} ({min(b):.3f} .. {max(b):.3f}), "
              f"a / b = {np.median(a) / np.median(b):.2f}", file=out)
