#!/usr/bin/env python
"""Median wall time of noisy expected improvement at the bench shape (N = 3000, d = 8, R = 4096, EI):

    (a) score        bohip_gp_score with all scores, set_batch_hint(R) forcing the full (unpruned) whole-K pass -- the yardstick
    (b) score_nei    bohip_gp_score_nei, warm (companion and fantasies kept), at S = 0, 16, 64
    (c) cold         bohip_gp_nei_release + bohip_gp_nei_prepare: the companion's refit plus the fantasies, beside
    (d) refit        bohip_gp_refit of the model itself

Medians of --reps calls, the forms alternated --rounds times in ONE process; the spread of a form is the range of its per-round
medians.  Then the stage split of one call of each form from the library's timing labels, and the FP64 rates of k_nei_means and
k_trigemm_sq from those labels (2 R Npad Sp and R Npad^2 flops).

    python tools/time_nei.py [--reps 30] [--rounds 3]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402
from bohip import _lib  # noqa: E402

N, D, R = 3000, 8, 4096
SS = (0, 16, 64)
JREL = 1e-8


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    lib = _lib.load()
    rng = np.random.default_rng(3)
    X = rng.random((N, D))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    Xs = np.asfortranarray(np.random.default_rng(4).random((R, D)).T)
    tau = [float(y.max()) - 1.0]
    m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
    m.append_(X.T, y)
    m.set_batch_hint(R)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    sc, mu, var, best = np.empty(R), np.empty(R), np.empty(R), _lib.Best()

    def nei(S):
        _lib.check(lib.bohip_gp_score_nei(m._h, _lib.ACQ["EI"], None, ptr(Xs), R, S, 1, JREL, ptr(sc), ptr(mu), ptr(var), C.byref(best)))

    def cold(S=64):
        m.nei_release()
        m.nei_prepare(S=S, seed=1, jitter_rel=JREL)

    forms = [("(a) score", lambda: m.score("EI", tau, Xs))]
    forms += [(f"(b) score_nei S={S}", (lambda S=S: nei(S))) for S in SS]
    forms += [("(c) cold: release + prepare S=64", cold), ("(d) refit", m.fit_)]
    for S in SS:                                                   # a handle keeps ONE set of fantasies: the timed loop of a form stays warm,
        nei(S)                                                     # the first call of a round after another S rebuilds them (not timed)
    print(f"delta in force {m.nei_info(_lib.NEI_INFO_DELTA):.3g}, delta steps {m.nei_info(_lib.NEI_INFO_JITTER_STEPS)}, "
          f"bytes held {m.nei_info(_lib.NEI_INFO_BYTES) / 2**20:.1f} MiB", flush=True)
    med = {name: [] for name, _ in forms}
    for _ in range(a.rounds):
        for name, f in forms:
            f()                                                    # (warm: fantasies of this S, caches)
            med[name].append(timed(f, max(3, a.reps // 6) if name[:3] in ("(c)", "(d)") else a.reps))
    spread = {}
    for name, v in med.items():
        spread[name] = max(v) - min(v)
        print(f"{name:36s} median of medians {np.median(v):9.3f} ms   per round {['%.3f' % t for t in v]}   spread {spread[name]:.3f} ms", flush=True)
    s = np.median(med["(a) score"])
    for S in SS:
        print(f"score_nei S={S} / score = {np.median(med[f'(b) score_nei S={S}']) / s:.2f}")
    print(f"cold (companion refit + fantasies) / refit = {np.median(med['(c) cold: release + prepare S=64']) / np.median(med['(d) refit']):.2f}")
    m.enable_timing(True)
    m.score("EI", tau, Xs)
    st = m.timing()
    print("stages (a):", ", ".join(f"{n} {t:.3f}" for n, t in st))
    Npad = (N + 1 + 127) // 128 * 128
    t_tri = sum(t for n, t in st if n.startswith("trigemm_sq"))
    for S in SS:
        nei(S)
        nei(S)
        st = m.timing()
        print(f"stages (b) S={S}, warm:", ", ".join(f"{n} {t:.3f}" for n, t in st))
        t_means = sum(t for n, t in st if n == "nei_means")
        t_tri_c = sum(t for n, t in st if n.startswith("trigemm_sq"))
        Sp = (max(S, 1) + 63) // 64 * 64
        print(f"    k_nei_means {2.0 * R * Npad * Sp / t_means / 1e9:8.2f} TF/s useful-padded ({2.0 * R * N * max(S, 1) / t_means / 1e9:.2f} TF/s of live columns)"
              f"   k_trigemm_sq {1.0 * R * Npad * Npad / t_tri_c / 1e9:8.2f} TF/s (companion), {1.0 * R * Npad * Npad / t_tri / 1e9:.2f} TF/s (model)")
    cold()
    print("stages (c) cold S=64:", ", ".join(f"{n} {t:.3f}" for n, t in m.timing()))
    m.fit_()
    print("stages (d) refit:", ", ".join(f"{n} {t:.3f}" for n, t in m.timing()))
    m.close()


if __name__ == "__main__":
    main()
