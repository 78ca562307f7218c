#!/usr/bin/env python
"""Median wall time of scoring under pending evaluations at the bench shape (N = 3000, d = 8, R = 4096, EI):

    (a) score            bohip_gp_score with all scores, set_batch_hint(R) forcing the unpruned whole-K route -- the yardstick
    (b) score_pending    at (p, S) = (8, 0), (8, 64), (32, 1024)
    (c) definition       what (8, 64) means, on the device: 64 x (fresh handle + append of the 8 fantasised outcomes + score)

Medians of --reps calls ((c): --reps / 6, at least 3), the three forms alternated --rounds times in ONE process; the spread of a
form is the range of its per-round medians.  Then the stage split of one call of each form from the library's timing labels.

    python tools/time_pending.py [--reps 30] [--rounds 3]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bohip  # noqa: E402

N, D, R = 3000, 8, 4096
CASES = [(8, 0), (8, 64), (32, 1024)]


def model(X, y, extra=0):
    m = bohip.ElasticGPE(D, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(D, np.log(0.5)), 0.0), logNoise=-2.0,
                         capacity=len(y) + extra)
    m.append_(X.T, y)
    return m


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def definition(X, y, Xp, Yf, tau, Xs):
    """(c): every fantasy is a model of its own -- built, extended by the pending points in ONE append, scored."""
    acc = np.zeros(Xs.shape[1])
    for yf in Yf:
        m = model(X, y, extra=len(yf))
        m.append_(Xp, yf)
        acc += m.score("EI", tau, Xs)[0]
        m.close()
    return acc / len(Yf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(3)
    X = rng.random((N, D))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    Xs = np.asfortranarray(np.random.default_rng(4).random((R, D)).T)
    XP = np.asfortranarray(np.random.default_rng(5).random((32, D)).T)
    tau = [float(y.max()) - 1.0]
    m = model(X, y)
    m.set_batch_hint(R)
    m.set_pending(XP[:, :8])
    _, mu_p, cov_p = m.pending_info()
    Z = np.array([[bohip._lib.load().bohip_thompson_normal(1, s, i) for i in range(8)] for s in range(64)])
    Yf = mu_p[None, :] + Z @ np.linalg.cholesky(cov_p).T
    want = definition(X, y, XP[:, :8], Yf, tau, Xs)
    got = m.score_pending("EI", tau, Xs, fantasies=64, seed=1).scores
    print(f"(8, 64): max |score_pending - definition| = {np.max(np.abs(got - want)):.3g} (largest value {np.max(np.abs(want)):.3g})", flush=True)
    m32 = model(X, y)                                             # a handle per pending set: the derived state is kept between calls
    m32.set_batch_hint(R)
    m32.set_pending(XP)
    by_p = {8: m, 32: m32}
    forms = [("(a) score", lambda: m.score("EI", tau, Xs))]
    for p, S in CASES:
        forms.append((f"(b) score_pending p={p} S={S}", (lambda p=p, S=S: by_p[p].score_pending("EI", tau, Xs, fantasies=S, seed=1))))
    forms.append(("(c) definition p=8 S=64", lambda: definition(X, y, XP[:, :8], Yf, tau, Xs)))
    for _, f in forms[:-1]:
        for _ in range(5):
            f()
    med = {name: [] for name, _ in forms}
    for _ in range(a.rounds):
        for name, f in forms:
            med[name].append(timed(f, max(3, a.reps // 6) if name.startswith("(c)") else a.reps))
    spread = {}
    for name, v in med.items():
        spread[name] = max(v) - min(v)
        print(f"{name:34s} median of medians {np.median(v):9.3f} ms   per round {['%.3f' % t for t in v]}   spread {spread[name]:.3f} ms", flush=True)
    b, c = "(b) score_pending p=8 S=64", "(c) definition p=8 S=64"
    gain, bar = np.median(med[c]) - np.median(med[b]), 5 * max(spread[b], spread[c])
    print(f"(c) - (b) at (8, 64) = {gain:.3f} ms against the bar 5 x the larger spread = {bar:.3f} ms: {'beats it' if gain > bar else 'DOES NOT beat it'}")
    print(f"(b) - (a) at (8, 0) = {np.median(med['(b) score_pending p=8 S=0']) - np.median(med['(a) score']):.3f} ms")
    m.enable_timing(True)
    m.score("EI", tau, Xs)
    print("stages (a):", ", ".join(f"{n} {t:.3f}" for n, t in m.timing()))
    m32.enable_timing(True)
    for p, S in CASES:
        h = by_p[p]
        h.set_pending(XP[:, :p])                                     # (the same set again: the derived state is rebuilt once)
        h.score_pending("EI", tau, Xs, fantasies=S, seed=1)
        first = h.timing()
        h.score_pending("EI", tau, Xs, fantasies=S, seed=1)          # the steady state: the derived state is kept
        print(f"stages (b) p={p} S={S}, state built:", ", ".join(f"{n} {t:.3f}" for n, t in first))
        print(f"stages (b) p={p} S={S}, steady     :", ", ".join(f"{n} {t:.3f}" for n, t in h.timing()))
    m.close(); m32.close()


if __name__ == "__main__":
    main()
