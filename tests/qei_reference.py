"""NumPy twin of the greedy Monte-Carlo q-EI selection (include/bohip_qei.h), a helper of the q-EI tests, not a test
module.  It restates the summation order that is part of the ABI, so it reproduces the device bit for bit:

    m_s = tau;  round k:  u(f, m) = (f > m) ? f - m : 0
        part_b(j) = sum_{s = 32 b .. min(32 b + 31, S - 1)} u(F_sj, m_s)    s ascending, from +0.0
        tot(j)    = sum_b part_b(j)                                         b ascending
        gain(j)   = tot(j) / S
        j* = first maximum of gain under strict '>' from 0;  none: idx[k..] = -1, gain[k..] = 0, stop
        idx[k] = j*, gain[k] = gain(j*), m_s = (F_sj* > m_s) ? F_sj* : m_s
"""
import itertools
import math

import numpy as np

B = 32   # draws per block of the summation order


def gains(F, m):
    """gain(j) of one round, in the ABI's order (vectorised over the candidates; every add is one IEEE FP64 add)."""
    F = np.asarray(F, dtype=np.float64)
    S, R = F.shape
    with np.errstate(invalid="ignore"):
        U = np.where(F > m[:, None], F - m[:, None], 0.0)       # (F > m is False for NaN; the unused branch may hold NaN / Inf - Inf)
    tot = np.zeros(R)
    for b0 in range(0, S, B):
        part = np.zeros(R)
        for s in range(b0, min(b0 + B, S)):
            part = part + U[s]
        tot = tot + part
    return tot / np.float64(S)


def qei_greedy(F, tau, q):
    """(idx[q] int64, gain[q]) of the contract."""
    F = np.asarray(F, dtype=np.float64)
    S, R = F.shape
    m = np.full(S, float(tau))
    idx = np.full(q, -1, dtype=np.int64)
    gain = np.zeros(q)
    for k in range(q):
        g = gains(F, m)
        j = int(np.argmax(g))                                   # (the first maximum; no NaN is ever produced)
        if not g[j] > 0.0:
            break
        idx[k], gain[k] = j, g[j]
        m = np.where(F[:, j] > m, F[:, j], m)
    return idx, gain


def qei_value(F, tau, cols):
    """The sample-average q-EI of a batch, mean_s max(max_{j in cols} F_sj - tau, 0), in any order (for comparisons with a bound)."""
    F = np.asarray(F, dtype=np.float64)
    if len(cols) == 0:
        return 0.0
    return float(np.mean(np.maximum(np.max(F[:, list(cols)], axis=1) - tau, 0.0)))


def best_subset(F, tau, q):
    """(value, subset) of the best batch of q candidates by brute force."""
    R = np.asarray(F).shape[1]
    best, arg = -math.inf, None
    for c in itertools.combinations(range(R), q):
        v = qei_value(F, tau, c)
        if v > best:
            best, arg = v, c
    return best, arg


def textbook_ei(mu, var, tau):
    """Delta Phi(z) + sigma phi(z) with Delta = mu - tau, z = Delta / sigma (NOT the reference's functor, which drops the sigma)."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    sig = np.sqrt(np.maximum(var, 0.0))
    d = mu - tau
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sig > 0, d / sig, 0.0)
    Phi = 0.5 * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0)))
    phi = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return np.where(sig > 0, d * Phi + sig * phi, np.maximum(d, 0.0))
