"""The greedy q-EHVI selection of include/bohip_qehvi.h in exact rational arithmetic: every double is a rational, so the area a point
adds to a staircase, the sums over the draws and the division by S are exact, and doubles compare exactly as they stand."""
import bisect
from fractions import Fraction

import numpy as np


class Stair:
    """c = [r1, f1 of the points ..] ascending, h = [f2 of the points .., r2] descending; strip i spans [c[i], c[i + 1]] (the last one
    is open) above h[i].  P[i] is the exact area of the strips before i below their heights."""
    def __init__(self, T, ref):
        self.c, self.nh = [ref[0]] + [x for x, _ in T], [-y for _, y in T] + [-ref[1]]
        self.cF, self.hF = [Fraction(x) for x in self.c], [-Fraction(x) for x in self.nh]
        self.P = [Fraction(0)]
        for t in range(len(T)):
            self.P.append(self.P[-1] + (self.cF[t + 1] - self.cF[t]) * self.hF[t])

    def improvement(self, a, b):
        """HV(T + (a, b)) - HV(T): strips lo .. last contribute; the last is cut at a, the others are whole."""
        last = bisect.bisect_left(self.c, a) - 1           # the strip that holds a
        lo = bisect.bisect_right(self.nh, -b)              # strips lo .. have a height below b
        fa, fb = Fraction(a), Fraction(b)
        return Fraction(0) if lo > last else (fa - self.cF[last]) * (fb - self.hF[last]) + fb * (self.cF[last] - self.cF[lo]) - (self.P[last] - self.P[lo])


def insert(T, a, b):   # T with (a, b) folded in, unchanged if a point of T weakly dominates it; -> (T', points removed)
    if any(x >= a and y >= b for x, y in T):
        return T, 0
    keep = [(x, y) for x, y in T if not (x <= a and y <= b)]
    return sorted(keep + [(a, b)]), len(T) - len(keep)


def greedy(F0, F1, front, ref, q):
    """-> idx[q] (-1: nothing could win), gains (Fractions), seconds (per round the largest gain that differs from the winner's), the
    most points one pick removed from one staircase.  Exact ties with the winner must be copies of its column (the same bytes on the device)."""
    S, R = F0.shape
    valid = np.isfinite(F0) & np.isfinite(F1) & (F0 > ref[0]) & (F1 > ref[1])
    stairs = [[(float(x), float(y)) for x, y in zip(front[0], front[1])] for _ in range(S)]
    idx, gains, seconds, most = np.full(q, -1, dtype=np.int64), [Fraction(0)] * q, [Fraction(0)] * q, 0
    for k in range(q):
        tot = [Fraction(0)] * R
        for s, T in enumerate(stairs):
            st = Stair(T, ref)
            for j in np.flatnonzero(valid[s]):
                tot[j] += st.improvement(float(F0[s, j]), float(F1[s, j]))
        best = max(tot)
        if best <= 0:
            break
        js = tot.index(best)
        assert all(F0[:, j].tobytes() == F0[:, js].tobytes() and F1[:, j].tobytes() == F1[:, js].tobytes() for j in range(R) if tot[j] == best)
        idx[k], gains[k] = js, best / S
        seconds[k] = max([t for t in tot if t != best], default=Fraction(0)) / S
        for s in np.flatnonzero(valid[:, js]):
            stairs[s], gone = insert(stairs[s], float(F0[s, js]), float(F1[s, js]))
            most = max(most, gone)
    return idx, gains, seconds, most
