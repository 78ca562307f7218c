"""NumPy references of the knowledge gradient over a candidate set (include/bohip_kg.h).  No device.

kg_march(a, b)  the contract of the header, operation for operation: the march along the upper envelope, z by one IEEE subtraction
                each and one division, the arg-min with its tie rule, the terms db h(-|z|) in csrc/acq_log.h's two forms added in
                march order.  -> (kg, nseg).  The device differs from it only in exp and erfc (libm's here).
kg_hull(a, b)   the independent check, Frazier's algorithm as it is usually written: sort by (b, a), drop the equal-slope losers,
                stack scan for the upper envelope, then sum_i a_i dPhi_i + b_i dphi_i - max a.  -> (kg, vertices).  It cancels
                against max a, so its absolute error is of the order eps (max|a| + max|b|) whatever the size of kg.
"""
import math

import numpy as np

SWITCH, CF_DEPTH = -4.0, 40


def kg_term(db, x):
    """T(db, x) = db h(x), h(x) = phi(x) + x Phi(x), x <= 0."""
    if x > SWITCH:
        phi = 0.3989422804014327 * math.exp(-0.5 * (x * x))
        Phi = 0.5 * math.erfc(-x / 1.4142135623730951)
        return db * (phi + x * Phi)
    t = -x
    r = 0.0
    for k in range(CF_DEPTH, 1, -1):
        r = float(k) / (t + r)
    c1 = 1.0 / (t + r)
    tc = t + c1
    e = math.exp(-0.25 * (x * x))
    return (db * e) * ((0.3989422804014327 * e) * (c1 / tc))


def kg_march(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    live = np.flatnonzero(np.isfinite(a) & np.isfinite(b))
    if live.size == 0:
        return 0.0, 0
    c = int(live[np.lexsort((live, -a[live], b[live]))[0]])          # smallest b, then largest a, then smallest index
    kg, nseg = 0.0, 0
    while True:
        U = live[b[live] > b[c]]
        if U.size == 0:
            break
        with np.errstate(all="ignore"):
            z = (a[c] - a[U]) / (b[U] - b[c])
        ok = ~np.isnan(z)
        U, z = U[ok], z[ok]
        if U.size == 0:
            break
        k = int(np.lexsort((U, -a[U], -b[U], z))[0])                  # smallest z, then largest b, largest a, smallest index
        t = int(U[k])
        kg += kg_term(float(b[t] - b[c]), -abs(float(z[k])))
        nseg += 1
        c = t
    return kg, nseg


def kg_hull(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    ok = np.isfinite(a) & np.isfinite(b)
    a, b = a[ok], b[ok]
    if a.size == 0:
        return 0.0, 0
    order = np.lexsort((a, b))
    a, b = a[order], b[order]
    keep = np.append(b[1:] != b[:-1], True)                           # of equal slopes the last one has the largest a
    a, b = a[keep], b[keep]
    stack, cut = [0], [-math.inf]                                     # cut[k]: where line stack[k] takes over from stack[k - 1]
    for i in range(1, a.size):
        while True:
            j = stack[-1]
            z = (a[j] - a[i]) / (b[i] - b[j])
            if z <= cut[-1] and len(stack) > 1:
                stack.pop()
                cut.pop()
            else:
                break
        stack.append(i)
        cut.append(z)
    cut.append(math.inf)
    Phi = [0.5 * math.erfc(-z / math.sqrt(2.0)) if math.isfinite(z) else (0.0 if z < 0 else 1.0) for z in cut]
    phi = [math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) if math.isfinite(z) else 0.0 for z in cut]
    tot = math.fsum(a[j] * (Phi[k + 1] - Phi[k]) + b[j] * (phi[k] - phi[k + 1]) for k, j in enumerate(stack))
    return tot - float(a.max()), len(stack)
