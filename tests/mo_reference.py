"""NumPy references of two-objective optimisation (include/bohip_mo.h).  No device.  A helper, not a test module.

The float64 twin follows k_ehvi operation for operation (the device differs from it in exp and erfc -- libm's here):
  front(Y, ref)                        the observed front [2, n_front] and its hypervolume -- bohip_mo_front
  psi(mu, s2, sd, t)                   Psi = E[(f - t)+], Phi, phi, broadcast
  ehvi(front, ref, mu, var)            value[R], dmu[2, R], dvar[2, R] in the kernel's summation order -- bohip_mo_ehvi_values
  gradient(pm, pv, var, jmu, jvar)     the d gradient entries from the two models' Jacobians, ascending m from +0.0
  record(values)                       the arg-max record of bohip_gp_score
  score_mo(models, front, ref, Xs)     the whole call on the members' twins (matern_reference.MaternGP)
  propagate(models, tw)                the members' error bounds propagated to first order through the twin's partials
  hvi(front, ref, y)                   the hypervolume improvement of points y [2, S] (what EHVI is the expectation of)
The extended-precision evaluator (mpmath, 50 digits): mp_ehvi, mp_table (cached under tests/golden/ where it is slow).
"""
import hashlib
import math
import os

import numpy as np
from scipy.special import erfc

import con_reference as cr

SQRT2, RSQRT2PI = 1.4142135623730951, 0.3989422804014327
G = 16                                  # BOHIP_MO_GROUP
FRONT_MAX = 1024                        # BOHIP_MO_FRONT_MAX
EPS = np.finfo(np.float64).eps
KEYS = ("value", "dmu1", "dvar1", "dmu2", "dvar2")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The twin's worst error against the 50-digit evaluator over the crafted grid of tests/test_mo_host.py (n_front = 0, 1, 2, 15, 16,
# 17, 64, 1024 at R = 257, seeds grid_seed(n_front, R)), measured with glibc's exp and SciPy's erfc as
# |twin - ref| / max(S, 1e-300), S the sum the strip differences cancel against (mp_ehvi), and rounded up to two digits:
# value, d/dmu1 and d/dvar1 1.4839e-10 (n_front = 15, column 237, S = 1.3e-289), d/dmu2 and d/dvar2 1.4027e-10 (n_front = 17,
# column 88, S = 3.9e-274).  The maxima sit where EVERY strip is deep in a tail: the measure is relative to S, so a candidate whose
# whole score is 1e-289 counts like any other, and there Psi = sd phi + D Phi cancels to z^-2 of its terms while exp(-z^2 / 2)
# carries z^2 eps / 2 -- z^4 eps / 2 = 1e-10 at z = -36, the last z before the terms underflow.  Away from the tails (S > 1e-30)
# the same grid gives 1.84e-12.  The host test bounds the twin by 2 x WORST (another libm), the device tests bound the kernel by
# 16 x WORST, the convention of con_reference.WORST.
WORST = {"value": 1.5e-10, "dmu1": 1.5e-10, "dvar1": 1.5e-10, "dmu2": 1.5e-10, "dvar2": 1.5e-10}


# ---- the front ------------------------------------------------------------------------------------------------------------------------
def front(Y, ref):
    """-> (front[2, n_front], hv): the columns of Y [2, n] that strictly dominate ref and are not weakly dominated by another column,
    ascending in f1 (descending in f2), of equal points one; hv = sum_i (f1_i - f1_{i-1}) (f2_i - r2), ascending i from +0.0."""
    Y = np.asarray(Y, dtype=np.float64).reshape(2, -1)
    if not np.all(np.isfinite(Y)) or not np.all(np.isfinite(ref)):
        raise ValueError("not finite")
    pts = sorted(((a, b) for a, b in Y.T if a > ref[0] and b > ref[1]), key=lambda p: (-p[0], -p[1]))
    keep, top = [], -math.inf
    for a, b in pts:
        if b > top:
            keep.append((a, b))
            top = b
    keep.reverse()
    hv, prev = 0.0, float(ref[0])
    for a, b in keep:
        hv += (a - prev) * (b - ref[1])
        prev = a
    return np.array(keep, dtype=np.float64).reshape(-1, 2).T.copy(), hv


def corners(fr, ref):
    """c[0 .. n + 1] (c[0] = r1, c[n + 1] = +Inf) and b[0 .. n] (b[n] = r2): strip s spans [c[s], c[s + 1]] above b[s]."""
    fr = np.asarray(fr, dtype=np.float64).reshape(2, -1)
    return np.concatenate([[ref[0]], fr[0], [np.inf]]), np.concatenate([fr[1], [ref[1]]])


def hvi(fr, ref, y):
    """The hypervolume improvement of each column of y [2, S] over the front: the area of the box below y that no front point
    dominates, strip by strip."""
    c, b = corners(fr, ref)
    y = np.asarray(y, dtype=np.float64).reshape(2, -1)
    w = np.clip(np.minimum(y[0][:, None], c[None, 1:]) - c[None, :-1], 0.0, None)
    return np.sum(w * np.clip(y[1][:, None] - b[None, :], 0.0, None), axis=1)


# ---- the twin of k_ehvi ---------------------------------------------------------------------------------------------------------------
def psi(mu, s2, sd, t):
    """(Psi, Phi, phi) at threshold t, broadcast: mo_psi of kernels_mo.hip."""
    mu, s2, sd, t = np.broadcast_arrays(mu, s2, sd, t)
    with np.errstate(all="ignore"):
        D = mu - t
        z = D / sd
        Phi = 0.5 * erfc(-z / SQRT2)
        phi = RSQRT2PI * np.exp(-0.5 * (z * z))
        P = sd * phi + D * Phi
        zero = s2 == 0.0
        P = np.where(zero, np.where(D > 0.0, D, 0.0), P)
        Phi = np.where(zero, np.where(D > 0.0, 1.0, 0.0), Phi)
        phi = np.where(zero, 0.0, phi)
        inf = t == np.inf
        return np.where(inf, 0.0, P), np.where(inf, 0.0, Phi), np.where(inf, 0.0, phi)


def group_sum(terms):
    """The kernel's order over the strips (last axis): lane g adds strips g, g + 16, ... in ascending order from +0.0, then the
    butterfly a_g <- a_g + a_{g xor o}, o = 8, 4, 2, 1; lane 0's result."""
    R, K = terms.shape
    acc = np.zeros((R, G))
    for s0 in range(0, K, G):
        w = min(G, K - s0)
        acc[:, :w] = acc[:, :w] + terms[:, s0:s0 + w]
    lanes = np.arange(G)
    for o in (8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def ehvi(fr, ref, mu, var):
    """-> (value[R], dmu[2, R], dvar[2, R]) of bohip_mo_ehvi_values."""
    mu, var = np.atleast_2d(np.asarray(mu, dtype=np.float64)), np.atleast_2d(np.asarray(var, dtype=np.float64))
    c, b = corners(fr, ref)
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(mu).all(axis=0) & np.isfinite(var).all(axis=0) & (var >= 0.0).all(axis=0))
        sd = np.sqrt(var)
        P1, F1, f1 = psi(mu[0][:, None], var[0][:, None], sd[0][:, None], c[None, :])
        hP, hF, hf = psi(mu[1][:, None], var[1][:, None], sd[1][:, None], b[None, :])
        dlt = P1[:, :-1] - P1[:, 1:]
        v = group_sum(dlt * hP)
        am1 = group_sum((F1[:, :-1] - F1[:, 1:]) * hP)
        as1 = group_sum((f1[:, :-1] - f1[:, 1:]) * hP)
        am2 = group_sum(dlt * hF)
        as2 = group_sum(dlt * hf)
        q1 = np.where(var[0] > 0.0, as1 / (2.0 * sd[0]), 0.0)
        q2 = np.where(var[1] > 0.0, as2 / (2.0 * sd[1]), 0.0)
        pm, pv = np.stack([am1, am2]), np.stack([q1, q2])
        v = np.where(bad, np.nan, v)
        pm[:, bad], pv[:, bad] = np.nan, np.nan
    return v, pm, pv


def gradient(pm, pv, var, jmu, jvar):
    """grad[R, d] = sum_m pm[m] jmu[m] + (var[m] > 0) pv[m] jvar[m], ascending m from +0.0; jmu, jvar [2, R, d]."""
    g = np.zeros(jmu.shape[1:])
    with np.errstate(all="ignore"):
        for m in range(2):
            g = g + pm[m][:, None] * jmu[m]
            g = np.where((var[m] > 0.0)[:, None], g + pv[m][:, None] * jvar[m], g)
    return g


record = cr.record


def score_mo(models, fr, ref, Xs, want_grad=True):
    """The whole call on the members' twins -> dict(scores, grad[R, d], mu, var, pm, pv, jmu, jvar, best_val, best_idx)."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    R, d = Xs.shape
    mu, var, jmu, jvar = np.empty((2, R)), np.empty((2, R)), np.empty((2, R, d)), np.empty((2, R, d))
    for m, gp in enumerate(models):
        mu[m], var[m], jmu[m], jvar[m] = cr.posterior_jac(gp, Xs)
    f, pm, pv = ehvi(fr, ref, mu, var)
    g = gradient(pm, pv, var, jmu, jvar) if want_grad else None
    bv, bi = record(f)
    return dict(scores=f, grad=g, mu=mu, var=var, pm=pm, pv=pv, jmu=jmu, jvar=jvar, best_val=bv, best_idx=bi)


def propagate(models, tw):
    """First-order bounds of score_mo's outputs from the members' bounds (con_reference.moment_bounds, jac_bound) and the twin's
    partials:  score: sum_m |pm| d_mu_m + |pv| d_var_m + 1e-6 |score| + 1e-12;
    grad: sum_m |pm| d_jmu_m + [var > 0] |pv| d_jvar_m + 1e-6 |grad| + 1e-12."""
    ts = 1e-6 * np.abs(tw["scores"]) + 1e-12
    tg = 1e-6 * np.abs(tw["grad"]) + 1e-12 if tw["grad"] is not None else None
    for m, gp in enumerate(models):
        dm, dv = cr.moment_bounds(gp, tw["mu"][m], tw["var"][m])
        ts = ts + np.abs(tw["pm"][m]) * dm + np.abs(tw["pv"][m]) * dv
        if tg is not None:
            tg = tg + np.abs(tw["pm"][m])[:, None] * cr.jac_bound(tw["jmu"][m]) \
                + np.where((tw["var"][m] > 0)[:, None], np.abs(tw["pv"][m])[:, None] * cr.jac_bound(tw["jvar"][m]), 0.0)
    return ts, tg


# ---- extended precision ----------------------------------------------------------------------------------------------------------------
def mp_ehvi(fr, ref, mu, var, dps=50, as_float=True):
    """One candidate at 50 digits from the exact formulas: mu, var of length 2 (mpmath numbers or floats).
    -> (vals, scales): vals = (EHVI, d/dmu1, d/ds2_1, d/dmu2, d/ds2_2), scales the sums S each of them cancels against
    (the same sums with + in place of the strip difference)."""
    import mpmath as mp

    with mp.workdps(dps):
        c, b = corners(fr, ref)
        m1, v1, m2, v2 = (mp.mpf(x) for x in (mu[0], var[0], mu[1], var[1]))

        def three(m, v, t):
            if t == np.inf:
                return mp.mpf(0), mp.mpf(0), mp.mpf(0)
            D = m - mp.mpf(float(t))
            if v == 0:
                return (D if D > 0 else mp.mpf(0)), (mp.mpf(1) if D > 0 else mp.mpf(0)), mp.mpf(0)
            sd = mp.sqrt(v)
            z = D / sd
            Phi, phi = mp.ncdf(z), mp.npdf(z)
            return sd * phi + D * Phi, Phi, phi

        one = [three(m1, v1, t) for t in c]
        two = [three(m2, v2, t) for t in b]
        vals, scales = [mp.mpf(0)] * 5, [mp.mpf(0)] * 5
        h1 = 1 / (2 * mp.sqrt(v1)) if v1 > 0 else mp.mpf(0)
        h2 = 1 / (2 * mp.sqrt(v2)) if v2 > 0 else mp.mpf(0)
        for s in range(len(b)):
            (lP, lF, lf), (uP, uF, uf), (hP, hF, hf) = one[s], one[s + 1], two[s]
            for k, (lo, up, w) in enumerate(((lP, uP, hP), (lF, uF, hP), (lf * h1, uf * h1, hP), (lP, uP, hF), (lP, uP, hf * h2))):
                vals[k] = vals[k] + (lo - up) * w
                scales[k] = scales[k] + (lo + up) * w
        if as_float:
            return [float(x) for x in vals], [float(x) for x in scales]
        return vals, scales


def _case_file(n_front, R, seed):
    return os.path.join(GOLDEN, f"mo_mp_n{n_front}_R{R}_s{seed}.npz")


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def mp_table(fr, ref, mu, var, cache=None):
    """mp_ehvi over the columns whose moments are valid -> dict of KEYS -> [R] and "S_" + key -> [R]; NaN columns elsewhere.
    cache = (n_front, R, seed) of `crafted`: the table is read from tests/golden/ when a file recorded for exactly these inputs
    (by their SHA-256) is there -- at n_front = 1024 the 50-digit evaluation takes minutes -- and computed otherwise."""
    digest = _digest(fr, ref, mu, var)
    if cache is not None and os.path.exists(_case_file(*cache)):
        z = np.load(_case_file(*cache))
        if str(z["digest"]) == digest:
            return {k: z[k] for k in z.files if k != "digest"}
    R = mu.shape[1]
    out = {k: np.full(R, np.nan) for k in KEYS}
    out.update({"S_" + k: np.full(R, np.nan) for k in KEYS})
    for j in range(R):
        if np.all(np.isfinite(mu[:, j])) and np.all(np.isfinite(var[:, j])) and np.all(var[:, j] >= 0.0):
            vals, scales = mp_ehvi(fr, ref, mu[:, j], var[:, j])
            for k, v, s in zip(KEYS, vals, scales):
                out[k][j], out["S_" + k][j] = v, s
    return out


def write_golden(n_front, R, seed):
    """Records the 50-digit table of crafted(n_front, R, seed) under tests/golden/ (development use: python -c ...)."""
    fr, ref, mu, var = crafted(n_front, R, seed)
    tab = mp_table(fr, ref, mu, var)
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez(_case_file(n_front, R, seed), digest=_digest(fr, ref, mu, var), **tab)
    return tab


def shares(got, tab, bound):
    """got = (value, dmu[2, R], dvar[2, R]); -> dict key -> max |got - ref| / (bound[key] max(S, 1e-300)) over the valid columns;
    the others must be NaN in every output."""
    f, pm, pv = got
    mine = dict(zip(KEYS, (f, pm[0], pv[0], pm[1], pv[1])))
    ok = np.isfinite(tab["value"])
    out = {}
    for k in KEYS:
        assert np.all(np.isnan(mine[k][~ok])), (k, "a column with a NaN or negative moment must be NaN")
        assert np.all(np.isfinite(mine[k][ok])), k
        out[k] = float(np.max(np.abs(mine[k][ok] - tab[k][ok]) / (bound[k] * np.maximum(tab["S_" + k][ok], 1e-300)))) if ok.any() else 0.0
    return out


# ---- crafted fronts and moments ------------------------------------------------------------------------------------------------------
def grid_seed(n_front, R):
    return 1000 * n_front + R


def crafted(n_front, R, seed=0):
    """(front[2, n], ref[2], mu[2, R], var[2, R]): a front of n points over [-2, 2]^2 above ref = (-2.25, -2.125); every objective's
    z = (mu - t) / sigma against a corner t of its own (one of the front's coordinates in that objective or ref's; the nearest one
    wherever sigma is small against the front's spacing) runs over [-12, 8] in an order of its own, sigma over [1e-3, 10].  With
    R >= 16, columns 0..8 carry sigma^2 = 0 in objective 1 (above, below and on a corner), in objective 2 likewise, and in both (above
    the front, below ref, on corners), column 9 a NaN mean, 10 a NaN variance, 11 a negative variance."""
    rng = np.random.default_rng(seed)
    ref = np.array([-2.25, -2.125])
    fr = np.stack([np.sort(rng.uniform(-2.0, 2.0, n_front)), -np.sort(-rng.uniform(-2.0, 2.0, n_front))])
    assert n_front < 2 or (np.all(np.diff(fr[0]) > 0) and np.all(np.diff(fr[1]) < 0))
    mu, var = np.empty((2, R)), np.empty((2, R))
    for m in range(2):
        pool = np.concatenate([[ref[m]], fr[m]])
        t = pool[rng.integers(0, pool.size, R)]
        sd = 10.0 ** rng.uniform(-3, 1, R)
        z = rng.permutation(np.linspace(-12.0, 8.0, R)) if R > 1 else np.array([0.7 - m])
        mu[m], var[m] = t + z * sd, sd * sd
    if R >= 16:
        t1 = fr[0, n_front // 2] if n_front else ref[0]
        t2 = fr[1, n_front // 2] if n_front else ref[1]
        var[0, 0:3] = 0.0
        mu[0, 0:3] = [t1 + 0.25, t1 - 0.25, t1]
        var[1, 3:6] = 0.0
        mu[1, 3:6] = [t2 + 0.25, t2 - 0.25, t2]
        var[:, 6:9] = 0.0
        mu[:, 6] = [2.5, 2.25]
        mu[:, 7] = [ref[0] - 0.5, ref[1] - 0.25]
        mu[:, 8] = [t1, t2]
        mu[0, 9] = np.nan
        var[1, 10] = np.nan
        var[0, 11] = -1e-3
    return fr, ref, mu, var
