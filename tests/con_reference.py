"""NumPy references of constrained optimisation (include/bohip_con.h).  No device.  A helper, not a test module.

The float64 twin follows k_con_combine operation for operation (the device differs from it in exp, erfc, log, log1p -- libm's
here -- and in the contractions its compiler may form inside bohip_acq_eval's partials):
  term(mu, s2, thr, sense)             l_c = log Phi(z_c) and its two partials, broadcast
  combine(acq, params, thr, senses, mu, var)      value, logfeas, dmu, dvar [(C + 1), R] -- bohip_con_values
  gradient(acq, dmu, dvar, var, jmu, jvar)        the d gradient entries from the models' Jacobians, ascending m from +0.0
  record(values)                       the arg-max record of bohip_gp_score
  posterior_jac(model, Xs)             mu, var, grad mu, grad sigma^2 (UNMASKED) of a matern_reference.MaternGP -- bohip_gp_predict_grad
  score_con(models, acq, params, thr, senses, Xs)  the whole call on the members' twins
  moment_bounds / jac_bounds / propagate           the members' error bounds and their first-order propagation through the partials
The extended-precision evaluator (mpmath, 50 digits): mp_combine.
"""
import math

import numpy as np
import scipy.linalg as sl
from scipy.special import erfc

from logei_reference import logei
from matern_reference import acq_partials, acq_value, fx_of_r, k_of_r

C0, SQRT2, RSQRT2PI = 0.9189385332046728, 1.4142135623730951, 0.3989422804014327
SWITCH, CF_DEPTH = -4.0, 40
CMAX = 16
EPS = np.finfo(np.float64).eps
# The twin's worst error against the 50-digit evaluator over the crafted grid of the tests (every form, C = 0, 1, 5, R = 1, 257;
# |d| / max(1, |ref|), rounded up to two digits).  The value and d/dmu maxima are LogEI's next to its switch (logei_reference.WORST);
# d/dvar's is PI's and EI's phi z / (2 s2) at |z| ~ 12, where exp(-z^2 / 2) carries z^2 eps.  The host test bounds the twin by
# 2 x WORST (another libm), the device test bounds the kernel by 16 x WORST.
WORST = {"value": 2.6e-15, "dmu": 3.8e-14, "dvar": 1.8e-12}
# The same measurement for more than 5 constraints, over crafted_near's grid (every form, C = 6, 15, 16, R = 257; tests/test_con_host.py
# test_twin_against_mpmath_many_constraints): value 2.03e-15 (LogEI, C = 6: not larger, WORST's figure stands), d/dmu 1.47e-13 and
# d/dvar 1.21e-11 (both EI at C = 6: the objective's (D - z) phi / sigma and phi z / (2 s2) terms at sigma ~ 1e-3 -- this grid pairs
# other z with the small sigmas than `crafted` does; at C = 15 and 16 the figures are 3.3e-14 and 1.2e-12).  Rounded up to two digits.
# Granted for C > 5 only: the host test bounds the twin by 2 x WORST_MANY, the device test bounds the kernel by 16 x WORST_MANY.
WORST_MANY = {"value": 2.6e-15, "dmu": 1.5e-13, "dvar": 1.3e-11}
PRODUCT = ("EI", "PI")
FORMS = ("EI", "PI", "LogEI", "Feasibility")


def term(mu, s2, thr, sense):
    """(l, dl/dmu, dl/ds2) of one constraint, broadcast over mu and s2."""
    mu, s2 = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(s2, dtype=np.float64))
    s = float(sense)
    l = np.full(mu.shape, np.nan)
    dm, dv = l.copy(), l.copy()
    with np.errstate(all="ignore"):
        ok = np.isfinite(mu) & np.isfinite(s2) & (s2 >= 0.0)
        D = s * (mu - thr)
        zero = ok & (s2 == 0.0)
        l[zero] = np.where(D[zero] >= 0.0, 0.0, -np.inf)
        dm[zero], dv[zero] = 0.0, 0.0
        live = ok & ~zero
        sd = np.sqrt(s2[live])
        z = D[live] / sd
        ll, rho = np.empty_like(z), np.empty_like(z)
        pos, mid, deep = z > 0.0, (z <= 0.0) & (z > SWITCH), z <= SWITCH
        x = z[pos]
        phi = RSQRT2PI * np.exp(-0.5 * (x * x))
        Phic = 0.5 * erfc(x / SQRT2)
        ll[pos], rho[pos] = np.log1p(-Phic), phi / (1.0 - Phic)
        x = z[mid]
        phi = RSQRT2PI * np.exp(-0.5 * (x * x))
        Phi = 0.5 * erfc(-x / SQRT2)
        ll[mid], rho[mid] = np.log(Phi), phi / Phi
        x = z[deep]
        t = -x
        r = np.zeros_like(t)
        for k in range(CF_DEPTH, 1, -1):
            r = float(k) / (t + r)
        c1 = 1.0 / (t + r)
        rho[deep] = t + c1
        ll[deep] = (-0.5 * (x * x) - C0) - np.log(t + c1)
        l[live] = ll
        dm[live] = (s * rho) / sd
        dv[live] = -((z * rho) / (2.0 * s2[live]))
    return l, dm, dv


def objective(acq, params, mu, s2):
    """(a, da/dmu, da/ds2) of bohip_acq_eval's functor on arrays."""
    mu, s2 = np.asarray(mu, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    if acq == "LogEI":
        return logei(mu, s2, params[0])
    with np.errstate(all="ignore"):
        a = np.asarray(acq_value(acq, params, mu, s2), dtype=np.float64)
        am, av = np.full(mu.shape, np.nan), np.full(mu.shape, np.nan)
        for i in np.flatnonzero(np.isfinite(mu) & np.isfinite(s2) & (s2 >= 0.0)):
            am[i], av[i] = acq_partials(acq, params, float(mu[i]), float(s2[i]))
        a = np.where(np.isnan(mu) | np.isnan(s2) | (s2 < 0.0), np.nan, a)      # (the device's erf / sqrt of a NaN or negative variance)
    return a, am, av


def combine(acq, params, thr, senses, mu, var):
    """-> (value[R], logfeas[R], dmu[(C + 1), R], dvar[(C + 1), R])."""
    mu, var = np.atleast_2d(np.asarray(mu, dtype=np.float64)), np.atleast_2d(np.asarray(var, dtype=np.float64))
    C, R = mu.shape[0] - 1, mu.shape[1]
    pm, pv = np.zeros((C + 1, R)), np.zeros((C + 1, R))
    L = np.zeros(R)
    with np.errstate(all="ignore"):
        for c in range(C):
            l, pm[c + 1], pv[c + 1] = term(mu[c + 1], var[c + 1], thr[c], senses[c])
            L = L + l
        product = acq in PRODUCT
        e = np.ones(R)
        if acq == "Feasibility":
            f, am, av = L.copy(), np.zeros(R), np.zeros(R)
        else:
            a, am, av = objective(acq, params, mu[0], var[0])
            if product:
                e = np.exp(L)
                f = a * e
            else:
                f = a + L
        nan = np.isnan(f)
        dead = ~nan & ((f == -np.inf) | (product & (e == 0.0)))
        fo, fc = (e, f) if product else (np.ones(R), np.ones(R))
        pm[0], pv[0] = fo * am, fo * av
        pm[1:], pv[1:] = fc * pm[1:], fc * pv[1:]
        if acq == "Feasibility":
            pm[0], pv[0] = 0.0, 0.0
        pm[:, dead], pv[:, dead] = 0.0, 0.0
        pm[:, nan], pv[:, nan] = np.nan, np.nan
    return f, L, pm, pv


def gradient(acq, pm, pv, var, jmu, jvar):
    """grad[R, d] = sum_m pm[m] jmu[m] + (var[m] > 0) pv[m] jvar[m], ascending m from +0.0; jmu, jvar [(C + 1), R, d].  (A dead
    score has zero partials, so its gradient is the sum of zeros.)"""
    M, R, d = jmu.shape
    g = np.zeros((R, d))
    with np.errstate(all="ignore"):
        for m in range(1 if acq == "Feasibility" else 0, M):
            g = g + pm[m][:, None] * jmu[m]
            g = np.where((var[m] > 0.0)[:, None], g + pv[m][:, None] * jvar[m], g)
    return g


def record(vals):
    """bohip_gp_score's arg-max: first maximum under strict '>' from -Inf, NaN never wins, (-Inf, -1) if nothing can win."""
    v = np.asarray(vals, dtype=np.float64)
    ok = v > -np.inf
    if not ok.any():
        return -math.inf, -1
    best = np.max(v[ok])
    return float(best), int(np.flatnonzero(ok & (v == best))[0])


def posterior_jac(ref, Xs):
    """(mu[R], var[R], dmu[R, d], dvar[R, d]) of a MaternGP at the rows of Xs; dvar is reported unmasked."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    diff = Xs[:, None, :] - ref.X[None, :, :]                              # (R, N, d)
    r = (diff * diff) @ ref.il2                                            # (R, N)
    ks = k_of_r(ref.fam, r, ref.s2f)
    dk = fx_of_r(ref.fam, r, ref.s2f)[:, :, None] * diff * ref.il2         # (R, N, d)
    V = sl.solve_triangular(ref.L, ks.T, lower=True)                       # (N, R)
    U = sl.solve_triangular(ref.L, V, lower=True, trans="T")               # cK^-1 k*
    mu = ref.beta + ks @ ref.alpha
    var = np.maximum(ref.s2f - np.sum(V * V, axis=0), 0.0)
    return mu, var, np.einsum("rnd,n->rd", dk, ref.alpha), -2.0 * np.einsum("rnd,nr->rd", dk, U)


def score_con(models, acq, params, thr, senses, Xs, want_grad=True):
    """The whole call on the members' twins (models[0] the objective, None under "Feasibility" if it has no observations).
    -> dict(scores, logfeas, grad[R, d], mu, var, pm, pv, jmu, jvar, best_val, best_idx)."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    R, d = Xs.shape
    M = len(models)
    mu, var = np.full((M, R), np.nan), np.full((M, R), np.nan)
    jmu, jvar = np.zeros((M, R, d)), np.zeros((M, R, d))
    for m, ref in enumerate(models):
        if m == 0 and acq == "Feasibility":
            continue
        mu[m], var[m], jmu[m], jvar[m] = posterior_jac(ref, Xs)
    f, L, pm, pv = combine(acq, params, thr, senses, mu, var)
    g = gradient(acq, pm, pv, var, jmu, jvar) if want_grad else None
    bv, bi = record(f)
    return dict(scores=f, logfeas=L, grad=g, mu=mu, var=var, pm=pm, pv=pv, jmu=jmu, jvar=jvar, best_val=bv, best_idx=bi)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def mu_floor(alpha, s2f):
    return 64 * EPS * s2f * np.abs(alpha).sum()


def var_tol(ref, N, s2f, rel=1e-6):
    return rel * np.abs(ref) + 64 * N * EPS * s2f


def moment_bounds(ref, mu, var):
    """The project's bounds on a member's moments: 1e-6 |mu| + mu_floor, var_tol."""
    return 1e-6 * np.abs(mu) + mu_floor(ref.alpha, ref.s2f), var_tol(var, ref.N, ref.s2f)


def jac_bound(j):
    """test_matern_gpu's bound on a gradient: rtol 1e-6, atol 1e-9 max|g_ref| + 1e-12."""
    return 1e-6 * np.abs(j) + 1e-9 * np.abs(j).max() + 1e-12


def propagate(models, acq, tw):
    """First-order bounds of score_con's outputs from the members' bounds and the twin's partials:
    score: sum_m |pm| d_mu_m + |pv| d_var_m + 1e-6 |score| + 1e-12;
    grad:  sum_m |pm| d_jmu_m + [var > 0] |pv| d_jvar_m  (the Jacobians' own bounds through the partials), + 1e-6 |grad| + 1e-12."""
    R = tw["scores"].size
    ts = 1e-6 * np.abs(tw["scores"]) + 1e-12
    tg = 1e-6 * np.abs(tw["grad"]) + 1e-12 if tw["grad"] is not None else None
    for m, ref in enumerate(models):
        if m == 0 and acq == "Feasibility":
            continue
        dm, dv = moment_bounds(ref, tw["mu"][m], tw["var"][m])
        ts = ts + np.abs(tw["pm"][m]) * dm + np.abs(tw["pv"][m]) * dv
        if tg is not None:
            tg = tg + np.abs(tw["pm"][m])[:, None] * jac_bound(tw["jmu"][m]) \
                + np.where((tw["var"][m] > 0)[:, None], np.abs(tw["pv"][m])[:, None] * jac_bound(tw["jvar"][m]), 0.0)
    return ts, tg


# ---- extended precision ----------------------------------------------------------------------------------------------------------------
def mp_combine(acq, params, thr, senses, mu, var, dps=50):
    """The three score forms and their partials at 50 digits, from exact formulas (ncdf, npdf): one candidate, mu and var of length
    C + 1.  -> (value, logfeas, dmu[C + 1], dvar[C + 1]) as floats; +-inf where the exact value is."""
    import mpmath as mp

    with mp.workdps(dps):
        C = len(mu) - 1
        L = mp.mpf(0)
        dl = []
        for c in range(C):
            m, v, t, s = mp.mpf(float(mu[c + 1])), mp.mpf(float(var[c + 1])), mp.mpf(float(thr[c])), int(senses[c])
            if v == 0:
                L = L + (mp.mpf(0) if s * (m - t) >= 0 else mp.mpf("-inf"))
                dl.append((mp.mpf(0), mp.mpf(0)))
                continue
            sd = mp.sqrt(v)
            z = s * (m - t) / sd
            Phi = mp.ncdf(z)
            rho = mp.npdf(z) / Phi
            L = L + mp.log(Phi)
            dl.append((s * rho / sd, -z * rho / (2 * v)))
        if acq == "Feasibility":
            f, am, av = L, mp.mpf(0), mp.mpf(0)
            a = None
        else:
            m, v, tau = mp.mpf(float(mu[0])), mp.mpf(float(var[0])), mp.mpf(float(params[0]))
            D = m - tau
            if v == 0:
                if acq == "EI":
                    a, am, av = (D if D > 0 else mp.mpf(0)), (mp.mpf(1) if D > 0 else mp.mpf(0)), mp.mpf(0)
                elif acq == "PI":
                    a, am, av = (mp.mpf(1) if D > 0 else mp.mpf(0)), mp.mpf(0), mp.mpf(0)
                else:
                    a, am, av = (mp.log(D) if D > 0 else mp.mpf("-inf")), (1 / D if D > 0 else mp.mpf(0)), mp.mpf(0)
            else:
                sd = mp.sqrt(v)
                z = D / sd
                Phi, phi = mp.ncdf(z), mp.npdf(z)
                if acq == "EI":      # the reference's form: D Phi(z) + phi(z)  (sqrt(s2) * normal_pdf(D, s2) = phi(z))
                    a, am, av = D * Phi + phi, Phi + (D - z) * phi / sd, (D - z) * phi * (-z / (2 * v))
                elif acq == "PI":
                    a, am, av = Phi, phi / sd, phi * (-z / (2 * v))
                else:
                    h = phi + z * Phi
                    a, am, av = mp.log(sd) + mp.log(h), Phi / (sd * h), phi / (2 * v * h)
            f = a * mp.exp(L) if acq in PRODUCT else a + L
        if acq in PRODUCT:
            e = mp.exp(L)
            pm = [e * am] + [f * d[0] for d in dl]
            pv = [e * av] + [f * d[1] for d in dl]
        else:
            pm = [am] + [d[0] for d in dl]
            pv = [av] + [d[1] for d in dl]
        if f == mp.mpf("-inf") or (acq in PRODUCT and L == mp.mpf("-inf")):
            pm, pv = [mp.mpf(0)] * (C + 1), [mp.mpf(0)] * (C + 1)
        return float(f), float(L), np.array([float(x) for x in pm]), np.array([float(x) for x in pv])


# ---- crafted moments ---------------------------------------------------------------------------------------------------------------------
def crafted(C, R, seed=0, tau=0.3):
    """(thr[C], senses[C], mu[(C + 1), R], var[(C + 1), R]): every constraint's z = s (mu - t) / sigma runs over [-40, 10] (both sides
    of the switch at -4 and of 0, in an order of its own), sigma over [1e-3, 10]; the objective's z over [-12, 6].  Where R allows
    it: sigma^2 = 0 on both sides of (and on) the threshold, z next to the switch, and one NaN moment per row kind."""
    rng = np.random.default_rng(seed)
    thr = rng.uniform(-2.0, 2.0, C)
    senses = np.array([1 if c % 2 == 0 else -1 for c in range(C)], dtype=np.int64)
    mu, var = np.empty((C + 1, R)), np.empty((C + 1, R))
    sd0 = 10.0 ** rng.uniform(-3, 1, R)
    z0 = rng.permutation(np.linspace(-12.0, 6.0, R)) if R > 1 else np.array([0.7])
    mu[0], var[0] = tau + z0 * sd0, sd0 * sd0
    for c in range(C):
        sd = 10.0 ** rng.uniform(-3, 1, R)
        z = rng.permutation(np.linspace(-40.0, 10.0, R)) if R > 1 else np.array([-5.0 if c % 2 else 0.4])
        if R >= 16:
            z[:6] = [-4.0, np.nextafter(-4.0, 0.0), np.nextafter(-4.0, -5.0), 0.0, -39.5, 9.5]
        mu[c + 1], var[c + 1] = thr[c] + senses[c] * z * sd, sd * sd
        if R >= 16:
            var[c + 1, 6:9] = 0.0
            mu[c + 1, 6:9] = [thr[c] + 0.5, thr[c] - 0.5, thr[c]]
    if R >= 16:
        var[0, 9] = 0.0                       # a clamped objective above and below tau
        mu[0, 9:11] = [tau + 0.25, tau - 0.25]
        var[0, 10] = 0.0
        mu[0, 11] = np.nan                    # NaN moments: the objective's mean, a constraint's variance
        if C:
            var[C, 12] = np.nan
    return thr, senses, mu, var


def crafted_near(C, R, seed=0, tau=0.3):
    """(thr[C], senses[C], mu[(C + 1), R], var[(C + 1), R]) for many constraints: `crafted` sends every constraint's z down to -40, so
    with C = 16 the product forms are 0 at all but a few candidates.  Here z runs over [-1, 4] (both sides of 0), which keeps
    L = sum_c log Phi(z_c) within a few units of 0, and a minority of entries in EVERY constraint row, at columns of the row's own
    (16 c + k) mod R, are the hard ones: k = 0 the deep tail z = -40, 1 and 2 the neighbours of the switch at -4, 3 to 5
    sigma^2 = 0 above, below and on the threshold, 6 a NaN (mean in even rows, variance in odd ones).  Neighbouring constraints
    differ in threshold (by more than 1) and in sense; no two thresholds are equal.  The objective's z runs over [-12, 6] as in
    `crafted`, with a clamped variance on both sides of tau and a NaN mean in the last columns.  R >= 17."""
    assert R >= 17
    rng = np.random.default_rng(seed)
    thr = np.array([(-1.0) ** c * (0.5 + 0.1 * c) for c in range(C)])
    senses = np.array([1 if c % 2 == 0 else -1 for c in range(C)], dtype=np.int64)
    mu, var = np.empty((C + 1, R)), np.empty((C + 1, R))
    sd0 = 10.0 ** rng.uniform(-3, 1, R)
    z0 = rng.permutation(np.linspace(-12.0, 6.0, R))
    mu[0], var[0] = tau + z0 * sd0, sd0 * sd0
    var[0, R - 3], var[0, R - 2] = 0.0, 0.0
    mu[0, R - 3:] = [tau + 0.25, tau - 0.25, np.nan]
    for c in range(C):
        sd = 10.0 ** rng.uniform(-3, 1, R)
        z = rng.permutation(np.linspace(-1.0, 4.0, R))
        k = [(16 * c + i) % R for i in range(7)]
        z[k[:3]] = [-40.0, np.nextafter(-4.0, 0.0), np.nextafter(-4.0, -5.0)]
        mu[c + 1], var[c + 1] = thr[c] + senses[c] * z * sd, sd * sd
        var[c + 1, k[3:6]] = 0.0
        mu[c + 1, k[3:6]] = [thr[c] + 0.5, thr[c] - 0.5, thr[c]]
        if c % 2 == 0:
            mu[c + 1, k[6]] = np.nan
        else:
            var[c + 1, k[6]] = np.nan
    return thr, senses, mu, var


def worst_share(got, ref, const):
    """max |got - ref| / (const max(1, |ref|)) over the finite references; the others must match exactly (NaN with NaN)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), ("non-finite rows differ", got[~fin][:4], ref[~fin][:4])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / (const * np.maximum(1.0, np.abs(ref[fin])))))


def mp_table(acq, params, thr, senses, mu, var):
    """mp_combine over the columns whose moments are finite -> (value, logfeas, dmu, dvar) with NaN columns elsewhere."""
    M, R = mu.shape
    f, L, pm, pv = np.full(R, np.nan), np.full(R, np.nan), np.full((M, R), np.nan), np.full((M, R), np.nan)
    rows = slice(1, None) if acq == "Feasibility" else slice(None)
    for j in range(R):
        if np.all(np.isfinite(mu[rows, j])) and np.all(np.isfinite(var[rows, j])):
            f[j], L[j], pm[:, j], pv[:, j] = mp_combine(acq, params, thr, senses, mu[:, j], var[:, j])
    return f, L, pm, pv
