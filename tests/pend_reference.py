"""CPU references for pending evaluations (include/bohip_pend.h) -- TEST INFRASTRUCTURE ONLY.  No device.

Two independent statements of "the acquisition averaged over fantasised outcomes at the pending points" (Snoek, Larochelle & Adams
2012, section 3.2), over ``batch_reference.gp_factory`` so that every kernel id is covered:

  * ``refit_per_fantasy``  the definition: append (Xp, y_f,s) to the data, refit the whole model, score, average over s;
  * ``recurrence``         what the library computes: one fit, b(x) = L_p^-1 (k(x, Xp) - v(x)'V_p), mu_s = mu + b'z_s, s^2 = sigma^2 - |b|^2.

Both take the standard normals Z (S x p, row s = z_s) as an argument; the device's are bohip_thompson_normal(seed, s, i).  S = 0 (the
Kriging believer) is Z = zeros((1, p)).  Arrays are row-observation: X (N, d), Xp (p, d), Xs (R, d).
"""
import math

import numpy as np
import scipy.linalg as sl

from logei_reference import logei
from matern_reference import acq_value
from oracle.oracle import NOISE_EPS

TAU_ACQS = ("EI", "PI", "LogEI")
EPS = np.finfo(np.float64).eps


def acq(name, params, mu, s2):
    """One acquisition on (mu, sigma^2) arrays: the reference's functors, LogEI from the twin of acq_log.h."""
    if name == "LogEI":
        return np.asarray(logei(mu, s2, params[0])[0], dtype=np.float64)
    return np.asarray(acq_value(name, params, mu, s2), dtype=np.float64)


def with_tau(name, params, tau):
    return [tau] + list(params[1:]) if name in TAU_ACQS else list(params)


def average(name, values):
    """The mean over the fantasies in their order (rows of `values`, S x R); LogEI: log-mean-exp, max-shifted."""
    values = np.asarray(values, dtype=np.float64)
    S = values.shape[0]
    if name != "LogEI":
        tot = np.zeros(values.shape[1])
        for row in values:
            tot = tot + row
        return tot / S
    with np.errstate(all="ignore"):
        m = values.max(axis=0)
        tot = np.zeros(values.shape[1])
        for row in values:
            tot = tot + np.where(row == m, 1.0, np.exp(row - m))
        return np.where(m == -np.inf, -np.inf, m + np.log(tot / S))


def pending_moments(gp, Xp):
    """(mu_p, Sigma_p, V_p): the model's predictive mean and covariance of the NOISY outcomes at Xp (nu on the diagonal)."""
    Xp = np.atleast_2d(Xp)
    Kp = gp.cov(gp.X, Xp)
    Vp = sl.solve_triangular(gp.L, Kp, lower=True)
    nu = math.exp(2.0 * gp.lognoise) + NOISE_EPS
    return gp.beta + Kp.T @ gp.alpha, gp.cov(Xp, Xp) - Vp.T @ Vp + nu * np.eye(len(Xp)), Vp


def fantasies(mu_p, Sigma_p, Z):
    """y_f (S x p): row s = mu_p + L_p z_s."""
    return mu_p[None, :] + np.asarray(Z, float) @ np.linalg.cholesky(Sigma_p).T


def _taus(name, params, Yf, raise_tau):
    if name not in TAU_ACQS:
        return [None] * len(Yf)
    return [max(params[0], float(yf.max())) if raise_tau else params[0] for yf in Yf]


def refit_moments(factory, X, y, Xp, Xs, Z):
    """The refits of the definition, once for every acquisition: dict(mu_s (S x R), var, Yf, mu, mu_p, Sigma_p, asum)."""
    X, y, Xp, Xs = np.asarray(X, float), np.asarray(y, float), np.atleast_2d(Xp), np.atleast_2d(Xs)
    gp = factory(X, y)
    mu_p, Sigma_p, _ = pending_moments(gp, Xp)
    Yf = fantasies(mu_p, Sigma_p, Z)
    mu0, _ = gp.predict(Xs)
    asum = float(np.abs(gp.alpha).sum())
    mus, var = [], None
    for yf in Yf:
        gs = factory(np.vstack([X, Xp]), np.concatenate([y, yf]))
        mu_s, var = gs.predict(Xs)
        asum = max(asum, float(np.abs(gs.alpha).sum()))
        mus.append(mu_s)
    return dict(mu_s=np.array(mus), var=np.maximum(var, 0.0), Yf=Yf, mu=mu0, mu_p=mu_p, Sigma_p=Sigma_p, asum=asum)


def score_refits(mom, name, params, raise_tau=False):
    """refit_per_fantasy's result from refit_moments' refits."""
    each = np.array([acq(name, with_tau(name, params, tau), mu_s, mom["var"])
                     for mu_s, tau in zip(mom["mu_s"], _taus(name, params, mom["Yf"], raise_tau))])
    return dict(score=average(name, each), mu=mom["mu"], var=mom["var"], each=each, mu_p=mom["mu_p"], Sigma_p=mom["Sigma_p"],
                asum=mom["asum"])


def refit_per_fantasy(factory, X, y, Xp, Xs, name, params, Z, raise_tau=False):
    """The definition.  Returns dict(score, mu, var, each (S x R), mu_p, Sigma_p, asum): mu the resident mean, var the conditioned
    variance (of the last refit; it is the same for every fantasy), asum the largest sum|alpha| of the fits (the bound's floor)."""
    return score_refits(refit_moments(factory, X, y, Xp, Xs, Z), name, params, raise_tau)


def recurrence(factory, X, y, Xp, Xs, name, params, Z, raise_tau=False, condition=True, log_of_mean=True):
    """The formulas of include/bohip_pend.h from ONE fit.  condition=False drops the conditioning (b = 0), log_of_mean=False averages
    LogEI's logarithms instead of taking the log-mean-exp: the two mistakes the tests must be able to see.  Also returns B (R x p)."""
    X, y, Xp, Xs = np.asarray(X, float), np.asarray(y, float), np.atleast_2d(Xp), np.atleast_2d(Xs)
    gp = factory(X, y)
    mu_p, Sigma_p, Vp = pending_moments(gp, Xp)
    Lp = np.linalg.cholesky(Sigma_p)
    Ks = gp.cov(gp.X, Xs)
    V = sl.solve_triangular(gp.L, Ks, lower=True)
    mu = gp.beta + Ks.T @ gp.alpha
    s2f = math.exp(2.0 * gp.logsig)
    var0 = np.maximum(s2f - np.einsum("nr,nr->r", V, V), 0.0)
    Cx = gp.cov(Xs, Xp) - V.T @ Vp                                   # (R, p)
    B = sl.solve_triangular(Lp, Cx.T, lower=True).T                  # row r = b(x_r)
    if not condition:
        B = np.zeros_like(B)
    var = np.maximum(var0 - np.einsum("rp,rp->r", B, B), 0.0)
    Z = np.asarray(Z, float)
    Yf = mu_p[None, :] + Z @ Lp.T
    each = np.array([acq(name, with_tau(name, params, tau), mu + B @ z, var) for z, tau in zip(Z, _taus(name, params, Yf, raise_tau))])
    score = average(name, each) if log_of_mean or name != "LogEI" else each.mean(axis=0)
    return dict(score=score, mu=mu, var=var, each=each, mu_p=mu_p, Sigma_p=Sigma_p, asum=float(np.abs(gp.alpha).sum()), B=B, Yf=Yf)


def value_bound(ref, s2f, asum):
    """test_batch_gpu.compare's bound on values and means: 1e-6 relative + 64 eps s_f^2 sum|alpha| + 1e-12."""
    return 1e-6 * np.abs(ref) + 64 * EPS * s2f * asum + 1e-12


def top_two_gap(score):
    """(index, relative gap to the runner-up) of the arg-max under (value desc, index asc); NaN / -Inf never win."""
    s = np.where(np.isnan(score), -np.inf, score)
    i = int(np.argmax(s))
    if not s[i] > -np.inf:
        return -1, math.inf
    rest = np.delete(s, i)
    second = rest.max() if rest.size else -np.inf
    return i, float((s[i] - second) / max(abs(s[i]), 1e-300)) if second > -np.inf else math.inf
