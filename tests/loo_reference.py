"""NumPy twin of leave-one-out cross-validation (include/bohip_loo.h).  No device.  A helper, not a test module.

Two forms of the same quantities, for every kernel id (tests/matern_reference.py supplies the families):

    fast    kappa = diag(cK^-1):  mu_-i = y_i - alpha_i / kappa_i,  var_-i = 1 / kappa_i,
            logp_i = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi                      (Rasmussen & Williams 5.4.2)
    brute   N refits with one row deleted, each predicting the NOISY observation it left out

and the gradient of total = sum_i logp_i:  sum_ab D_ab G_ab with G = 1/2 (b alpha' + alpha b') - cK^-1 diag(c) cK^-1,
q = alpha / kappa, b = cK^-1 q, c = 1/2 (1 / kappa + alpha^2 / kappa^2), D = d cK / d theta; d / d beta = sum_i b_i.
"""
import math

import numpy as np
import scipy.linalg as sl

from matern_reference import MaternGP, fx_of_r, is_iso, k_of_r

LOG2PI = math.log(2.0 * math.pi)


def loo_fast(kern, X, y, loglen, logsig, lognoise, beta):
    """(mu, var, logp, total) from kappa = diag(cK^-1)."""
    g = MaternGP(kern, X, y, loglen, logsig, lognoise, beta)
    kappa = np.diag(sl.cho_solve((g.L, True), np.eye(g.N)))
    mu, var = g.y - g.alpha / kappa, 1.0 / kappa
    logp = 0.5 * np.log(kappa) - 0.5 * g.alpha ** 2 / kappa - 0.5 * LOG2PI
    return mu, var, logp, float(logp.sum())


def loo_brute(kern, X, y, loglen, logsig, lognoise, beta):
    """The same by N delete-one refits; one observation alone is predicted from the prior."""
    X, y = np.asarray(X, float), np.asarray(y, float)
    N = len(y)
    mu, var = np.empty(N), np.empty(N)
    for i in range(N):
        keep = np.arange(N) != i
        if N == 1:
            mu[i], var[i] = beta, math.exp(2.0 * logsig)
        else:
            g = MaternGP(kern, X[keep], y[keep], loglen, logsig, lognoise, beta)
            m, v = g.predict(X[i:i + 1])
            mu[i], var[i] = m[0], v[0]
    var = var + MaternGP(kern, X[:1], y[:1], loglen, logsig, lognoise, beta).noise     # the left-out y_i carries its noise
    logp = -0.5 * np.log(var) - 0.5 * (y - mu) ** 2 / var - 0.5 * LOG2PI
    return mu, var, logp, float(logp.sum())


def loo_grad(kern, X, y, loglen, logsig, lognoise, beta):
    """(total, d/dlogNoise, d/dbeta, d/d[ll..., lsigma]) in the slots of MaternGP.mll_grad."""
    g = MaternGP(kern, X, y, loglen, logsig, lognoise, beta)
    Kinv = sl.cho_solve((g.L, True), np.eye(g.N))
    kappa = np.diag(Kinv)
    q = g.alpha / kappa
    b = Kinv @ q
    c = 0.5 * (1.0 / kappa + g.alpha ** 2 / kappa ** 2)
    G = 0.5 * (np.outer(b, g.alpha) + np.outer(g.alpha, b)) - (Kinv * c) @ Kinv
    diff = g.X[:, None, :] - g.X[None, :, :]
    D2 = diff * diff
    r = D2 @ g.il2
    K = k_of_r(g.fam, r, g.s2f)
    ft = -fx_of_r(g.fam, r, g.s2f)
    dll = np.einsum("ij,ijk->k", G * ft, D2 * g.il2)
    dkern = np.concatenate([[dll.sum()] if is_iso(kern) else dll, [np.sum(G * 2.0 * K)]])
    dnoise = np.trace(G) * 2.0 * math.exp(2.0 * g.lognoise)
    total = float(np.sum(0.5 * np.log(kappa) - 0.5 * g.alpha ** 2 / kappa - 0.5 * LOG2PI))
    return total, float(dnoise), float(b.sum()), dkern


def theta_of(kern, d, loglen, logsig, lognoise, beta):
    """[logNoise, mean, ll..., lsigma] with one length entry for an iso kernel."""
    ll = np.atleast_1d(np.asarray(loglen, float))
    ll = ll[:1] if is_iso(kern) else np.broadcast_to(ll, (d,))
    return np.concatenate([[lognoise, beta], ll, [logsig]])


def total_at(kern, X, y, t):
    return loo_fast(kern, X, y, t[2:-1], t[-1], t[0], t[1])[3]


def grad_vec(kern, X, y, t):
    tot, dn, dm, dk = loo_grad(kern, X, y, t[2:-1], t[-1], t[0], t[1])
    return tot, np.concatenate([[dn, dm], np.ravel(dk)])


def central_differences(kern, X, y, t, h=1e-5):
    t = np.asarray(t, float)
    out = np.empty(t.size)
    for k in range(t.size):
        e = np.zeros(t.size)
        e[k] = h
        out[k] = (total_at(kern, X, y, t + e) - total_at(kern, X, y, t - e)) / (2.0 * h)
    return out

