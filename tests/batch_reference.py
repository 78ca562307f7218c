"""CPU references for greedy batch selection (bohip_gp_select_batch) -- TEST INFRASTRUCTURE ONLY.

Two independent statements of "q picks, each conditioned on the fantasised observations of the earlier ones":

  * ``refit_per_pick``  the definition: append (x_s, y_f) to the data, refit the whole model, score again;
  * ``recurrence``      what the library computes: rank-one updates of (mu, sigma^2) over the candidate set from one
                        V = L^-1 K*, the model untouched.

Models: ``oracle.NumpyGP`` (SEArd, Mat52Ard) or ``matern_reference.MaternGP`` (every kernel), wrapped by ``gp_factory``.
The arg-max is the project's rule: value descending, index ascending, NaN / -Inf never win, earlier picks excluded.
"""
import math

import numpy as np
import scipy.linalg as sl

from matern_reference import MaternGP, acq_value, cov as matern_cov
from oracle.oracle import NOISE_EPS, NumpyGP


class _Fitted:
    """mu, var at candidates + what the recurrence needs (L, alpha, kernel), for one data set."""

    def __init__(self, kern, X, y, loglen, logsig, lognoise, beta):
        self.kern, self.loglen, self.logsig, self.lognoise, self.beta = kern, loglen, logsig, lognoise, beta
        if kern in ("SEArd", "Mat52Ard"):
            gp = NumpyGP(X.shape[1], loglen, logsig, lognoise, beta, kern=kern).fit(X, y)
            self.predict = gp.predict_f
        else:
            gp = MaternGP(kern, X, y, loglen, logsig, lognoise, beta)
            self.predict = gp.predict
        self.X, self.L, self.alpha = np.asarray(X, float), gp.L, gp.alpha

    def cov(self, A, B):
        return matern_cov(self.kern, np.atleast_2d(A), np.atleast_2d(B), self.loglen, self.logsig)


def gp_factory(kern, loglen, logsig, lognoise, beta):
    return lambda X, y: _Fitted(kern, X, y, loglen, logsig, lognoise, beta)


def masked_argmax(score, picked):
    """(index, value, relative gap to the runner-up) under (value desc, index asc); -1 when nothing can win."""
    s = np.where(np.isnan(score) | picked, -np.inf, score)
    i = int(np.argmax(s))                      # first maximum
    if not s[i] > -np.inf:
        return -1, -math.inf, math.inf
    rest = np.delete(s, i)
    second = rest.max() if rest.size else -np.inf
    gap = (s[i] - second) / max(abs(s[i]), 1e-300) if second > -np.inf else math.inf
    return i, float(s[i]), float(gap)


def _fantasy_value(fantasy, mu_s):
    return mu_s if fantasy == "believer" else float(fantasy)


def _params_with_tau(acq, params, tau):
    return [tau] + list(params[1:]) if acq in ("EI", "PI") else list(params)


def refit_per_pick(factory, X, y, Xs, acq, params, q, fantasy="believer", raise_tau=False):
    """Rows (idx, val, mu, var, gap, sum|alpha|) of the q picks; X (N, d), Xs (R, d); fantasy 'believer' or a number."""
    X, y = np.array(X, float), np.array(y, float)
    picked = np.zeros(len(Xs), bool)
    tau = params[0] if acq in ("EI", "PI") else None
    out = []
    for _ in range(q):
        gp = factory(X, y)
        mu, var = gp.predict(Xs)
        sc = acq_value(acq, _params_with_tau(acq, params, tau), mu, np.maximum(var, 0.0))
        i, v, gap = masked_argmax(sc, picked)
        if i < 0:
            out.append((-1, -math.inf, math.nan, math.nan, math.inf, float(np.abs(gp.alpha).sum())))
            continue
        out.append((i, v, float(mu[i]), float(var[i]), gap, float(np.abs(gp.alpha).sum())))
        picked[i] = True
        yf = _fantasy_value(fantasy, float(mu[i]))
        if raise_tau and tau is not None:
            tau = max(tau, yf)
        X = np.vstack([X, Xs[i]])
        y = np.append(y, yf)
    return out


def recurrence(factory, X, y, Xs, acq, params, q, fantasy="believer", raise_tau=False):
    """The same picks from ONE fit: c_r = k(x_r, x_s) - v_r.v_s - sum_i u_i[r] u_i[s];  S = c_s + noise;
    mu_r += c_r (y_f - mu_s) / S;  u_j[r] = c_r / sqrt(S);  sigma^2_r -= u_j[r]^2."""
    gp = factory(np.asarray(X, float), np.asarray(y, float))
    Ks = gp.cov(gp.X, Xs)                                   # (N, R)
    V = sl.solve_triangular(gp.L, Ks, lower=True)           # column r = v_r
    mu = gp.beta + Ks.T @ gp.alpha
    var = math.exp(2.0 * gp.logsig) - np.einsum("nr,nr->r", V, V)
    noise = math.exp(2.0 * gp.lognoise) + NOISE_EPS
    picked = np.zeros(len(Xs), bool)
    tau = params[0] if acq in ("EI", "PI") else None
    U = np.zeros((0, len(Xs)))
    out = []
    for _ in range(q):
        sc = acq_value(acq, _params_with_tau(acq, params, tau), mu, np.maximum(var, 0.0))
        s, v, gap = masked_argmax(sc, picked)
        if s < 0:
            out.append((-1, -math.inf, math.nan, math.nan, math.inf, 0.0))
            continue
        out.append((s, v, float(mu[s]), float(max(var[s], 0.0)), gap, float(np.abs(gp.alpha).sum())))
        picked[s] = True
        c = gp.cov(Xs, Xs[s])[:, 0] - V.T @ V[:, s] - U.T @ U[:, s]
        S = c[s] + noise
        yf = _fantasy_value(fantasy, float(mu[s]))
        mu = mu + c * (yf - mu[s]) / S
        u = c / math.sqrt(S)
        var = var - u * u
        U = np.vstack([U, u])
        if raise_tau and tau is not None:
            tau = max(tau, yf)
    return out
