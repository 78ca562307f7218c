"""NumPy / SciPy model of the GP for every kernel id of include/bohip.h (SE and Matérn 1/2, 3/2, 5/2, ARD and iso).

A helper of the Matérn tests, not a test module.  It restates what the library computes, independently of the oracle
(whose `np_cov` knows SE and Matérn 5/2 only):

    r = sum_k (x_k - y_k)^2 exp(-2 ll_k),  rho = sqrt(r),  s_f^2 = exp(2 lsigma)
    cK = K + (exp(2 logNoise) + NOISE_EPS) I,  L = chol(cK)  (LAPACK),  alpha = cK^-1 (y - beta)
    mu = beta + K*' alpha,  sigma^2 = max(s_f^2 - |L^-1 k*|^2, 0)

Derivatives use fx = 2 dk/dr: dk(x*, x_j)/dx*_k = fx (x*_k - x_jk) il2_k and dk/dll_k = -fx (x_k - y_k)^2 il2_k.  Matérn 1/2
has fx = -s_f^2 exp(-rho) / rho, and 0 at rho = 0: the minimum-norm subgradient of rho where a point meets an observation.
"""
import math

import numpy as np
import scipy.linalg as sl
from scipy.special import erf

from oracle.oracle import NOISE_EPS

# name -> (family, iso)
KERNELS = {"SEArd": ("SE", False), "SEIso": ("SE", True), "Mat52Ard": ("M52", False), "Mat32Ard": ("M32", False),
           "Mat12Ard": ("M12", False), "Mat52Iso": ("M52", True), "Mat32Iso": ("M32", True), "Mat12Iso": ("M12", True)}
NEW_KERNELS = ["Mat32Ard", "Mat12Ard", "Mat52Iso", "Mat32Iso", "Mat12Iso"]


def family(kern):
    return KERNELS[kern][0]


def is_iso(kern):
    return KERNELS[kern][1]


def il2_of(kern, loglen, d):
    ll = np.atleast_1d(np.asarray(loglen, dtype=np.float64))
    if is_iso(kern):
        ll = np.full(d, ll[0])
    return np.exp(-2.0 * np.broadcast_to(ll, (d,)))


def k_of_r(fam, r, s2f):
    rho = np.sqrt(r)
    if fam == "SE":
        return s2f * np.exp(-0.5 * r)
    if fam == "M12":
        return s2f * np.exp(-rho)
    if fam == "M32":
        s = math.sqrt(3.0) * rho
        return s2f * (1.0 + s) * np.exp(-s)
    s = math.sqrt(5.0) * rho
    return s2f * (1.0 + s + 5.0 / 3.0 * r) * np.exp(-s)


def fx_of_r(fam, r, s2f):
    """2 dk/dr (Matérn 1/2: 0 at r = 0)."""
    r = np.asarray(r, dtype=np.float64)
    rho = np.sqrt(r)
    if fam == "SE":
        return -s2f * np.exp(-0.5 * r)
    if fam == "M12":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(rho > 0.0, -s2f * np.exp(-rho) / np.where(rho > 0.0, rho, 1.0), 0.0)
    if fam == "M32":
        return -3.0 * s2f * np.exp(-math.sqrt(3.0) * rho)
    s = math.sqrt(5.0) * rho
    return -(5.0 / 3.0) * s2f * (1.0 + s) * np.exp(-s)


def cov(kern, X, Y, loglen, logsig):
    """k(X_i, Y_j) for row-observation arrays X (n, d), Y (m, d)."""
    il2 = il2_of(kern, loglen, X.shape[1])
    diff = X[:, None, :] - Y[None, :, :]
    r = np.einsum("nmk,k->nm", diff * diff, il2)
    return k_of_r(family(kern), r, math.exp(2.0 * logsig))


def acq_value(name, params, mu, s2):
    """The functors of the reference's src/acquisitionfunctions.jl, vectorised."""
    mu, s2 = np.asarray(mu, float), np.asarray(s2, float)
    if name in ("EI", "PI"):
        tau = params[0]
        D = mu - tau
        s = np.sqrt(np.where(s2 > 0, s2, 1.0))
        cdf = 0.5 * (1.0 + erf(D / np.sqrt(2.0 * np.where(s2 > 0, s2, 1.0))))
        pdf = np.exp(-D ** 2 / (2 * np.where(s2 > 0, s2, 1.0))) / np.sqrt(2 * math.pi * np.where(s2 > 0, s2, 1.0))
        if name == "EI":
            return np.where(s2 > 0, D * cdf + s * pdf, np.maximum(D, 0.0))
        return np.where(s2 > 0, cdf, (mu > tau).astype(float))
    if name == "UCB":
        return mu + params[0] * np.sqrt(s2)
    if name == "MI":
        return mu + params[0] * (np.sqrt(s2 + params[1]) - math.sqrt(params[1]))
    if name == "MaxMean":
        return mu.copy()
    raise KeyError(name)


def acq_partials(name, params, mu, s2):
    """(d acq / d mu, d acq / d sigma^2) of acq_value, with the library's values at sigma^2 = 0."""
    if name in ("EI", "PI"):
        if s2 == 0.0:
            return (1.0 if (name == "EI" and mu > params[0]) else 0.0), 0.0
        D = mu - params[0]
        s = math.sqrt(s2)
        z = D / s
        phi = math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
        if name == "EI":   # acq = D Phi(z) + phi(z): the reference's sqrt(s2) * normal_pdf(D, s2)
            return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0))) + (D - z) * phi / s, (D - z) * phi * (-z / (2.0 * s2))
        return phi / s, phi * (-z / (2.0 * s2))
    if name == "UCB":
        return 1.0, (params[0] / (2.0 * math.sqrt(s2)) if s2 > 0 else 0.0)
    if name == "MI":
        return 1.0, params[0] / (2.0 * math.sqrt(s2 + params[1]))
    return 1.0, 0.0


def first_argmax(scores):
    """Strict '>' from -Inf, first maximum wins (reference src/acquisition.jl:55-66)."""
    best, idx = -math.inf, -1
    for i, v in enumerate(scores):
        if v > best:
            best, idx = v, i
    return best, idx


class MaternGP:
    """The model of one bohip handle: observations X (N, d) row-major, y (N,)."""

    def __init__(self, kern, X, y, loglen, logsig, lognoise, beta):
        self.kern, self.fam = kern, family(kern)
        self.X, self.y = np.array(X, dtype=np.float64), np.array(y, dtype=np.float64)
        self.N, self.d = self.X.shape
        self.loglen = np.atleast_1d(np.asarray(loglen, dtype=np.float64)).copy()
        self.logsig, self.lognoise, self.beta = float(logsig), float(lognoise), float(beta)
        self.s2f = math.exp(2.0 * self.logsig)
        self.il2 = il2_of(kern, self.loglen, self.d)
        self.noise = math.exp(2.0 * self.lognoise) + NOISE_EPS
        self.cK = cov(kern, self.X, self.X, self.loglen, self.logsig) + self.noise * np.eye(self.N)
        self.L = np.linalg.cholesky(self.cK)
        self.alpha = sl.cho_solve((self.L, True), self.y - self.beta)

    # -- posterior ----------------------------------------------------------------------------------------
    def kstar(self, Xs):
        return cov(self.kern, self.X, np.atleast_2d(Xs), self.loglen, self.logsig)   # (N, R)

    def predict(self, Xs):
        Ks = self.kstar(Xs)
        V = sl.solve_triangular(self.L, Ks, lower=True)
        return self.beta + Ks.T @ self.alpha, np.maximum(self.s2f - np.sum(V * V, axis=0), 0.0)

    def predict_cov(self, Xs):
        Xs = np.atleast_2d(Xs)
        Ks = self.kstar(Xs)
        V = sl.solve_triangular(self.L, Ks, lower=True)
        return self.beta + Ks.T @ self.alpha, cov(self.kern, Xs, Xs, self.loglen, self.logsig) - V.T @ V

    def score(self, acq, params, Xs):
        mu, s2 = self.predict(Xs)
        return acq_value(acq, params, mu, s2)

    def posterior_grad(self, x):
        """(mu, sigma^2, d mu/dx, d sigma^2/dx) at one point x (d,)."""
        x = np.asarray(x, dtype=np.float64)
        diff = x[None, :] - self.X                                        # (N, d)
        r = (diff * diff) @ self.il2
        ks = k_of_r(self.fam, r, self.s2f)
        dk = fx_of_r(self.fam, r, self.s2f)[:, None] * diff * self.il2    # d k*_j / dx  (N, d)
        v = sl.solve_triangular(self.L, ks, lower=True)
        u = sl.solve_triangular(self.L, v, lower=True, trans="T")         # cK^-1 k*
        s2 = self.s2f - v @ v
        return self.beta + ks @ self.alpha, max(s2, 0.0), dk.T @ self.alpha, (-2.0 * (dk.T @ u) if s2 > 0 else np.zeros(self.d))

    def score_grad(self, acq, params, Xs):
        """Scores and d score / dx for the columns of Xs (R, d) -> (R,), (R, d)."""
        Xs = np.atleast_2d(Xs)
        sc, g = np.empty(len(Xs)), np.empty(Xs.shape)
        for i, x in enumerate(Xs):
            mu, s2, dmu, ds2 = self.posterior_grad(x)
            sc[i] = acq_value(acq, params, np.array([mu]), np.array([s2]))[0]
            a, b = acq_partials(acq, params, mu, s2)
            g[i] = a * dmu + (b * ds2 if s2 > 0 else 0.0)
        return sc, g

    # -- marginal likelihood ----------------------------------------------------------------------------
    def mll(self):
        return float(-0.5 * (self.y - self.beta) @ self.alpha - np.sum(np.log(np.diag(self.L)))
                     - 0.5 * self.N * math.log(2 * math.pi))

    def mll_grad(self):
        """(mll, d/dlogNoise, d/dbeta, d/d[ll..., lsigma]) in GaussianProcesses.get_params order."""
        Kinv = sl.cho_solve((self.L, True), np.eye(self.N))
        G = 0.5 * (np.outer(self.alpha, self.alpha) - Kinv)
        diff = self.X[:, None, :] - self.X[None, :, :]
        D2 = diff * diff                                                   # (N, N, d)
        r = D2 @ self.il2
        K = k_of_r(self.fam, r, self.s2f)
        ft = -fx_of_r(self.fam, r, self.s2f)                               # 2 dk/d(-r)
        dll = np.einsum("ij,ijk->k", G * ft, D2 * self.il2)
        dkern = np.concatenate([[dll.sum()] if is_iso(self.kern) else dll, [np.sum(G * 2.0 * K)]])
        dnoise = np.trace(G) * 2.0 * math.exp(2.0 * self.lognoise)
        return self.mll(), float(dnoise), float(np.sum(self.alpha)), dkern


def mll_of(kern, X, y, loglen, logsig, lognoise, beta):
    return MaternGP(kern, X, y, loglen, logsig, lognoise, beta).mll()
