"""NumPy twin of the posterior sample paths (bohip_paths, include/bohip_paths.h), a helper of the path tests, not a test module.

    f_s(x) = beta + sum_m w_sm phi_m(x) + sum_j u_sj k(x, X_j),   u_s = K^-1 (y - beta - Phi(X) w_s - eps_s)
    phi_2m = sqrt(s2f / F) cos(omega_m . x),  phi_2m+1 = sqrt(s2f / F) sin(omega_m . x)

Everything random is rebuilt from the documented keys of bohip_thompson_normal(seed, stream, counter):
    z_mk = (seed, -1 - m, k), the n normals of chi2_m = (seed, -1 - m, d + i);  w_sm = (seed, s, m);  eps_si = sqrt(n) (seed, s, M + i)
K and k* come from matern_reference (every kernel id); solves are LAPACK's.
"""
import math

import numpy as np
import scipy.linalg as sl

import matern_reference as mr
from oracle.oracle import NOISE_EPS

EPS = np.finfo(np.float64).eps
DOF = {"SE": 0, "M12": 1, "M32": 3, "M52": 5}


def normal(seed, s, j):
    """z(seed, s, j): the NumPy twin of bohip_thompson_normal for a scalar stream s (negative allowed) and an int64 array j."""
    M = np.uint64

    def sm(x):
        x = x + M(0x9E3779B97F4A7C15)
        x = (x ^ (x >> M(30))) * M(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> M(27))) * M(0x94D049BB133111EB)
        return x ^ (x >> M(31))

    j = np.asarray(j, dtype=np.int64)
    with np.errstate(over="ignore"):
        key = np.full(j.shape, s, dtype=np.int64).astype(np.uint64) * M(0xD1B54A32D192ED03) + j.astype(np.uint64)
        h = sm(np.full(j.shape, seed, dtype=np.uint64) ^ sm(key))
        h2 = sm(h)
    u1 = ((h >> M(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)
    u2 = (h2 >> M(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def frequencies(kern, loglen, d, F, seed):
    """Omega (F x d): omega_mk = z_mk exp(-loglen_k) t_m."""
    ll = np.atleast_1d(np.asarray(loglen, dtype=np.float64))
    ll = np.full(d, ll[0]) if mr.is_iso(kern) else np.broadcast_to(ll, (d,))
    n = DOF[mr.family(kern)]
    Om = np.empty((F, d))
    for m in range(F):
        z = normal(seed, -1 - m, np.arange(d + n))
        t = 1.0
        if n:
            chi2 = 0.0
            for i in range(n):
                chi2 += z[d + i] * z[d + i]
            t = 1.0 / math.sqrt(chi2 / n)
        Om[m] = z[:d] * np.exp(-ll) * t
    return Om


def normal_tol(z):
    """What two correct implementations of z = sqrt(-2 log u1) cos(2 pi u2) may differ by: a few ulp of log, sqrt and cos on |z|, plus
    the rounding of the cosine's argument (<= 2 pi eps) times the radius (<= sqrt(-2 log 2^-53) < 8.6): 8 eps (|z| + 2 pi 8.6)."""
    return 8.0 * EPS * (np.abs(z) + 2.0 * math.pi * 8.6)


def frequencies_tol(kern, loglen, d, F, seed):
    """Elementwise bound on |Omega_device - Omega_twin| (F x d): the normals' own tolerance carried through
    omega = z exp(-ll) t, t = (chi2 / n)^-1/2 (d t / t = -1/2 d chi2 / chi2, d chi2 = 2 sum |z_i| dz_i), plus 8 eps for exp, sqrt
    and the products."""
    ll = np.atleast_1d(np.asarray(loglen, dtype=np.float64))
    ll = np.full(d, ll[0]) if mr.is_iso(kern) else np.broadcast_to(ll, (d,))
    n = DOF[mr.family(kern)]
    tol = np.empty((F, d))
    for m in range(F):
        z = normal(seed, -1 - m, np.arange(d + n))
        t, rel_t = 1.0, 0.0
        if n:
            chi2 = float(np.sum(z[d:] ** 2))
            t = 1.0 / math.sqrt(chi2 / n)
            rel_t = float(np.sum(np.abs(z[d:]) * normal_tol(z[d:]))) / chi2
        om = z[:d] * np.exp(-ll) * t
        tol[m] = np.exp(-ll) * t * normal_tol(z[:d]) + np.abs(om) * (rel_t + 8.0 * EPS)
    return tol


def features(Om, X, s2f):
    """Phi (n x 2F), columns interleaved cos, sin."""
    P = X @ Om.T
    F = Om.shape[0]
    out = np.empty((X.shape[0], 2 * F))
    out[:, 0::2] = np.cos(P)
    out[:, 1::2] = np.sin(P)
    return math.sqrt(s2f / F) * out


def weights(seed, s, M):
    return normal(seed, s, np.arange(M))


def noise_normals(seed, s, M, N):
    return normal(seed, s, M + np.arange(N))


class PathTwin:
    """The paths of one model.  diag = what the model adds to K's diagonal (exp(2 logNoise) + NOISE_EPS)."""

    def __init__(self, kern, X, y, loglen, logsig, lognoise, beta, M, seed):
        self.kern, self.X, self.y, self.ll, self.ls, self.beta, self.M, self.seed = kern, X, y, loglen, logsig, beta, M, seed
        self.N, self.d = X.shape
        self.s2f = math.exp(2.0 * logsig)
        self.diag = math.exp(2.0 * lognoise) + NOISE_EPS
        self.Om = frequencies(kern, loglen, self.d, M // 2, seed)
        self.K = mr.cov(kern, X, X, loglen, logsig) + self.diag * np.eye(self.N)
        self.PhiX = features(self.Om, X, self.s2f)

    def w(self, s):
        return weights(self.seed, s, self.M)

    def eps(self, s):
        return math.sqrt(self.diag) * noise_normals(self.seed, s, self.M, self.N)

    def rhs(self, s):
        return (self.y - self.beta) - self.PhiX @ self.w(s) - self.eps(s)

    def u(self, s):
        return sl.cho_solve(sl.cho_factor(self.K, lower=True), self.rhs(s))

    def terms(self, xs, u, w):
        """(kernel terms R x N, feature terms R x M) of the sum f - beta at the rows of xs."""
        ks = mr.cov(self.kern, xs, self.X, self.ll, self.ls)
        return ks * u[None, :], features(self.Om, xs, self.s2f) * w[None, :]

    def value(self, xs, u, w):
        a, b = self.terms(xs, u, w)
        return self.beta + a.sum(1) + b.sum(1)

    def value_bound(self, xs, u, w, c=8):
        """(N + M + c) eps (sum |u_j k_j| + sum |w_m phi_m|) for the sum in any order, plus d eps |omega_m . x| per feature for the
        rounding of the cosine's argument (|d/dp cos p| <= 1), doubled: the twin's own evaluation carries the same error."""
        a, b = self.terms(xs, u, w)
        amp = math.sqrt(self.s2f / (self.M // 2))
        arg = np.abs(xs) @ np.abs(self.Om).T                    # >= |omega . x| term by term, R x F
        wpair = np.abs(w[0::2]) + np.abs(w[1::2])
        return 2.0 * ((self.N + self.M + c) * EPS * (np.abs(a).sum(1) + np.abs(b).sum(1)) + self.d * EPS * amp * (arg @ wpair))

    def grad(self, xs, u, w):
        """d f / d x at the rows of xs: R x d."""
        il2 = mr.il2_of(self.kern, self.ll, self.d)
        diff = xs[:, None, :] - self.X[None, :, :]
        r = np.einsum("rnk,k->rn", diff * diff, il2)
        fx = mr.fx_of_r(mr.family(self.kern), r, self.s2f)
        g = np.einsum("rn,rnk->rk", fx * u[None, :], diff) * il2[None, :]
        P = xs @ self.Om.T
        amp = math.sqrt(self.s2f / (self.M // 2))
        q = amp * (-w[None, 0::2] * np.sin(P) + w[None, 1::2] * np.cos(P))
        return g + q @ self.Om

    def grad_bound(self, xs, u, w, c=8):
        """the same bound on the gradient's sums, component by component: R x d"""
        il2 = mr.il2_of(self.kern, self.ll, self.d)
        diff = xs[:, None, :] - self.X[None, :, :]
        r = np.einsum("rnk,k->rn", diff * diff, il2)
        fx = mr.fx_of_r(mr.family(self.kern), r, self.s2f)
        a = np.einsum("rn,rnk->rk", np.abs(fx * u[None, :]), np.abs(diff)) * il2[None, :]
        amp = math.sqrt(self.s2f / (self.M // 2))
        wpair = np.abs(w[0::2]) + np.abs(w[1::2])
        b = amp * (wpair[None, :] * np.ones((xs.shape[0], 1))) @ np.abs(self.Om)
        arg = np.abs(xs) @ np.abs(self.Om).T
        return 2.0 * ((self.N + self.M + c + 4 * self.d) * EPS * (a + b) + self.d * EPS * amp * ((arg * wpair[None, :]) @ np.abs(self.Om)))


def conditional_moments(twin, xs):
    """Given Omega the paths are exactly Gaussian: mean mu(x*), covariance G G' + diag A'A with A = K^-1 k*, G = Phi(x*) - A' Phi(X)."""
    ks = mr.cov(twin.kern, twin.X, xs, twin.ll, twin.ls)               # N x R
    A = sl.cho_solve(sl.cho_factor(twin.K, lower=True), ks)
    mu = twin.beta + A.T @ (twin.y - twin.beta)
    G = features(twin.Om, xs, twin.s2f) - A.T @ twin.PhiX
    return mu, G @ G.T + twin.diag * (A.T @ A)
