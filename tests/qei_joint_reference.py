"""The NumPy twin of the joint q-EI of a batch and its gradient (include/bohip_qei_joint.h) -- TEST INFRASTRUCTURE ONLY.
No device.  The header's statements, run at float64 or np.longdouble (nei_reference's factor and substitutions, pend_grad_reference's
kernels), and the table of cases of tests/test_qei_joint_gpu.py.

WORST_VALUE / WORST_GRAD: the largest |float64 twin - extended twin| over every case (tests/test_qei_joint_host.py recomputes them and
asserts the stored constants within 2 x), rounded up to two digits; the value in units of s_f, the gradient in units of s_f / l.  The
device is held to DEVICE_FACTOR = 16 x these, the project's rule for its gradient routes.
"""
import math

import numpy as np

import nei_reference as nr
import pend_reference as pr
import test_pend_gpu as tp
from conftest import synth
from pend_grad_reference import cov_fx

DEVICE_FACTOR = 16.0
WORST_VALUE = 6.9e-14   # measured: 6.84e-14
WORST_GRAD = 2.1e-13    # measured: 2.05e-13
JITTER_REL = 1e-6   # of the cases: q = 16 points a length-scale apart leave Sigma with eigenvalues far below one ulp of s_f^2
MARGIN = 1e-9       # every sample's gap between best and second best, and |f_s,j* - tau|, in the extended twin

# name: (kernel, N, d, q, B, S, seed).  q = 1, 2, 5, 16; N = 129 (one row past a tile) and 1030 (past the small-model routes);
# B q = q, 135 = 27 x 5 and 144 = 9 x 16 (past one 128-row tile, no multiple of it); S = 1, 70, 1024; d = 3 and 20 (bucket 32); the SE,
# Matern 5/2 and Matern 1/2 (the LOW family whose dk/dx is 0 at r = 0) kernels.  The data of a (kernel, N, d) is shared (one fit).
CASES = {
    "se-n129-q1-B1-S1": ("SEArd", 129, 3, 1, 1, 1, 0),
    "se-n129-q2-B1-S70": ("SEArd", 129, 3, 2, 1, 70, 1),
    "se-n129-q5-B27-S70": ("SEArd", 129, 3, 5, 27, 70, 2),
    "se-n129-q16-B9-S1024": ("SEArd", 129, 3, 16, 9, 1024, 3),
    "se-n129-d20-q5-B27-S70": ("SEArd", 129, 20, 5, 27, 70, 4),
    "m52-n129-q5-B1-S1024": ("Mat52Ard", 129, 3, 5, 1, 1024, 5),
    "m52-n129-q16-B1-S70": ("Mat52Ard", 129, 3, 16, 1, 70, 6),
    "m52-n1030-q5-B27-S70": ("Mat52Ard", 1030, 3, 5, 27, 70, 7),
    "m52-n1030-q1-B1-S1024": ("Mat52Ard", 1030, 3, 1, 1, 1024, 14),   # (seed 8: no sample above tau)
    "m12-n129-q2-B1-S1": ("Mat12Iso", 129, 3, 2, 1, 1, 9),
    "m12-n129-q5-B27-S1024": ("Mat12Iso", 129, 3, 5, 27, 1024, 10),
    "m12-n129-d20-q16-B9-S70": ("Mat12Iso", 129, 20, 16, 9, 70, 11),
    "m12-n1030-q16-B9-S70": ("Mat12Iso", 1030, 3, 16, 9, 70, 12),
}


def normals(seed, S):
    """Z [S][16] as the library draws it: bohip_thompson_normal(seed, s, i) (host code: no GPU needed)."""
    from bohip import _lib

    lib = _lib.load()
    return np.array([[lib.bohip_thompson_normal(seed, s, i) for i in range(16)] for s in range(S)])


def inputs(case):
    """(kern, X, y, Xs [B q, d], q, S, seed, tau): the data of the case's (kernel, N, d), its own points in the unit box."""
    kern, N, d, q, B, S, seed = CASES[case]
    X, y, _ = synth(N, d, 1, 0)
    Xs = np.random.default_rng(500 + seed).random((B * q, d))
    return kern, X, y, Xs, q, S, 77 + seed, float(np.median(y))


class Twin:
    """One fit at the precision dt (test_pend_gpu's recipe) and the header's statements per group."""

    def __init__(self, kern, X, y, dt=np.float64):
        self.kern, self.dt = kern, dt
        self.X, y = np.asarray(X, dtype=dt), np.asarray(y, dtype=dt)
        self.il = np.exp(-dt(tp.LL)) * np.ones(self.X.shape[1], dtype=dt)
        self.s2f, self.beta = np.exp(dt(2.0) * dt(tp.LSIG)), dt(tp.BETA)
        nu = np.exp(dt(2.0) * dt(tp.LNOISE)) + dt(pr.NOISE_EPS)
        self.L = nr.chol(self.cov(self.X, self.X)[0] + nu * np.eye(len(y), dtype=dt))
        self.alpha = nr.solve_lower_t(self.L, nr.solve_lower(self.L, y - self.beta))

    def cov(self, A, B):
        return cov_fx(self.kern, A, B, self.il, self.s2f, self.dt)

    def posterior(self, Xs):
        """mu [R], V [N, R], Ks: the noise-free posterior pieces at the rows of Xs."""
        Ks = self.cov(self.X, Xs)[0]
        return self.beta + Ks.T @ self.alpha, nr.solve_lower(self.L, Ks)

    def group(self, Xg, mu, V, Z, tau, jitter_rel, want_grad=True):
        """(value, grad [q, d], pivot, margin) of one group; margin: the smallest gap best - second best and |f_s,j* - tau|."""
        dt, q = self.dt, len(Xg)
        A = self.cov(Xg, Xg)[0] - V.T @ V + dt(jitter_rel) * self.s2f * np.eye(q, dtype=dt)
        for k in range(q):                                        # right-looking, the update written c_j (c_i / d)
            d = A[k, k]
            if not (d > 0 and np.isfinite(d)):
                return -math.inf, np.zeros(Xg.shape), k + 1, math.inf
            for i in range(k + 1, q):
                A[i:, i] = A[i:, i] - A[i:, k] * (A[i, k] / d)
        L = np.tril(A) / np.sqrt(np.diag(A))[None, :]
        Zq = np.asarray(Z[:, :q], dtype=dt)
        F = mu[None, :] + Zq @ L.T                                # (S, q)
        js = np.argmax(F, axis=1)                                 # (the first maximum)
        best = F[np.arange(len(F)), js]
        hit = best > dt(tau)
        S = len(F)
        value = np.where(hit, best - dt(tau), dt(0)).sum() / dt(S)
        second = np.sort(F, axis=1)[:, -2] if q > 1 else np.full(S, -np.inf)
        margin = float(min(np.min(best - second), np.min(np.abs(best - dt(tau)))))
        if not want_grad:
            return value, None, 0, margin
        g = hit / dt(S)
        onehot = (js[:, None] == np.arange(q)[None, :]) * g[:, None]           # (S, q)
        mubar = onehot.sum(axis=0)
        Lbar = np.tril(onehot.T @ Zq)
        P = np.tril(L.T @ Lbar)
        P[np.diag_indices(q)] = P[np.diag_indices(q)] / dt(2)
        Li = nr.solve_lower(L, np.eye(q, dtype=dt))
        M = Li.T @ P @ Li
        Sbar = (M + M.T) / dt(2)
        U = nr.solve_lower_t(self.L, V)                                          # (N, q): column i = u_i
        E = mubar[:, None] * self.alpha[None, :] - dt(2) * Sbar @ U.T            # (q, N)
        il2 = self.il * self.il
        off = Sbar * (1 - np.eye(q, dtype=dt))
        grad = (np.einsum("jn,jnk->jk", self.cov(Xg, self.X)[1] * E, Xg[:, None, :] - self.X[None, :, :])
                + dt(2) * np.einsum("ji,jik->jk", self.cov(Xg, Xg)[1] * off, Xg[:, None, :] - Xg[None, :, :])) * il2
        return value, grad, 0, margin

    def qei(self, Xs, q, Z, tau, jitter_rel=JITTER_REL, want_grad=True):
        """(value [B], grad [B q, d] or None, pivot [B], margin) of the groups of q rows of Xs."""
        Xs = np.asarray(Xs, dtype=self.dt)
        mu, V = self.posterior(Xs)
        out = [self.group(Xs[r:r + q], mu[r:r + q], V[:, r:r + q], Z, tau, jitter_rel, want_grad) for r in range(0, len(Xs), q)]
        return (np.array([o[0] for o in out], dtype=self.dt), np.concatenate([o[1] for o in out]) if want_grad else None,
                np.array([o[2] for o in out]), min(o[3] for o in out))


_REF = {}


def reference(case, dt=np.float64):
    """dict(value [B], grad [B q, d], margin, and the inputs) of one case, computed once and shared; one fit per (kernel, N, d)."""
    if (case, dt) not in _REF:
        kern, X, y, Xs, q, S, seed, tau = inputs(case)
        fit = (kern, X.shape, dt)
        if fit not in _REF:
            _REF[fit] = Twin(kern, X, y, dt)
        value, grad, pivot, margin = _REF[fit].qei(Xs, q, normals(seed, S), tau)
        _REF[case, dt] = dict(value=value, grad=grad, pivot=pivot, margin=margin, kern=kern, X=X, y=y, Xs=Xs, q=q, S=S, seed=seed, tau=tau)
    return _REF[case, dt]


def distances(value, grad, ref):
    """(value distance in s_f, gradient distance in s_f / l): the largest over the case."""
    sf = math.exp(tp.LSIG)
    dv = float(np.max(np.abs(np.asarray(value, dtype=np.float64) - np.asarray(ref["value"], dtype=np.float64)))) / sf
    dg = float(np.max(np.abs(np.asarray(grad, dtype=np.float64) - np.asarray(ref["grad"], dtype=np.float64)))) / (sf * math.exp(-tp.LL))
    return dv, dg
