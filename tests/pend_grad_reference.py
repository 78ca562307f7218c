"""The NumPy twin of the gradient under pending evaluations (include/bohip_pend_grad.h) -- TEST INFRASTRUCTURE ONLY.
No device.  pend_reference.recurrence's pieces and the header's formula from the same statements at float64 or np.longdouble
(nei_reference's factor and substitutions); the functors and their partials are float64 closed forms.

WORST_GRAD[acq]: the largest |float64 twin - extended twin| gradient component over every input of tests/test_pend_grad_gpu.py
(test_pend_grad_host.py recomputes it and asserts the stored constants within 2 x), rounded up to two digits.  Scale-free as
nei_grad_reference's: in units of s_f / l (PI: 1 / l; LogEI: relative to max(1, |ref|_inf) of the candidate).
The device is held to DEVICE_FACTOR = 16 x these, the factor the NEI gradient uses.
"""
import math

import numpy as np

import nei_reference as nr
import pend_reference as pr
import test_pend_gpu as tp
from conftest import synth
from nei_grad_reference import partials as tau_partials

DEVICE_FACTOR = 16.0
ACQS = ("EI", "PI", "UCB", "MI", "MaxMean", "LogEI")
WORST_GRAD = {"EI": 2.3e-13, "PI": 2.0e-13, "UCB": 2.4e-13, "MI": 1.6e-13, "MaxMean": 1.3e-13, "LogEI": 4.5e-12}
# measured: 2.22e-13, 1.98e-13, 2.32e-13, 1.58e-13, 1.29e-13, 4.46e-12
# BOHIP_PEND_RAISE_TAU in the device comparison: LogEI carries it; EI and PI keep their tau (a raised incumbent, the largest fantasised
# outcome, puts them back at exactly 0 out there).  The host test differentiates all three both ways.
RAISE = {"EI": False, "PI": False, "UCB": True, "MI": True, "MaxMean": True, "LogEI": True}

# test_pend_gpu.CONFIGS' shapes (kernel, N, d, p, stress, S, R, seed), then: d = 20 (dimension bucket 32); nine row tiles with R = 300
# (the tiled finish); S = 63, 64, 65, 128 at N = 129 (k_pend_weights' lane split: 64 lanes, tiles of 128 fantasies at p = 32)
CASES = dict(tp.CONFIGS)
CASES["d20"] = ("SEArd", 129, 20, 5, None, 5, 40, 5)
CASES["n1030-R300"] = ("SEArd", 1030, 3, 8, None, 16, 300, 6)
for _S in (63, 64, 65, 128):
    CASES[f"n129-p32-S{_S}"] = ("Mat52Ard", 129, 3, 32, None, _S, 40, 7)
# EI and PI are exactly 0 at XS_BOX's candidates wherever the conditioned s^2 is small against (tau - mu)^2: there the comparison
# would say nothing.  They are compared at the same candidates moved FAR_SHIFT length-scales out of the data's box along the first
# coordinate with tau = the prior mean (s^2 is of the order of s_f^2 there, and z = O(1)), as nei_grad_reference.FAR_SHIFT does.
FAR_SHIFT = 1.5


def inputs(case, acq):
    """(kern, X, y, Xs, Xp, S, seed, params): test_pend_gpu.inputs' recipe for a case; EI and PI: see FAR_SHIFT (the odd pending
    points from the fourth on move with the candidates, so that b(x) is not negligible there)."""
    kern, N, d, p, stress, S, R, seed = CASES[case]
    X, y, Xs = synth(N, d, R, seed)
    Xs = tp.XS_BOX * Xs
    Xp = tp.XS_BOX * np.random.default_rng(1000 + seed).random((p, d))
    if stress == "dup":
        Xp[1] = Xp[0]
    if stress == "obs":
        Xp[p // 2] = X[N // 2]
    params = tp.params_of(acq, y)
    if acq in ("EI", "PI"):
        shift = (1.0 + FAR_SHIFT * math.exp(tp.LL)) * np.eye(d)[0]
        Xs = Xs + shift
        Xp[3::2] += shift
        params = [tp.BETA]
    return kern, X, y, Xs, Xp, S, 77 + seed, params


def cov_fx(kern, A, B, il, s2f, dt):
    """(k(A, B), fx(A, B)) rows = points: dk(a, b)/da_k = fx il_k^2 (a_k - b_k); Matern 1/2: fx = 0 at r = 0."""
    D = (A * il)[:, None, :] - (B * il)[None, :, :]
    r2 = (D * D).sum(axis=2)
    with np.errstate(all="ignore"):
        if kern == "SEArd":
            k = s2f * np.exp(-r2 / dt(2.0))
            return k, -k
        if kern == "Mat52Ard":
            s = np.sqrt(dt(5.0)) * np.sqrt(r2)
            return s2f * (dt(1.0) + s + s * s / dt(3.0)) * np.exp(-s), -(dt(5.0) / dt(3.0)) * s2f * (dt(1.0) + s) * np.exp(-s)
        if kern == "Mat32Iso":
            s = np.sqrt(dt(3.0) * r2)
            return s2f * (dt(1.0) + s) * np.exp(-s), -dt(3.0) * s2f * np.exp(-s)
        rho = np.sqrt(r2)                                                    # Mat12Iso
        k = s2f * np.exp(-rho)
        return k, np.where(rho > 0, -k / np.where(rho > 0, rho, dt(1.0)), dt(0.0))


def partials(acq, params, m, s2, tau):
    """(d/dmu, d/ds2) of the functor, float64: acq_partials' closed forms (kernels_score.hip); tau (S1,) or None."""
    if acq in pr.TAU_ACQS:
        return tau_partials(acq, m, s2, tau)
    one = np.ones(np.broadcast(m, s2).shape)
    with np.errstate(all="ignore"):
        if acq == "UCB":
            return one, np.where(s2 > 0.0, params[0] / (2.0 * np.sqrt(np.where(s2 > 0.0, s2, 1.0))), 0.0) * one
        if acq == "MI":
            return one, params[0] / (2.0 * np.sqrt(s2 + params[1])) * one
    return one, 0.0 * one


class Twin:
    """One fit and the pending state at the precision dt: L, alpha, V_p, mu_p, L_p and A = K^-1 K(X, Xp)."""

    def __init__(self, kern, X, y, Xp, dt=np.float64, fit=None):
        self.kern, self.dt, self._moments = kern, dt, {}
        self.X, self.Xp, y = np.asarray(X, dtype=dt), np.asarray(Xp, dtype=dt), np.asarray(y, dtype=dt)
        self.il = np.exp(-dt(tp.LL)) * np.ones(self.X.shape[1], dtype=dt)
        self.s2f, self.beta = np.exp(dt(2.0) * dt(tp.LSIG)), dt(tp.BETA)
        nu = np.exp(dt(2.0) * dt(tp.LNOISE)) + dt(pr.NOISE_EPS)
        if fit is None:                                                      # (fit: a twin of the same data whose factor is shared)
            self.L = nr.chol(self.cov(self.X, self.X)[0] + nu * np.eye(len(y), dtype=dt))
            self.alpha = nr.solve_lower_t(self.L, nr.solve_lower(self.L, y - self.beta))
        else:
            self.L, self.alpha = fit.L, fit.alpha
        Kp = self.cov(self.X, self.Xp)[0]
        self.Vp = nr.solve_lower(self.L, Kp)
        self.mu_p = self.beta + Kp.T @ self.alpha
        self.Lp = nr.chol(self.cov(self.Xp, self.Xp)[0] - self.Vp.T @ self.Vp + nu * np.eye(len(self.Xp), dtype=dt))
        self.A = nr.solve_lower_t(self.L, self.Vp)

    def cov(self, A, B):
        return cov_fx(self.kern, A, B, self.il, self.s2f, self.dt)

    def moments(self, Xs):
        """mu (R), s^2 (R), B (R, p), U = K^-1 K* (N, R) at the rows of Xs (kept: every acquisition of a case shares them)."""
        key = Xs.tobytes()
        if key not in self._moments:
            Ks = self.cov(self.X, Xs)[0]
            V = nr.solve_lower(self.L, Ks)
            var0 = np.maximum(self.s2f - (V * V).sum(axis=0), 0)
            B = nr.solve_lower(self.Lp, (self.cov(Xs, self.Xp)[0] - V.T @ self.Vp).T).T
            self._moments = {key: (self.beta + Ks.T @ self.alpha, np.maximum(var0 - (B * B).sum(axis=1), 0), B,
                                   nr.solve_lower_t(self.L, V))}
        return self._moments[key]

    def taus(self, acq, params, Z, raise_tau):
        if acq not in pr.TAU_ACQS:
            return None
        Yf = np.asarray(self.mu_p[None, :] + np.asarray(Z, dtype=self.dt) @ self.Lp.T, dtype=np.float64)
        return np.array([max(params[0], float(yf.max())) if raise_tau else params[0] for yf in Yf])

    def score(self, Xs, acq, params, Z, raise_tau=False):
        """(score (R), each (S1, R), m (R, S1), s^2, tau): float64 functors of the moments at the twin's precision."""
        mu, s2, B, _ = self.moments(np.asarray(Xs, dtype=self.dt))
        m = np.asarray(mu[:, None] + B @ np.asarray(Z, dtype=self.dt).T, dtype=np.float64)
        s64, tau = np.asarray(s2, dtype=np.float64), self.taus(acq, params, Z, raise_tau)
        each = np.array([pr.acq(acq, pr.with_tau(acq, params, tau[s]) if tau is not None else params, m[:, s], s64) for s in range(len(Z))])
        return pr.average(acq, each), each, m, s64, tau

    def gradient(self, Xs, acq, params, Z, raise_tau=False):
        """(grad (R, d), score (R)): the header's formula."""
        dt = self.dt
        Xs, Zd = np.asarray(Xs, dtype=dt), np.asarray(Z, dtype=dt)
        score, each, m, s64, tau = self.score(Xs, acq, params, Z, raise_tau)
        _, _, B, U = self.moments(Xs)
        S1 = len(Z)
        dmu, ds2 = partials(acq, params, m, s64[:, None], None if tau is None else tau[None, :])
        with np.errstate(all="ignore"):
            if acq == "LogEI":
                v = each.T
                vmax = v.max(axis=1, keepdims=True)
                e = np.where(v == vmax, 1.0, np.exp(v - vmax))
                p = np.where(vmax == -np.inf, 0.0, e / e.sum(axis=1, keepdims=True))
            else:
                p = np.full(dmu.shape, 1.0 / S1)
            omega = np.asarray(np.where(p == 0.0, 0.0, p * dmu), dtype=dt)                   # (R, S1)
            gamma = np.asarray(np.where(s64 > 0.0, np.where(p == 0.0, 0.0, p * ds2).sum(axis=1), 0.0), dtype=dt)
        t = nr.solve_lower_t(self.Lp, (omega @ Zd - dt(2.0) * gamma[:, None] * B).T).T       # (R, p)
        E =omega.sum(axis=1)[:, None] * self.alpha[None, :] - dt(2.0) * gamma[:, None] * U.T - t @ self.A.T
        il2 = self.il * self.il
        grad = (np.einsum("rn,rnk->rk", self.cov(Xs, self.X)[1] * E, Xs[:, None, :] - self.X[None, :, :])
                + np.einsum("ri,rik->rk", self.cov(Xs, self.Xp)[1] * t, Xs[:, None, :] - self.Xp[None, :, :])) * il2
        return grad, score


_REF = {}


def normals(case):
    kern, N, d, p, stress, S, R, seed = CASES[case]
    return tp.normals(77 + seed, S, p)


def reference(case, acq, raise_tau=False, dt=np.float64):
    """dict(grad (R, d), score, Xs, Xp, params, S, seed) of one case, computed once and shared."""
    key = (case, acq, raise_tau, dt)
    if key not in _REF:
        kern, X, y, Xs, Xp, S, seed, params = inputs(case, acq)
        tkey, okey = (case, acq in ("EI", "PI"), dt), (case, acq not in ("EI", "PI"), dt)
        if tkey not in _REF:
            _REF[tkey] = Twin(kern, X, y, Xp, dt, fit=_REF.get(okey))
        grad, score = _REF[tkey].gradient(Xs, acq, params, normals(case), raise_tau)
        _REF[key] = dict(grad=grad, score=score, kern=kern, X=X, y=y, Xs=Xs, Xp=Xp, params=params, S=S, seed=seed)
    return _REF[key]


def distance(acq, got, ref_grad):
    """max |got - ref| over a candidate's components, per candidate, in WORST_GRAD's units."""
    g = np.asarray(ref_grad, dtype=np.float64)
    d = np.abs(np.asarray(got, dtype=np.float64) - g).max(axis=1)
    if acq == "LogEI":
        return d / np.maximum(1.0, np.abs(g).max(axis=1))
    return d / (math.exp(-tp.LL) * (1.0 if acq == "PI" else math.exp(tp.LSIG)))
