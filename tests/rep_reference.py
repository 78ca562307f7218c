"""NumPy twin of a model with replicated sites (include/bohip_rep.h), and the inputs of its tests.  No device.  A helper
of tests/test_rep_host.py and tests/test_rep_gpu.py, not a test module.

A site is a position x_i with the mean ybar_i of its r_i evaluations, r_i, and s_i = sum_j (y_ij - ybar_i)^2.  With
nu = exp(2 logNoise) + NOISE_EPS the twin restates the contract:

    cK_w = K + nu diag(1 / r_i),  L = chol(cK_w),  alpha = cK_w^-1 (ybar - beta)
    mu = beta + K*' alpha,  sigma^2 = max(s_f^2 - |L^-1 k*|^2, 0)
    mll = [-1/2 (ybar - beta)' alpha - sum log L_ii - n/2 log 2 pi] + C
    C   = -1/2 (N_tot - n) log(2 pi nu) - 1/2 sum log r_i - (sum s_i) / (2 nu)
    d mll / d logNoise = 2 s^2 sum_i G_ii / r_i + 2 s^2 (-(N_tot - n) / (2 nu) + (sum s_i) / (2 nu^2)),  G = 1/2 (alpha alpha' - cK_w^-1)

Every step (the kernel, the Cholesky factorisation, the substitutions) is written out in the array's own dtype, so the same class runs
in float64 and in np.longdouble; nothing goes through LAPACK.  `ignore_weights=True` is the WRONG model, every 1 / r_i forced to 1 with
the site means kept: what a library computes that stores the sites and forgets the weights (the non-vacuity check of the host test).

The independent reference of every posterior and likelihood number is the model with every evaluation as a row of its own (`expand`):
the C oracle for SEArd, and for Mat32Iso -- a family the C oracle does not have -- matern_reference.MaternGP, the independent NumPy
model that every Matérn test of the suite is held to.  The twin is the reference only of L and alpha, whose shape differs.
"""
import functools
import math

import numpy as np

from matern_reference import KERNELS
from oracle.oracle import NOISE_EPS

EPS = np.finfo(np.float64).eps
D = 3
KERNS = ("SEArd", "Mat32Iso")
HYPERS = ((-2.0, 0.0), (-2.0, 1.0), (0.0, 5.0))                              # (logNoise, log sigma_f)
BETA = 0.1
LL = {"SEArd": np.linspace(-0.9, -0.3, D), "Mat32Iso": np.array([-0.5])}
SEED = 4100                                                                  # (test_rep_host asserts non-vacuity on every input made from it)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def draw_reps(n, rng):
    """r_i from {1 ... 5}, at least a quarter of the sites (the first ones drawn, then shuffled) at r = 1."""
    r = rng.integers(1, 6, n)
    r[:-(-n // 4)] = 1
    rng.shuffle(r)
    return r.astype(np.int64)


@functools.lru_cache(maxsize=None)
def raw(n, lnoise, lsig, seed=SEED):
    """(pos[n, D], reps[n], evals: list of n arrays, Xs[700, D]) of one input, read-only: evaluations of s_f (sum sin 3x) with noise
    exp(logNoise), so that the data has the scale the hyper-parameters say."""
    rng = np.random.default_rng(seed + n)
    pos = rng.random((n, D))
    reps = draw_reps(n, rng)
    f = math.exp(lsig) * np.sin(3 * pos).sum(1)
    evals = tuple(f[i] + math.exp(lnoise) * rng.standard_normal(int(reps[i])) for i in range(n))
    Xs = rng.random((700, D))
    for a in (pos, reps, Xs) + evals:
        a.setflags(write=False)
    return pos, reps, evals, Xs


def sites_of(pos, evals, lo=0, hi=None):
    """The sites [lo, hi) as append_sites_ takes them: (x[D, p], ybar, reps, ss, ymax), the statistics two-pass."""
    hi = len(evals) if hi is None else hi
    ybar = np.array([v.sum() / v.size if v.size > 1 else v[0] for v in evals[lo:hi]])
    reps = np.array([v.size for v in evals[lo:hi]], dtype=np.int64)
    ss = np.array([float(np.sum((v - m) ** 2)) if v.size > 1 else 0.0 for v, m in zip(evals[lo:hi], ybar)])
    ymax = np.array([v.max() for v in evals[lo:hi]])
    return np.asfortranarray(pos[lo:hi].T), ybar, reps, ss, ymax


def expand(pos, evals, lo=0, hi=None):
    """The same sites with every evaluation as a row of its own: (X[N_tot, D], y[N_tot]), a site's evaluations adjacent."""
    hi = len(evals) if hi is None else hi
    X = np.repeat(pos[lo:hi], [v.size for v in evals[lo:hi]], axis=0)
    y = np.concatenate([v for v in evals[lo:hi]]) if hi > lo else np.zeros(0)
    return np.ascontiguousarray(X), y


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
def _k_and_fx(fam, r, s2f, T):
    """(k, 2 dk/dr) of the family at the squared scaled distances r, in dtype T."""
    if fam == "SE":
        k = s2f * np.exp(-r / T(2))
        return k, -k
    if fam == "M32":
        s = np.sqrt(T(3)) * np.sqrt(r)
        e = np.exp(-s)
        return s2f * (T(1) + s) * e, -T(3) * s2f * e
    raise KeyError(fam)


def chol_lower(A):
    """Cholesky factor of A in A's dtype, column by column (no LAPACK: np.longdouble has none)."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        dj = A[j, j] - L[j, :j] @ L[j, :j]
        if not dj > 0:
            raise np.linalg.LinAlgError(f"not positive definite at pivot {j + 1}")
        L[j, j] = np.sqrt(dj)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution in L's dtype (B a vector or a matrix of right-hand sides)."""
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_upper_t(L, B):
    """L^-T B by back substitution."""
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


class RepTwin:
    """The model of one weighted handle: sites X (n, D) row-major, ybar, reps, ss; dtype float64 or np.longdouble."""

    def __init__(self, kern, X, ybar, reps, ss, loglen, logsig, lognoise, beta, dtype=np.float64, ignore_weights=False, jitter=0.0):
        T = self.T = dtype
        self.kern, (self.fam, self.iso) = kern, KERNELS[kern]
        self.X, self.ybar = np.asarray(X, dtype=T), np.asarray(ybar, dtype=T)
        self.n, self.d = self.X.shape
        self.reps = np.asarray(reps, dtype=np.int64)
        self.invr = np.ones(self.n, dtype=T) if ignore_weights else T(1) / self.reps.astype(T)
        self.ss_total = np.sum(np.asarray(ss, dtype=T))
        self.beta = T(beta)
        ll = np.atleast_1d(np.asarray(loglen, dtype=T))
        self.il2 = np.exp(-T(2) * (np.full(self.d, ll[0], dtype=T) if self.iso else ll))
        self.s2f, self.s2n = np.exp(T(2) * T(logsig)), np.exp(T(2) * T(lognoise))
        self.nu = self.s2n + T(NOISE_EPS) + T(jitter)
        diff = self.X[:, None, :] - self.X[None, :, :]
        self.D2 = diff * diff
        self.r = self.D2 @ self.il2
        self.K, self.fx = _k_and_fx(self.fam, self.r, self.s2f, T)
        self.cK = self.K + np.diag(self.nu * self.invr)
        self.L = chol_lower(self.cK)
        self.alpha = solve_upper_t(self.L, solve_lower(self.L, self.ybar - self.beta))

    def kstar(self, Xs):
        Xs = np.asarray(np.atleast_2d(Xs), dtype=self.T)
        diff = self.X[:, None, :] - Xs[None, :, :]
        return _k_and_fx(self.fam, (diff * diff) @ self.il2, self.s2f, self.T)[0]          # (n, R)

    def predict(self, Xs):
        Ks = self.kstar(Xs)
        V = solve_lower(self.L, Ks)
        return self.beta + Ks.T @ self.alpha, np.maximum(self.s2f - np.sum(V * V, axis=0), self.T(0))

    def predict_cov(self, Xs):
        Xs = np.asarray(np.atleast_2d(Xs), dtype=self.T)
        Ks = self.kstar(Xs)
        V = solve_lower(self.L, Ks)
        diff = Xs[:, None, :] - Xs[None, :, :]
        return self.beta + Ks.T @ self.alpha, _k_and_fx(self.fam, (diff * diff) @ self.il2, self.s2f, self.T)[0] - V.T @ V

    def site_constant(self):
        """(C, dC / d logNoise)."""
        T, m = self.T, self.T(int(self.reps.sum()) - self.n)
        Cv = -m / T(2) * np.log(T(2) * T(np.pi) * self.nu) - np.sum(np.log(self.reps.astype(T))) / T(2) - self.ss_total / (T(2) * self.nu)
        return Cv, T(2) * self.s2n * (-m / (T(2) * self.nu) + self.ss_total / (T(2) * self.nu * self.nu))

    def mll(self):
        T = self.T
        own = -(self.ybar - self.beta) @ self.alpha / T(2) - np.sum(np.log(np.diag(self.L))) - T(self.n) / T(2) * np.log(T(2) * T(np.pi))
        return own + self.site_constant()[0]

    def kinv(self):
        W = solve_lower(self.L, np.eye(self.n, dtype=self.T))
        return W.T @ W

    def mll_grad(self):
        """(mll, d/dlogNoise, d/dbeta, d/d[ll..., lsigma]) in GaussianProcesses.get_params order, all in the twin's dtype."""
        T = self.T
        G = (np.outer(self.alpha, self.alpha) - self.kinv()) / T(2)
        dll = np.einsum("ij,ijk->k", G * (-self.fx), self.D2 * self.il2)
        dkern = np.concatenate([[dll.sum()] if self.iso else dll, [np.sum(G * T(2) * self.K)]])
        dnoise = T(2) * self.s2n * np.sum(np.diag(G) * self.invr) + self.site_constant()[1]
        return self.mll(), dnoise, np.sum(self.alpha), dkern

    def loo(self):
        """(mu, var, logp, total) of leaving one SITE out: bohip_loo.h's formulas on cK_w (the prediction of the site's mean)."""
        kap = np.diag(self.kinv())
        logp = np.log(kap) / 2 - self.alpha ** 2 / kap / 2 - np.log(2 * np.pi) / 2
        return self.ybar - self.alpha / kap, 1 / kap, logp, logp.sum()


# ---- the bounds the device is held to (tests/test_parity_gpu.py, unchanged) -------------------------------------------------------------
def mu_floor(alpha, s2f):
    return 64 * EPS * s2f * np.abs(alpha).sum()


def var_tol(ref, N, s2f, rel=1e-6):
    return rel * np.abs(ref) + 64 * N * EPS * s2f


def mu_bound(mu_ref, alpha_ref, s2f):
    """test_seeded_vs_oracle: |d mu| <= 1e-6 |ref| + mu_floor."""
    return 1e-6 * np.abs(mu_ref) + mu_floor(alpha_ref, s2f)


def score_bound(acq, p, sc_ref, var_ref, alpha_ref, N, s2f):
    """test_seeded_vs_oracle's bound of a score: check_scores with its floor."""
    fl = mu_floor(alpha_ref, s2f)
    if acq in ("UCB", "MI"):
        floor = fl + max(1.0, abs(p[0])) * np.sqrt(var_tol(var_ref, N, s2f, rel=0))
    else:
        floor = fl + var_tol(var_ref, N, s2f, rel=0) + 1e-15
    return 1e-6 * np.abs(sc_ref) + floor


def grad_bound(g_ref):
    """test_mll_gradient_vs_oracle: rtol 1e-6, atol 1e-8 max|g|."""
    g_ref = np.asarray(g_ref, dtype=np.float64)
    return 1e-6 * np.abs(g_ref) + 1e-8 * np.abs(g_ref).max()


MLL_RTOL = 1e-9                                                              # every mll check of the suite


# ---- the expanded reference ------------------------------------------------------------------------------------------------------------
class Expanded:
    """The model with every evaluation as its own row, by the suite's independent references: the C oracle (SEArd) or MaternGP (Mat32Iso).
    predict -> (mu, var); score -> scores; mll_grad -> (mll, [dlogNoise, dbeta, dkern...]); alpha, N, s2f for the bounds."""

    def __init__(self, kern, X, y, ll, lsig, lnoise, beta, orc=None):
        self.kern, self.X, self.y, self.N = kern, X, y, len(y)
        self.ll, self.lsig, self.lnoise, self.beta, self.orc = ll, lsig, lnoise, beta, orc
        self.s2f = math.exp(2 * lsig)
        if kern == "SEArd":
            self.L, self.alpha = orc.fit(X, y, ll, lsig, lnoise, beta)
        else:
            from matern_reference import MaternGP

            self.gp = MaternGP(kern, X, y, ll, lsig, lnoise, beta)
            self.L, self.alpha = self.gp.L, self.gp.alpha

    def predict(self, Xs):
        if self.kern == "SEArd":
            return self.orc.predict(self.X, self.ll, self.lsig, self.beta, self.L, self.alpha, Xs)
        return self.gp.predict(Xs)

    def score(self, acq, p, Xs):
        if self.kern == "SEArd":
            return self.orc.score(self.X, self.ll, self.lsig, self.beta, self.L, self.alpha, acq, p, Xs)[0]
        return self.gp.score(acq, p, Xs)

    def mll_grad(self):
        if self.kern == "SEArd":
            return self.orc.mll_grad(self.X, self.y, self.ll, self.lsig, self.lnoise, self.beta)
        m, dn, dm, dk = self.gp.mll_grad()
        return m, np.concatenate([[dn, dm], np.ravel(dk)])


# ---- the history of the device test ------------------------------------------------------------------------------------------------------
# tests/lifecycle_inputs.py's shape at small size: capacity 100; 10 plain rows (the handle turns weighted later, with rows in it); a
# fill of 80 sites (a refit: past APPEND_PMAX) so that the appends that follow cross what the lifecycle history crosses -- 5 (incremental),
# 32 (95 + 32 > 100: growth, refit), 1 (127 -> 128 sites: Npad 128 -> 256), 2, 3; a plain append_ of 2 rows on the weighted handle; every
# hyper-parameter changed with no fit_(); 33 sites (past APPEND_PMAX: a refit).
CAPACITY, APPEND_PMAX = 100, 32
HISTORY = (("plain", 10), ("sites", 80), ("sites", 5), ("sites", 32), ("sites", 1), ("sites", 2), ("sites", 3), ("plain", 2),
           ("hyper", None), ("sites", 33))
N_ROWS = sum(a for k, a in HISTORY if k != "hyper")


def hyper_after(kern, lnoise, lsig):
    """(ll, lsig, lnoise, beta) after the "hyper" step: every one of them changed."""
    return LL[kern] + 0.1, lsig + 0.15, lnoise - 0.3, BETA + 0.15


@functools.lru_cache(maxsize=None)
def history_data(lnoise, lsig):
    """(pos[N_ROWS, D], evals, Xs) of the history: raw()'s sites, the rows of the "plain" steps cut to their first evaluation."""
    pos, _, evals, Xs = raw(N_ROWS, lnoise, lsig)
    evals, lo = list(evals), 0
    for kind, a in HISTORY:
        if kind == "plain":
            evals[lo:lo + a] = [v[:1] for v in evals[lo:lo + a]]
        lo += 0 if kind == "hyper" else a
    return pos, tuple(evals), Xs


def history_plan():
    """The history as the library routes it (csrc/bohip.hip append_rows): dicts(kind, arg, lo, n, cap, route, weighted, refits, appends),
    the counters cumulative and as they stand after the step AND the reads that follow it (the first read after "hyper" refits)."""
    n, cap, refits, appends, stale, weighted, out = 0, CAPACITY, 0, 0, True, False, []
    for kind, a in HISTORY:
        route, lo = None, n
        if kind == "hyper":
            refits += 1                                                     # (the reads of the check that follows)
        else:
            n += a
            weighted = weighted or kind == "sites"
            if n > cap:
                cap, route = max(2 * cap, n), "refit"
            elif not stale and lo > 0 and a <= APPEND_PMAX:
                route = "incremental"
            else:
                route = "refit"
            refits, appends, stale = refits + (route == "refit"), appends + (route == "incremental"), False
        out.append(dict(kind=kind, arg=a, lo=lo, n=n, cap=cap, route=route, weighted=weighted, refits=refits, appends=appends))
    return out
