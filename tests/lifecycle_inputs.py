"""Inputs of the life-cycle tests (tests/test_lifecycle_gpu.py, tests/test_lifecycle_host.py).  No device.  A helper, not a test module.

One scripted history per (kernel, d) pair: what a Bayesian-optimisation loop does to a handle between its creation and its 206th
observation -- a first fill, appends of 1 ... 32 rows, two capacity doublings (each a re-allocation with another leading dimension),
a change of every hyper-parameter with no fit_() behind it.  `plan` restates the library's routing rules (csrc/bohip.hip
bohip_gp_append, alloc_model) so that the device test can assert, step by step, that an append took the route the history was written
for; `checkpoint` gives the data, the hyper-parameters and the NumPy twin of the model at each of the places where features are called.

Part A's reference of the resident inverse factor is `inv_lower_ld` (forward substitution in np.longdouble on the DEVICE's own L) and
its bound `inverse_bounds`: the componentwise forward bound of triangular inversion, N eps (|W| |L| |W|)_ij (Higham, Accuracy and
Stability, 2nd ed., section 14.2: every method that computes W row by row or column by column by substitution satisfies
|W^ - W| <= c_N u |W| |L| |W| + O(u^2)), and the normwise form N eps kappa_inf(L) max|W| that is all a block method guarantees."""
import functools
import math

import numpy as np
import scipy.linalg as sl

import batch_reference as br
import path_reference as pr
from conftest import synth
from matern_reference import MaternGP

EPS = np.finfo(np.float64).eps
TILE, APPEND_PMAX = 128, 32                                                 # csrc/common.h, csrc/kernels_linalg.hip
PAIRS = (("SEArd", 3), ("Mat32Iso", 9))                                     # d = 9: the LOW instantiations in dimension bucket 16
CAPACITY = 100
N_END = 206
R_SCORE = (300, 40, 700)                                                    # R1, R2 < R1, R3 > R1
R_COV = (200, 30, 260)                                                      # ... of the features that factor Sigma
# (action, argument): "call" = the feature under test is called there, with candidate counts given by index into R_SCORE / R_COV
HISTORY = (("append", 90), ("call", "warm"), ("append", 5), ("append", 32), ("call", "A"),
           ("append", 1), ("append", 2), ("append", 3), ("append", 32), ("call", "B"),
           ("hyper", None), ("call", "C"),
           ("append", 32), ("append", 1), ("append", 5), ("append", 3), ("call", "D"))
CALLS = {"warm": (0,), "A": (1, 2), "B": (0,), "C": (0,), "D": (0,)}
N_AT = {"warm": 90, "A": 127, "B": 165, "C": 165, "D": 206}
CHECKPOINTS = ("A", "B", "C", "D")
# rows [lo, n) of W were written by appends since the last refit (the others by a refit)
APPENDED_FROM = {"A": 127, "B": 127, "C": 165, "D": 203}

# (ll, lsigma, logNoise, beta) before and after step 7: test_qei_gpu's and test_matern_gpu's to begin with (their twins are well
# conditioned there), then every one of them changed
HYPER = {"SEArd": ((np.full(3, -0.4), 0.2, -1.0, 0.1), (np.array([-0.6, -0.3, -0.5]), 0.35, -1.3, 0.25)),
         "Mat32Iso": ((np.array([-0.5]), 0.1, -2.0, 0.05), (np.array([-0.3]), 0.25, -1.6, -0.1))}


def ld_of(cap):
    """alloc_model: the row stride of L, W and W'."""
    return -(-(cap + 1) // TILE) * TILE + 16


def plan(history=HISTORY, capacity=CAPACITY, reads_model=True):
    """The history as the library routes it: a list of dicts(action, arg, n, cap, ld, refits, appends, route, freshen), the counters
    cumulative and as they stand after the step.  route: "refit" (a first fill, a growth or a stale handle), "incremental"
    (append_incremental) or None (a call).  reads_model: whether the feature called at a checkpoint reaches ensure_fresh.  One that
    does not (it reads the observations alone) leaves a stale handle stale: `freshen` then tells the driver to predict at one point
    after the call, so that the rest of the history takes the table's routes whatever the feature."""
    n, cap, refits, appends, stale, out = 0, capacity, 0, 0, True, []
    for action, arg in history:
        route, freshen = None, False
        if action == "append":
            n_old, n = n, n + arg
            if n > cap:                                                     # growth: alloc_model(max(2 cap, n)), then a refit
                cap, route = max(2 * cap, n), "refit"
            elif not stale and n_old > 0 and arg <= APPEND_PMAX:
                route = "incremental"
            else:
                route = "refit"
            refits, appends, stale = refits + (route == "refit"), appends + (route == "incremental"), False
        elif action == "hyper":
            stale = True
        elif action == "call" and stale:
            freshen = not reads_model
            refits, stale = refits + (0 if freshen else 1), False
        out.append(dict(action=action, arg=arg, n=n, cap=cap, ld=ld_of(cap), refits=refits, appends=appends, route=route, freshen=freshen))
        refits += freshen
    return out


@functools.lru_cache(maxsize=None)
def data(kern, d):
    """(X[206, d], y, Xs[700, d]) of a pair, read-only."""
    X, y, Xs = synth(N_END, d, max(R_SCORE), seed=1000 + 7 * N_END + 3 * d)
    for a in (X, y, Xs):
        a.setflags(write=False)
    return X, y, Xs


def hyper(kern, ck):
    return HYPER[kern][1 if ck in ("C", "D") else 0]


def theta_of(hyp):
    """[logNoise, mean, ll..., lsigma]: mll_grad_batch's row."""
    ll, lsig, lnoise, beta = hyp
    return np.concatenate([[lnoise, beta], np.atleast_1d(ll), [lsig]])


class Checkpoint:
    """The model a handle must hold at a checkpoint: data, hyper-parameters, the twin and its tolerances' ingredients."""

    def __init__(self, kern, d, name):
        X, y, Xs = data(kern, d)
        self.kern, self.d, self.name, self.n = kern, d, name, N_AT[name]
        self.X, self.y, self.Xs = X[:self.n], y[:self.n], Xs
        self.hyp = hyper(kern, name)
        self.ll, self.lsig, self.lnoise, self.beta = self.hyp
        self.ref = MaternGP(kern, self.X, self.y, self.ll, self.lsig, self.lnoise, self.beta)
        self.s2f = self.ref.s2f
        self.floor = 64 * EPS * self.s2f * np.abs(self.ref.alpha).sum()     # test_parity_gpu.mu_floor

    def __repr__(self):
        return f"{self.kern} d={self.d} checkpoint {self.name} (N = {self.n})"


@functools.lru_cache(maxsize=None)
def checkpoint(kern, d, name):
    return Checkpoint(kern, d, name)


@functools.lru_cache(maxsize=None)
def posterior(kern, d, name, R):
    """(mu, Sigma) of the twin over the first R candidates, read-only."""
    ck = checkpoint(kern, d, name)
    mu, cov = ck.ref.predict_cov(ck.Xs[:R])
    mu.setflags(write=False)
    cov.setflags(write=False)
    return mu, cov


# ---- Part A: the inverse factor ------------------------------------------------------------------------------------------------------
def inv_lower_ld(L):
    """L^-1 of a lower-triangular float64 L by forward substitution in np.longdouble, row by row; returned in np.longdouble."""
    Lq = np.asarray(L, dtype=np.longdouble)
    n = Lq.shape[0]
    W = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        row = -(Lq[i, :i] @ W[:i, :]) if i else np.zeros(n, dtype=np.longdouble)
        row[i] += 1.0
        W[i] = row / Lq[i, i]
    return W


def inverse_bounds(L, Wref):
    """(componentwise[n, n], normwise scalar): N eps (|W| |L| |W|)_ij and N eps kappa_inf(L) max|W|."""
    n = L.shape[0]
    aW, aL = np.abs(np.asarray(Wref, dtype=np.float64)), np.abs(L)
    comp = n * EPS * (aW @ aL @ aW)
    kappa = float(np.max(aL.sum(axis=1)) * np.max(aW.sum(axis=1)))
    return np.tril(comp), n * EPS * kappa * float(aW.max())


def inverse_share(W, Wref, bound, rows=slice(None)):
    """Worst |W - Wref| / bound over the lower triangle of the given rows (bound an array or a scalar)."""
    n = W.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))[rows]
    err = np.abs(np.asarray(W, dtype=np.longdouble) - Wref)[rows].astype(np.float64)
    b = np.broadcast_to(bound, (n, n))[rows] if np.ndim(bound) else np.full(err.shape, float(bound))
    if not low.any():
        return 0.0
    return float(np.max(err[low] / b[low]))


# ---- Part C: the jittered model ------------------------------------------------------------------------------------------------------
JIT_REL, JIT_TRIES = 1e-3, 3
JIT_LL, JIT_LSIG, JIT_LNOISE, JIT_BETA = np.zeros(2), 5.0, -25.0, 0.0
JIT_SEED = 5                                                               # the candidates' seed (non-vacuity is asserted on it)


def jitter_data():
    """test_hardening_gpu's singular model: 60 positions observed five times each."""
    rng = np.random.default_rng(11)
    pos = rng.random((60, 2)) * 10 - 5
    X = np.repeat(pos, 5, axis=0)
    y = -(((X - 1) ** 2).sum(1) + rng.standard_normal(len(X)))
    Xa = rng.random((3, 2)) * 10 - 5                                       # the three rows of the incremental append
    ya = -(((Xa - 1) ** 2).sum(1))
    return X, y, Xa, ya


def jitter_candidates(R, seed=JIT_SEED):
    return np.random.default_rng(seed).random((R, 2)) * 10 - 5


def lognoise_with(lognoise, J):
    """A jittered model is exactly a model whose noise is nu0 + J: the logNoise every twin takes."""
    return 0.5 * math.log(math.exp(2.0 * lognoise) + J)


JIT_R, JIT_Q, JIT_M, JIT_PATH_SEED = 300, 4, 256, 2024
JIT_BATCH = (("UCB", [2.0], "believer"), ("MI", [1.0, 0.3], "max"))        # (acquisition, its parameters, the fantasy)


def jitter_factory(J, fantasy_noise_has_j=True):
    """batch_reference's model of the jittered handle: fitted with nu0 + J on the diagonal.  fantasy_noise_has_j = False is the twin
    of a library that forgot J in the noise of the fantasised observation (the factor is still the jittered one)."""
    def make(X, y):
        f = br._Fitted("SEArd", X, y, JIT_LL, JIT_LSIG, lognoise_with(JIT_LNOISE, J), JIT_BETA)
        if not fantasy_noise_has_j:
            f.lognoise = JIT_LNOISE                                         # (recurrence reads the noise of the fantasy from here)
        return f
    return make


def jitter_batch_twin(X, y, Xs, acq, params, fantasy, J, fantasy_noise_has_j=True):
    fv = fantasy if fantasy == "believer" else float(y.max())
    return br.recurrence(jitter_factory(J, fantasy_noise_has_j), X, y, Xs, acq, params, JIT_Q, fv)


def batch_tols(row, N, s2f):
    """test_batch_gpu.compare's tolerances of one round: (val, mu, var)."""
    _, v0, mu0, var0, _, asum = row
    fl = 64 * EPS * s2f * asum
    return 1e-6 * abs(v0) + fl + 1e-12, 1e-6 * abs(mu0) + fl + 1e-12, 1e-6 * abs(var0) + 64 * N * EPS * s2f


def batch_moved(a, b, N, s2f):
    """How far the rounds of two twins lie apart, in units of batch_tols (inf when they pick another candidate)."""
    worst = 0.0
    for ra, rb in zip(a, b):
        if ra[0] != rb[0]:
            return math.inf
        tv, tm, ts = batch_tols(ra, N, s2f)
        worst = max(worst, abs(ra[1] - rb[1]) / tv, abs(ra[2] - rb[2]) / tm, abs(ra[3] - rb[3]) / ts)
    return worst


def jitter_path_twin(X, y, J):
    return pr.PathTwin("SEArd", X, y, JIT_LL, JIT_LSIG, lognoise_with(JIT_LNOISE, J), JIT_BETA, JIT_M, JIT_PATH_SEED)


def path_solve_bound(tw, u, w, rhs, ze):
    """test_path_gpu's bound on |K u - rhs|, entry by entry."""
    return (64 * tw.N * EPS * (np.abs(tw.K) @ np.abs(u) + np.abs(rhs)) + tw.value_bound(tw.X, np.zeros(tw.N), w)
            + math.sqrt(tw.diag) * pr.normal_tol(ze))


def solve_inverse(L):
    """float64 L^-1 by LAPACK's substitution (the host test measures its share of the bound)."""
    return sl.solve_triangular(L, np.eye(L.shape[0]), lower=True)
