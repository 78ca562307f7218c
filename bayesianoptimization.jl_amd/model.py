"""Model adapter: the six generic functions through which the reference's BO loop touches the GP
(reference src/models/gp.jl:2-18), backed by the device-resident factor in libbohip.

Arrays keep the reference's Julia shapes: a batch of points is ``d x R`` (one point per COLUMN).
``np.asfortranarray`` of such an array has exactly the memory layout the C ABI wants
(every point = d contiguous doubles).
"""
from __future__ import annotations

import ctypes as C
import math
import weakref

import numpy as np

from . import _lib
from ._lib import Best, check

_dp = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _cols(x, d):
    """d x R (or length-d vector) -> Fortran-contiguous float64 d x R."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    if x.shape[0] != d:
        raise ValueError(f"expected {d} rows (one point per column), got shape {x.shape}")
    return np.asfortranarray(x)


# ---- GaussianProcesses.jl constructor vocabulary used by the reference --------------------------
class MeanZero:
    beta = 0.0


class MeanConst:
    def __init__(self, beta):
        self.beta = float(beta)


class _Kernel:
    kern = "SEArd"
    iso = False    # one length-scale (ll has 1 entry) instead of d

    def __init__(self, ll, lsigma):
        self.ll = np.atleast_1d(np.asarray(ll, dtype=np.float64)).copy()
        self.lsigma = float(lsigma)


class SEArd(_Kernel):
    """SEArd(ll::Vector, lσ): k = exp(2lσ) exp(-½ Σ (x-y)²/exp(2 ll_k))  (README.md:24)."""
    kern = "SEArd"


class SEIso(_Kernel):
    """SEIso(ll, lσ)  (test/acquisition.jl:2)."""
    kern = "SEIso"
    iso = True


class Mat52Ard(_Kernel):
    """Mat52Ard(ll::Vector, lσ)  (default model, src/BayesianOptimization.jl:259-262)."""
    kern = "Mat52Ard"


class Mat52Iso(_Kernel):
    """Mat52Iso(ll, lσ): k = exp(2lσ) (1 + √5ρ + 5ρ²/3) exp(-√5ρ), ρ = |x-y|/exp(ll)."""
    kern = "Mat52Iso"
    iso = True


class Mat32Ard(_Kernel):
    """Mat32Ard(ll::Vector, lσ): k = exp(2lσ) (1 + √3ρ) exp(-√3ρ), ρ² = Σ (x-y)²/exp(2 ll_k)."""
    kern = "Mat32Ard"


class Mat32Iso(_Kernel):
    """Mat32Iso(ll, lσ): Mat32Ard with one length-scale."""
    kern = "Mat32Iso"
    iso = True


class Mat12Ard(_Kernel):
    """Mat12Ard(ll::Vector, lσ): k = exp(2lσ) exp(-ρ), ρ² = Σ (x-y)²/exp(2 ll_k).  Not differentiable where a point meets
    an observation (ρ = 0): gradients take the minimum-norm subgradient there, that observation contributes 0."""
    kern = "Mat12Ard"


class Mat12Iso(_Kernel):
    """Mat12Iso(ll, lσ): Mat12Ard with one length-scale (same rule at ρ = 0)."""
    kern = "Mat12Iso"
    iso = True


def collapse_evaluations(x, y):
    """Repeated evaluations as weighted sites (include/bohip_rep.h): groups the byte-identical columns of x (d x N)
    within this call, in order of first occurrence, wherever they stand.  Returns (x_sites [d, n], ybar [n], reps [n] int64, ss [n],
    ymax [n]): the mean of a site's evaluations, their count, the within-site sum of squares sum_j (y_j - ybar)^2 computed in a second
    pass around the mean (exactly 0 for a single evaluation) and the largest raw value."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    x = np.asfortranarray(x)
    y = np.ascontiguousarray(np.atleast_1d(np.asarray(y, dtype=np.float64)))
    if x.shape[1] != y.size:
        raise ValueError("x and y disagree on the number of observations")
    first, members = {}, []
    for j in range(y.size):
        key = x[:, j].tobytes()
        if key not in first:
            first[key] = len(members)
            members.append([])
        members[first[key]].append(j)
    n = len(members)
    xs = np.asfortranarray(x[:, [m[0] for m in members]]) if n else np.zeros((x.shape[0], 0), order="F")
    ybar, reps, ss, ymax = np.empty(n), np.empty(n, dtype=np.int64), np.empty(n), np.empty(n)
    for i, m in enumerate(members):
        v = y[m]
        reps[i] = v.size
        ybar[i] = v[0] if v.size == 1 else v.sum() / v.size
        ss[i] = 0.0 if v.size == 1 else float(np.sum((v - ybar[i]) ** 2))
        ymax[i] = v.max()
    return xs, ybar, reps, ss, ymax


def refuse_weighted(model, what):
    """ValueError for a feature that cannot take a model with replicated sites: its device kernels build the covariance themselves,
    with one noise term for every row (include/bohip_rep.h lists the refused entry points)."""
    if getattr(model, "weighted", False):
        raise ValueError(f"{what} does not support a model with replicated sites (collapse=True / append_sites_ with reps > 1): "
                         "its kernels build the covariance with one noise term for every row; use a model with collapse=False")


def _refuse_site_member(m, owner):
    """The member models of a constrained or two-objective model are updated column by column, one value per member and evaluation:
    they take no replicated sites."""
    if getattr(m, "collapse", False) or getattr(m, "weighted", False):
        raise ValueError(f"{owner} members do not support replicated sites (collapse=True / append_sites_ with reps > 1): every "
                         "member takes every evaluation as a row of its own; use members with collapse=False")


class ElasticGPE:
    """Drop-in for ``ElasticGPE(d; mean, kernel, logNoise, capacity)`` (README.md:22-27).

    Owns a ``bohip_gp`` handle: x, y, the Cholesky factor, its inverse and alpha live in HBM and
    survive across ``boptimize_`` calls; ``append_`` extends the factor (reference ``append!``).
    ``collapse=True`` (an extension): ``update_`` and ``from_data`` turn the repeated evaluations of one call
    (``BOpt(..., repetitions=r)``) into one weighted site each -- the same posterior and marginal likelihood at n positions instead
    of n r rows.  ``model.x`` / ``model.y`` are then site positions and site means, ``model.reps`` the counts, ``nobs`` the number
    of sites and ``nevals`` of evaluations; ``maxy`` stays the largest raw evaluation.
    ``model.x`` (d x n) and ``model.y`` are host mirrors, as the reference reads those fields
    directly (src/BayesianOptimization.jl:117-119, src/acquisitionfunctions.jl:136).
    """

    hyper_samples = None   # (Theta[H, P], weights) once MarginalGPOptimizer has run: what Marginalised acquisitions average over

    def __init__(self, d, mean=None, kernel=None, logNoise=-2.0, capacity=1024, device=0, collapse=False):
        self.dim = int(d)
        self.collapse = bool(collapse)
        self.mean = mean if mean is not None else MeanZero()
        self.kernel = kernel if kernel is not None else SEArd(np.zeros(d), 0.0)
        self.logNoise = float(logNoise)
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.bohip_gp_create(self.dim, int(capacity), _lib.KERN[self.kernel.kern], int(device), C.byref(h)))
        self._h = h
        _lib.register(self)
        self._x = np.zeros((self.dim, 0), order="F")
        self._y = np.zeros(0)
        self._reps = np.zeros(0, dtype=np.int64)
        self._ymax = np.zeros(0)
        self._push_hyper()

    def close(self):
        """Release the device model now (idempotent; also run for every live model at interpreter exit)."""
        h, self._h = getattr(self, "_h", None), None
        for p in list(getattr(self, "_paths", ())):               # paths objects borrow the handle's stream: they go first
            p.close()
        if h:
            self._lib.bohip_gp_destroy(h)

    @classmethod
    def from_data(cls, x, y, mean=None, kernel=None, logNoise=-2.0, **kw):
        """GPE(x, y, mean, kernel[, logNoise]) (test/acquisitionfunctions.jl:4, test/acquisition.jl:2)."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        if kw.get("collapse", False):
            sites = collapse_evaluations(x, y)
            m = cls(x.shape[0], mean=mean, kernel=kernel, logNoise=logNoise, capacity=max(sites[0].shape[1], 1), **kw)
            m.append_sites_(*sites)
            return m
        m = cls(x.shape[0], mean=mean, kernel=kernel, logNoise=logNoise, capacity=max(x.shape[1], 1), **kw)
        m.append_(x, y)
        return m

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- hyper-parameters (GP.set_params!) ---------------------------------------------------------
    def _push_hyper(self):
        ll = self.kernel.ll
        if not self.kernel.iso and ll.size != self.dim:
            raise ValueError("kernel length-scale vector must have d entries")
        ll = np.ascontiguousarray(np.broadcast_to(ll, (self.dim,)) if ll.size == 1 else ll)
        check(self._lib.bohip_gp_set_hyper(self._h, _ptr(ll), self.kernel.lsigma, self.logNoise, self.mean.beta))

    def set_params_(self, ll=None, lsigma=None, logNoise=None, beta=None):
        if ll is not None:
            self.kernel.ll = np.atleast_1d(np.asarray(ll, dtype=np.float64)).copy()
        if lsigma is not None:
            self.kernel.lsigma = float(lsigma)
        if logNoise is not None:
            self.logNoise = float(logNoise)
        if beta is not None:
            self.mean = MeanConst(beta)
        self._push_hyper()

    # -- fields the reference reads directly -------------------------------------------------------
    @property
    def x(self):
        return self._x

    @property
    def y(self):
        return self._y

    @property
    def nobs(self):
        return self._y.size

    @property
    def reps(self):
        """Evaluations behind every row (all 1 unless sites were appended)."""
        return self._reps

    @property
    def nevals(self):
        return int(self._reps.sum())

    @property
    def ymax(self):
        """The largest raw evaluation of every row (= y for plain rows): what maxy reads."""
        return self._ymax

    @property
    def weighted(self):
        """Whether the handle holds a site of more than one evaluation (bohip_gp_sites_info)."""
        return bool(np.any(self._reps > 1))

    def sites_info(self):
        """(n_sites, n_evals, sum s_i, sum log r_i, weighted) as the handle keeps them (bohip_gp_sites_info)."""
        n, ne, w = C.c_int64(), C.c_int64(), C.c_int()
        ss, slr = C.c_double(), C.c_double()
        check(self._lib.bohip_gp_sites_info(self._h, C.byref(n), C.byref(ne), C.byref(ss), C.byref(slr), C.byref(w)))
        return int(n.value), int(ne.value), ss.value, slr.value, int(w.value)

    def get_reps(self):
        r = np.zeros(self.nobs, dtype=np.int64)
        check(self._lib.bohip_gp_get_reps(self._h, r.ctypes.data_as(C.POINTER(C.c_int64))))
        return r

    # -- append! / fit! ----------------------------------------------------------------------------
    def append_(self, x, y):
        x = _cols(x, self.dim)
        y = np.ascontiguousarray(np.atleast_1d(np.asarray(y, dtype=np.float64)))
        if x.shape[1] != y.size:
            raise ValueError("x and y disagree on the number of observations")
        rc = self._lib.bohip_gp_append(self._h, _ptr(x), _ptr(y), y.size)
        if rc in (_lib.OK, _lib.E_NOTPD):  # observations are stored even when the factorisation fails
            self._x = np.asfortranarray(np.concatenate([self._x, x], axis=1))
            self._y = np.concatenate([self._y, y])
            self._reps = np.concatenate([self._reps, np.ones(y.size, dtype=np.int64)])
            self._ymax = np.concatenate([self._ymax, y])
        check(rc)
        return self

    def append_sites_(self, x, ybar, reps, ss, ymax=None):
        """Append weighted sites (bohip_gp_append_sites): column j of x with the mean ybar[j] of its reps[j] evaluations and their
        within-site sum of squares ss[j]; ymax[j] is the largest of them (default: ybar, right for reps = 1 only), kept for maxy.
        collapse_evaluations makes all five from raw columns.  All reps = 1 on an unweighted model is append_."""
        x = _cols(x, self.dim)
        ybar = np.ascontiguousarray(np.atleast_1d(np.asarray(ybar, dtype=np.float64)))
        reps = np.ascontiguousarray(np.atleast_1d(np.asarray(reps)).astype(np.int64))
        ss = np.ascontiguousarray(np.atleast_1d(np.asarray(ss, dtype=np.float64)))
        ymax = ybar.copy() if ymax is None else np.ascontiguousarray(np.atleast_1d(np.asarray(ymax, dtype=np.float64)))
        if not (x.shape[1] == ybar.size == reps.size == ss.size == ymax.size):
            raise ValueError("x, ybar, reps, ss and ymax disagree on the number of sites")
        rc = self._lib.bohip_gp_append_sites(self._h, _ptr(x), _ptr(ybar), reps.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(ss), ybar.size)
        if rc in (_lib.OK, _lib.E_NOTPD):
            self._x = np.asfortranarray(np.concatenate([self._x, x], axis=1))
            self._y = np.concatenate([self._y, ybar])
            self._reps = np.concatenate([self._reps, reps])
            self._ymax = np.concatenate([self._ymax, ymax])
        check(rc)
        return self

    def fit_(self):
        check(self._lib.bohip_gp_refit(self._h))
        return self

    def mll(self):
        out = C.c_double()
        check(self._lib.bohip_gp_mll(self._h, C.byref(out)))
        return out.value

    def mll_grad(self):
        """(mll, dlogNoise, dmean, dkern) -- gp.target / gp.dtarget after update_target_and_dtarget!
        (reference src/models/gp.jl:61-63); dkern = [dll..., dlsigma] in the kernel's parameter order."""
        nk = (1 if self.kernel.iso else self.dim) + 1
        m, dn, dm = C.c_double(), C.c_double(), C.c_double()
        dk = np.empty(nk)
        check(self._lib.bohip_gp_mll_grad(self._h, C.byref(m), C.byref(dn), C.byref(dm), _ptr(dk)))
        return m.value, dn.value, dm.value, dk

    def mll_batch_dims(self):
        """(P, nmax): the row length of mll_grad_batch's Theta and the largest model its batched form takes."""
        P, nmax = C.c_int64(), C.c_int64()
        check(self._lib.bohip_gp_mll_batch_dims(self._h, C.byref(P), C.byref(nmax)))
        return int(P.value), int(nmax.value)

    def mll_grad_batch(self, Theta, want_grad=True):
        """The log marginal likelihood, and its gradient, at the H rows of Theta in ONE launch (bohip_gp_mll_grad_batch):
        row = [logNoise, mean, ll..., lsigma], GP.get_params order.  Returns (mll[H], G[H, P] or None, pivot[H]); a row whose
        factorisation fails has pivot > 0, mll = -inf and a zero gradient.  The model itself is neither read (beyond its
        observations) nor changed."""
        return _mll_grad_batch(self._lib, self._h, Theta, want_grad)

    def loo(self):
        """Leave-one-out cross-validation at the observations (bohip_gp_loo): LOO(mu, var, logp, total, z), the
        prediction of every noisy y_i from all the others, its log-probability, their sum and the standardised residuals
        z = (y - mu) / sqrt(var) of Jones, Schonlau & Welch 1998.  The model is not changed."""
        return _loo(self._lib, self._h, self._y)

    def loo_grad(self):
        """(total, dlogNoise, dmean, dkern): the LOO predictive log-probability and its gradient, in the slots of mll_grad
        (bohip_gp_loo_grad; Rasmussen & Williams 5.4.2)."""
        return _loo_grad(self._lib, self._h, (1 if self.kernel.iso else self.dim) + 1)

    def loo_grad_batch(self, Theta, want_grad=True, want_logp=False):
        """The LOO predictive log-probability, and its gradient, at the H rows of Theta in ONE launch (bohip_gp_loo_grad_batch,
        DESIGN.md 6s): rows as for mll_grad_batch.  Returns (total[H], G[H, P] or None, pivot[H]) and, with want_logp, the
        per-point logp[H, N] as a fourth value; a row whose factorisation fails has pivot > 0, total = -inf, a zero gradient and
        a NaN row of logp.  At most mll_batch_dims()[1] observations.  The model itself is neither read (beyond its
        observations) nor changed."""
        return _loo_grad_batch(self._lib, self._h, self.nobs, Theta, want_grad, want_logp)

    # -- predict_f / scoring ------------------------------------------------------------------------
    def predict_f(self, xs):
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        mu = np.empty(R)
        var = np.empty(R)
        check(self._lib.bohip_gp_predict(self._h, _ptr(xs), R, _ptr(mu), _ptr(var)))
        return mu, var

    def predict_cov(self, xs):
        """predict_f(gp, X; full_cov = true): (mu, R x R posterior covariance of the latent f)."""
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        mu = np.empty(R)
        cov = np.empty((R, R))
        check(self._lib.bohip_gp_predict_cov(self._h, _ptr(xs), R, _ptr(mu), _ptr(cov)))
        return mu, cov

    def score(self, acq, params, xs, want_scores=True):
        """Fused predict + acquisition + arg-max.  Returns (scores or None, best_val, best_idx)."""
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
        if p.size < 2:
            p = np.concatenate([p, np.zeros(2 - p.size)])
        sc = np.empty(R) if want_scores else None
        best = Best()
        check(self._lib.bohip_gp_score(self._h, _lib.ACQ[acq], _ptr(p), _ptr(xs), R,
                                       _ptr(sc) if want_scores else None, C.byref(best)))
        return sc, best.val, best.idx

    def score_ensemble(self, acq, params, xs, Theta, weights=None, want_each=False, want_moments=False):
        """The acquisition `acq` averaged over the H hyper-parameter settings in the rows of Theta (row = [logNoise, mean, ll...,
        lsigma], mll_grad_batch's layout): scores[j] = sum_h w~_h a(x_j; theta_h), the integrated acquisition of Snoek, Larochelle &
        Adams 2012 (an extension).  weights: H numbers >= 0 (None: equal), renormalised over the settings whose factorisation
        succeeds; a failed setting has pivot > 0 and NaN rows.  Returns an EnsembleScore; its `route` says what ran: "device"
        (bohip_gp_score_ens, include/bohip_ens.h: all settings in one call, the model neither read beyond its observations nor
        changed) up to mll_batch_dims()[1] observations, "host" above that (set_params_ + score / predict_f per row, the model's
        own parameters restored afterwards), with the same averaging rule.  Value only: no gradient."""
        refuse_weighted(self, "score_ensemble (Marginalised acquisitions)")
        return score_ensemble(self, acq, params, xs, Theta, weights, want_each, want_moments)

    def score_ensemble_grad(self, acq, params, xs, Theta, weights=None, want_each=False):
        """score_ensemble's scores together with their gradient with respect to every candidate: (EnsembleScore, grad[d, R]), and
        each_grad[H, d, R] with want_each (NaN rows for a failed setting).  "device": bohip_gp_score_ens_grad
        (include/bohip_ens_grad.h) -- scores, each and the arg-max are score_ensemble's bit for bit, and successive calls with the same
        Theta and unchanged observations factor the settings once (timing() then shows no "ens_factor"); "host" above
        mll_batch_dims()[1] observations: set_params_ + score_grad per row, the model's own parameters restored afterwards."""
        refuse_weighted(self, "score_ensemble_grad (Marginalised acquisitions)")
        return score_ensemble_grad(self, acq, params, xs, Theta, weights, want_each)

    def select_batch(self, acq, params, xs, q, fantasy="believer", raise_tau=False):
        """q candidates to evaluate in parallel (bohip_gp_select_batch; an extension, the reference proposes one point per
        iteration): greedy arg-max under the posterior conditioned on the fantasised observations of the earlier picks.
        fantasy: "believer" (y_f = mu(x_s)) or a number (constant liar).  raise_tau: EI / PI incumbent follows the fantasies.
        The model is not changed.  Returns (idx[q] int64, val[q], mu[q], var[q]); idx = -1, val = -Inf where nothing could win."""
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        q = int(q)
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
        if p.size < 2:
            p = np.concatenate([p, np.zeros(2 - p.size)])
        if isinstance(fantasy, str):
            if fantasy != "believer":
                raise ValueError(f"fantasy must be 'believer' or a number, got {fantasy!r}")
            mode, fv = _lib.FANTASY_BELIEVER, 0.0
        else:
            mode, fv = _lib.FANTASY_CONST, float(fantasy)
        n = max(q, 1)
        idx = np.full(n, -1, dtype=np.int64)
        val, mu, var = np.empty(n), np.empty(n), np.empty(n)
        check(self._lib.bohip_gp_select_batch(self._h, _lib.ACQ[acq], _ptr(p), _ptr(xs), R, q, mode, fv,
                                              _lib.BATCH_RAISE_TAU if raise_tau else 0,
                                              idx.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(val), _ptr(mu), _ptr(var)))
        return idx, val, mu, var

    # -- pending evaluations (include/bohip_pend.h) ----------------------------------------------------------------
    def set_pending(self, xp):
        """The points that are out for evaluation and not back yet (d x p, p <= 32; an empty array clears the set).  Replaces the
        model's pending set (bohip_gp_pending_set); nothing is computed until score_pending or pending_info reads it.  Every other
        method ignores the set."""
        if self.collapse:
            raise ValueError("pending evaluations do not support a model with collapse=True (replicated sites)")
        refuse_weighted(self, "set_pending (pending evaluations)")
        xp = np.zeros((self.dim, 0), order="F") if xp is None or np.size(xp) == 0 else _cols(xp, self.dim)
        check(self._lib.bohip_gp_pending_set(self._h, _ptr(xp) if xp.shape[1] else None, xp.shape[1]))
        self._pending = xp.copy(order="F")
        return self

    def clear_pending(self):
        return self.set_pending(None)

    @property
    def pending(self):
        """A copy of the pending set, d x p."""
        return getattr(self, "_pending", np.zeros((self.dim, 0), order="F")).copy(order="F")

    def pending_info(self):
        """(Xp [d, p], mu_p [p], Sigma_p [p, p]): the pending set with the model's predictive mean and covariance of the NOISY
        outcomes there (bohip_gp_pending_info; nu on the diagonal).  Brings the model and the derived state up to date."""
        p = C.c_int64()
        check(self._lib.bohip_gp_pending_info(self._h, C.byref(p), None, None, None))
        p = int(p.value)
        xp, mu, cov = np.zeros((self.dim, p), order="F"), np.empty(p), np.empty((p, p))
        if p:
            check(self._lib.bohip_gp_pending_info(self._h, None, _ptr(xp), _ptr(mu), _ptr(cov)))
        return xp, mu, cov

    def score_pending(self, acq, params, xs, fantasies=0, seed=0, raise_tau=False, want_scores=True):
        """The acquisition `acq` averaged over `fantasies` fantasised outcomes at the pending points (bohip_gp_score_pending; Snoek,
        Larochelle & Adams 2012, section 3.2).  fantasies = 0: the Kriging believer (the mean stays, the variance shrinks).
        raise_tau: the incumbent of EI / PI / LogEI follows each fantasy.  With an empty pending set it is `score`.  Returns
        PendingScore(scores, mu, var, best_val, best_idx): mu the model's mean, var the variance conditioned on the pending points.
        The model is not changed."""
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
        if p.size < 2:
            p = np.concatenate([p, np.zeros(2 - p.size)])
        sc = np.empty(R) if want_scores else None
        mu, var = np.empty(R), np.empty(R)
        best = Best()
        check(self._lib.bohip_gp_score_pending(self._h, _lib.ACQ[acq], _ptr(p), _ptr(xs), R, int(fantasies), int(seed),
                                               _lib.PEND_RAISE_TAU if raise_tau else 0, _ptr(sc) if want_scores else None, _ptr(mu),
                                               _ptr(var), C.byref(best)))
        return PendingScore(sc, mu, var, best.val, best.idx)

    def pend_values(self, acq, params, mu, var, B, Z, tau_s=None):
        """The averaging stage on its own, from host arrays (bohip_pend_values): mu, var [R], B [R, p], Z [S, p], tau_s [S] or None.
        Returns (scores[R], best_val, best_idx)."""
        mu, var = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64) for a in (mu, var))
        B, Z = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (B, Z))
        R, pp, S = mu.size, Z.shape[1], Z.shape[0]
        if var.size != R or B.shape != (R, pp):
            raise ValueError("mu, var [R], B [R, p] and Z [S, p] disagree")
        tau = None if tau_s is None else np.ascontiguousarray(np.atleast_1d(tau_s), dtype=np.float64)
        if tau is not None and tau.size != S:
            raise ValueError("tau_s must have one value per fantasy")
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
        if p.size < 2:
            p = np.concatenate([p, np.zeros(2 - p.size)])
        sc = np.empty(R)
        best = Best()
        check(self._lib.bohip_pend_values(self._h, _lib.ACQ[acq], _ptr(p), R, pp, S, _ptr(mu), _ptr(var), _ptr(B), _ptr(Z),
                                          _ptr(tau) if tau is not None else None, _ptr(sc), C.byref(best)))
        return sc, best.val, best.idx

    # -- noisy expected improvement (include/bohip_nei.h) -------------------------------------------------------------
    def nei(self, X, S=32, seed=0, acq="ei", jitter_rel=1e-8, want_scores=True):
        """Noisy expected improvement at the columns of X (bohip_gp_score_nei; Letham, Karrer, Ottoni & Bakshy 2019, eq. 6): `acq`
        ("ei", "pi" or "logei") averaged over S posterior draws of the NOISE-FREE function values at the observed sites, each with
        its own incumbent tau_s and its own noise-free conditional mean.  S = 0: the plug-in form, the incumbent is the largest
        posterior mean at the sites.  Returns NEIScore(score, mu, var, best, tau): mu the mean over the draws of m_s, var the shared
        noise-free variance, best = (value, index), tau the S incumbents.  The model is not changed."""
        return _nei(self._lib, self._h, _cols(X, self.dim), S, seed, acq, jitter_rel, want_scores)

    def nei_fantasies(self, S=32, seed=0, jitter_rel=1e-8):
        """(F [max(S, 1), n], tau [max(S, 1)]): the fantasised noise-free function values at the observed sites, row s = f_s, and
        their maxima (bohip_gp_nei_fantasies).  Brings the model, its noise-free companion and the fantasies up to date."""
        return _nei_fantasies(self._lib, self._h, self.nobs, S, seed, jitter_rel)

    def nei_prepare(self, S=32, seed=0, jitter_rel=1e-8):
        check(self._lib.bohip_gp_nei_prepare(self._h, float(jitter_rel), int(S), int(seed)))
        return self

    def nei_values(self, acq, mu_s, var, tau_s):
        """The averaging stage on its own, from host arrays (bohip_nei_values): mu_s [R, S], var [R], tau_s [S].
        Returns (scores[R], mean over s of mu_s [R], best_val, best_idx)."""
        mu_s = np.ascontiguousarray(np.atleast_2d(mu_s), dtype=np.float64)
        var, tau_s = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64) for a in (var, tau_s))
        R, S = mu_s.shape
        if var.size != R or tau_s.size != S:
            raise ValueError("mu_s [R, S], var [R] and tau_s [S] disagree")
        sc, mm = np.empty(R), np.empty(R)
        best = Best()
        check(self._lib.bohip_nei_values(self._h, _lib.ACQ[_NEI_ACQ[str(acq).lower()]], R, S, _ptr(mu_s), _ptr(var), _ptr(tau_s), _ptr(sc),
                                         _ptr(mm), C.byref(best)))
        return sc, mm, best.val, best.idx

    def nei_info(self, what):
        """bohip_gp_nei_info: a _lib.NEI_INFO_* quantity (counts come back as int, the delta in force as float)."""
        v = C.c_double()
        check(self._lib.bohip_gp_nei_info(self._h, int(what), C.byref(v)))
        return v.value if what == _lib.NEI_INFO_DELTA else int(v.value)

    def nei_release(self):
        check(self._lib.bohip_gp_nei_release(self._h))
        return self

    def score_grad(self, acq, params, xs):
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
        if p.size < 2:
            p = np.concatenate([p, np.zeros(2 - p.size)])
        sc = np.empty(R)
        grad = np.empty((self.dim, R), order="F")
        check(self._lib.bohip_gp_score_grad(self._h, _lib.ACQ[acq], _ptr(p), _ptr(xs), R, _ptr(sc), _ptr(grad)))
        return sc, grad

    def set_maxtime(self, seconds):
        """NLopt's maxtime for the device ascent (0 = unlimited)."""
        check(self._lib.bohip_gp_set_maxtime(self._h, float(seconds)))

    def set_ascent_stop(self, ftol_abs=0.0, xtol_rel=0.0, stopval=float("inf")):
        """NLopt's ftol_abs / xtol_rel / stopval for the device ascent (0 / 0 / +Inf = off), reference src/acquisition.jl:24-27."""
        check(self._lib.bohip_gp_set_ascent_stop(self._h, float(ftol_abs), float(xtol_rel), float(stopval)))

    def set_jitter(self, rel, max_tries=10):
        """Jitter escalation on a failed factorisation (the role of GaussianProcesses.jl's make_posdef! behind update!,
        src/models/gp.jl:11,16 -- UPSTREAM-UNVERIFIED, off by default): a refit that fails is repeated with
        rel x mean(diag cK) more on the diagonal, x10 per further try; info(INFO_JITTER_STEPS) tells how many it took."""
        check(self._lib.bohip_gp_set_jitter(self._h, float(rel), int(max_tries)))

    def ascend(self, acq, params, lowerbounds, upperbounds, starts, maxeval=2000, ftol_rel=1e-10, xtol_abs=1e-10):
        """Local search of acquire_max on the device (src/acquisition.jl:48-68 with :LD_LBFGS and bounds): every start
        column is refined by a projected L-BFGS ascent, all columns in the same device passes.  Returns
        (f[R], X[d, R], best_f, best_index, best_x[d], evaluations)."""
        starts = _cols(starts, self.dim)
        R = starts.shape[1]
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
        if p.size < 2:
            p = np.concatenate([p, np.zeros(2 - p.size)])
        lb = np.ascontiguousarray(lowerbounds, dtype=np.float64)
        ub = np.ascontiguousarray(upperbounds, dtype=np.float64)
        if lb.size != self.dim or ub.size != self.dim:
            raise ValueError("bounds must have one entry per input dimension")
        f = np.empty(R)
        X = np.empty((self.dim, R), order="F")
        best = Best()
        bx = np.empty(self.dim)
        ev = C.c_int64(0)
        check(self._lib.bohip_gp_acquire_max(self._h, _lib.ACQ[acq], _ptr(p), _ptr(lb), _ptr(ub), _ptr(starts), R, int(maxeval),
                                             float(ftol_rel), float(xtol_abs), _ptr(X), _ptr(f), C.byref(best), _ptr(bx),
                                             C.byref(ev)))
        return f, X, best.val, best.idx, bx, ev.value

    # -- one process per device: communicator on the handle, exchange inside libbohip (in-library RCCL) ---------
    def comm_init(self, unique_id, rank, nranks):
        buf = C.create_string_buffer(bytes(unique_id), _lib.UNIQUE_ID_BYTES)
        check(self._lib.bohip_gp_comm_init(self._h, buf, _lib.UNIQUE_ID_BYTES, int(rank), int(nranks)))

    def comm_destroy(self):
        check(self._lib.bohip_gp_comm_destroy(self._h))

    def score_sharded_dev(self, acq, params, d_xs_ptr, R_local, col_offset, R_total, d_best_ptr, d_score_ptr=None):
        """Enqueue: score this rank's shard, all-gather the records over RCCL, reduce on the device; the global winner
        lands at d_best_ptr (device or pinned-host address), identical on every rank.  No host synchronisation."""
        p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
        if p.size < 2:
            p = np.concatenate([p, np.zeros(2 - p.size)])
        check(self._lib.bohip_gp_score_sharded_dev(self._h, _lib.ACQ[acq], _ptr(p), C.c_void_p(d_xs_ptr), int(R_local),
                                                   int(col_offset), int(R_total),
                                                   C.c_void_p(d_score_ptr) if d_score_ptr else None, C.c_void_p(d_best_ptr)))

    def thompson_sharded(self, xs, S, seed, col_offset, R_total):
        xs = _cols(xs, self.dim)
        out = (Best * S)()
        check(self._lib.bohip_gp_thompson_sharded(self._h, _ptr(xs), xs.shape[1], S, seed, int(col_offset), int(R_total), out))
        return np.array([b.val for b in out]), np.array([b.idx for b in out], dtype=np.int64)

    def synchronize(self):
        check(self._lib.bohip_gp_synchronize(self._h))

    def direct_max(self, acq, params, lowerbounds, upperbounds, maxeval=2000, stopval=float("inf"), maxtime=0.0, seed=0):
        """:GN_DIRECT_L on the device model in one call (bohip_gp_direct_max; reference src/acquisition.jl:7-9, :20-38): the
        dividing-rectangles bookkeeping runs in the library, every iteration's points are one scoring call.  acq = "ThompsonDraw":
        x -> myrand(model, x), one posterior draw per point from the library's counter-based generator keyed by `seed`.
        Returns (best value, best point, evaluations, device calls)."""
        lb = np.ascontiguousarray(lowerbounds, dtype=np.float64)
        ub = np.ascontiguousarray(upperbounds, dtype=np.float64)
        if lb.size != self.dim or ub.size != self.dim:
            raise ValueError("bounds must have one entry per input dimension")
        p = np.zeros(2)
        if params is not None:
            q = np.atleast_1d(np.asarray(params, dtype=np.float64))
            p[:q.size] = q[:2]
        bf = C.c_double(); bx = np.empty(self.dim); ev = C.c_int64(); dc = C.c_int64()
        check(self._lib.bohip_gp_direct_max(self._h, _lib.ACQ[acq], _ptr(p), _ptr(lb), _ptr(ub), int(maxeval), float(stopval),
                                            float(maxtime or 0.0), int(seed), C.byref(bf), _ptr(bx), C.byref(ev), C.byref(dc)))
        return float(bf.value), bx, int(ev.value), int(dc.value)

    def thompson(self, xs, S, seed=0, j0=0):
        xs = _cols(xs, self.dim)
        out = (Best * S)()
        check(self._lib.bohip_gp_thompson(self._h, _ptr(xs), xs.shape[1], S, seed, j0, out))
        return np.array([b.val for b in out]), np.array([b.idx for b in out], dtype=np.int64)

    def sample_joint(self, xs, S=1, seed=0, jitter=1e-12, max_tries=40, want_samples=True, want_factor=False):
        """S JOINT draws of the posterior over the columns of xs on the device (bohip_gp_sample_joint; reference
        myrand(model, X::Matrix), src/models/gp.jl:7): f_s = mu + C z_s, C C' = Sigma + jitter I, z from the library's counter-based
        generator keyed (seed, s, j).  `thompson` draws every candidate independently; this is the draw whose arg-max is a draw of
        the maximiser.  Only what is asked for crosses to the host.  Returns a JointSample."""
        return _sample_joint(self._lib, self._h, _cols(xs, self.dim), S, seed, jitter, max_tries, want_samples, want_factor)

    def qei_batch(self, xs, q, S=256, seed=0, tau=None, jitter=1e-12, max_tries=40, want_samples=False):
        """Greedy Monte-Carlo q-EI batch over the columns of xs (bohip_gp_qei_batch, include/bohip_qei.h; an extension, as
        select_batch is): sample_joint's S draws for the same (xs, S, seed, jitter rule) stay on the device and q rounds pick the
        candidate with the largest sample-average gain E[max(max_B f - tau, 0)] over the batch so far.  tau defaults to maxy.
        With q = 1 this estimates the TEXTBOOK EI (Delta Phi(z) + sigma phi(z)), not the reference's ExpectedImprovement functor
        (Delta Phi(z) + phi(z)).  The model is not changed.  Returns a QEIBatch; idx = -1, gain = 0 where nothing could win."""
        if tau is None:
            tau = maxy(self)
        return _qei_batch(self._lib, self._h, _cols(xs, self.dim), q, S, seed, tau, jitter, max_tries, want_samples)

    def qei_select(self, samples, tau, q):
        """The selection of qei_batch alone on the caller's S x R sample matrix (bohip_gp_qei_select): the model supplies the
        device and the stream only.  Returns (idx[q] int64, gain[q])."""
        return _qei_select(self._lib, self._h, samples, tau, q)

    def kg(self, xs, n_eval=None):
        """The knowledge gradient of the first n_eval columns of xs (default: all) over the candidate set xs, exact, on the device
        (bohip_gp_kg, include/bohip_kg.h; an extension): KG(e) = E[max_j mu'_j] - max_j mu_j, the expected rise of the maximum of the
        posterior mean over the candidates after ONE noisy observation at x_e.  The posterior covariance stays on the device; the
        model is not changed.  Returns a KGResult."""
        return _kg(self._lib, self._h, _cols(xs, self.dim), n_eval)

    def kg_lines(self, a, B):
        """The march of kg alone on the caller's lines (bohip_kg_lines): a[R] intercepts, B E x R slopes, one evaluation point per
        row.  The model supplies the device and the stream only.  Returns (values[E], nseg[E] int32)."""
        return _kg_lines(self._lib, self._h, a, B)

    def mes(self, xs, samples=16, mode="gumbel", seed=0, floor=None, jitter_rel=1e-12, max_tries=40):
        """Max-value entropy search over the candidate set xs on the device (bohip_gp_mes, include/bohip_mes.h; an extension; Wang &
        Jegelka 2017): MES_j = mean_k u(mu_j, s2_j, m_k) over `samples` draws m_k of the maximum of the posterior over the
        candidates.  mode "gumbel": a Gumbel fit to three quantiles of the maximum of independent candidates (any R up to
        _lib.MES_RMAX); "joint": the row maxima of sample_joint's draws for the same (xs, S = samples, seed, jitter rule), R
        within one chunk.  floor (None: none) is a lower limit of every max value, e.g. the best observation.  The model is not
        changed.  Returns a MESResult."""
        return _mes(self._lib, self._h, _cols(xs, self.dim), samples, mode, seed, floor, jitter_rel, max_tries)

    def mes_values(self, mu, var, maxvals, want_grad=False):
        """The functor of mes alone on the caller's (mu, var, maxvals) (bohip_mes_values): the model supplies the device and the
        stream only.  Returns (values[R], best_val, best_idx), or (values, dmu, dvar, best_val, best_idx) with want_grad."""
        return _mes_values(self._lib, self._h, mu, var, maxvals, want_grad)

    def predict_grad(self, xs):
        """The posterior and its own Jacobians in x (bohip_gp_predict_grad, include/bohip_con.h): (mu[R], var[R], dmu[d, R],
        dvar[d, R]), dmu = grad mu, dvar = grad sigma^2 reported unmasked (where var == 0 the clamp is the caller's).  An extension:
        what a score over several models (ConstrainedGPE) is differentiated through."""
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        mu, var = np.empty(max(R, 1)), np.empty(max(R, 1))
        dmu, dvar = np.empty((self.dim, max(R, 1)), order="F"), np.empty((self.dim, max(R, 1)), order="F")
        check(self._lib.bohip_gp_predict_grad(self._h, _ptr(xs), R, _ptr(mu), _ptr(var), _ptr(dmu), _ptr(dvar)))
        return mu[:R], var[:R], dmu[:, :R], dvar[:, :R]

    def con_values(self, acq, params, thresholds, senses, mu, var, want_grad=False):
        """The combine stage of a constrained score alone, on the caller's moments (bohip_con_values); see con_values."""
        return con_values(self, acq, params, thresholds, senses, mu, var, want_grad)

    def mes_gumbel(self, mu, var, samples=16, seed=0, floor=None):
        """The max-value sampler of mode "gumbel" alone on the caller's (mu, var) (bohip_mes_gumbel).  Returns (quantiles[3],
        maxvals[samples])."""
        return _mes_gumbel(self._lib, self._h, mu, var, samples, seed, floor)

    def draw_paths(self, S=1, M=2048, seed=0):
        """S posterior SAMPLE PATHS (bohip_gp_paths_draw): draws that are functions, f_s(x) = beta + sum_m w_sm phi_m(x) +
        sum_j u_sj k(x, X_j) with M random features for the prior term and the exact data term (pathwise conditioning).  The result
        can be evaluated and differentiated anywhere afterwards and does not follow later changes of the model.  Close it (or use it
        as a context manager) before the model is closed.  Returns a PosteriorPaths."""
        refuse_weighted(self, "draw_paths (and the \"pathwise\" options that use it)")
        p = PosteriorPaths(self._lib, self._h, self.dim, S, M, seed)
        if not hasattr(self, "_paths"):
            self._paths = weakref.WeakSet()
        self._paths.add(p)
        return p

    # -- introspection ------------------------------------------------------------------------------
    def factor(self):
        n = self.nobs
        L = np.zeros((n, n))
        check(self._lib.bohip_gp_get_factor(self._h, _ptr(L)))
        return L

    def alpha(self):
        a = np.zeros(self.nobs)
        check(self._lib.bohip_gp_get_alpha(self._h, _ptr(a)))
        return a

    def info(self, what):
        v = C.c_int64()
        check(self._lib.bohip_gp_info(self._h, what, C.byref(v)))
        return v.value

    def set_batch_hint(self, total_candidates):
        """Score shards of a larger candidate set with the summation schedule of the whole set (bit-identical to the
        unsharded call); 0 clears the hint."""
        check(self._lib.bohip_gp_set_batch_hint(self._h, int(total_candidates)))

    def enable_timing(self, on=True):     # True/1: every stage; 2: only the dominant kernel; 3: as 2, read after the loop
        check(self._lib.bohip_gp_enable_timing(self._h, int(on)))

    def timing(self, cap=64):
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        n = self._lib.bohip_gp_get_timing(self._h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(min(n, cap))]

    def __repr__(self):
        return (f"ElasticGPE(dim={self.dim}, nobs={self.nobs}, kernel={self.kernel.kern}"
                f"(ll={self.kernel.ll.tolist()}, lσ={self.kernel.lsigma}), mean β={self.mean.beta}, "
                f"logNoise={self.logNoise}) [device-resident, libbohip]")


def _mll_grad_batch(lib, h, Theta, want_grad):
    P, nmax = C.c_int64(), C.c_int64()
    check(lib.bohip_gp_mll_batch_dims(h, C.byref(P), C.byref(nmax)))
    Theta = np.ascontiguousarray(np.atleast_2d(np.asarray(Theta, dtype=np.float64)))
    if Theta.shape[1] != P.value:
        raise ValueError(f"Theta must have {P.value} columns [logNoise, mean, ll..., lsigma], got {Theta.shape[1]}")
    H = Theta.shape[0]
    mll = np.empty(H)
    G = np.empty((H, P.value)) if want_grad else None
    pivot = np.zeros(H, dtype=np.int64)
    check(lib.bohip_gp_mll_grad_batch(h, H, _ptr(Theta), _ptr(mll), _ptr(G) if want_grad else None,
                                      pivot.ctypes.data_as(C.POINTER(C.c_int64))))
    return mll, G, pivot


class PendingScore:
    """score_pending's result: scores [R] (None without want_scores), mu [R] the model's mean, var [R] the variance conditioned on
    the pending points, and the arg-max record."""
    __slots__ = ("scores", "mu", "var", "best_val", "best_idx")

    def __init__(self, scores, mu, var, best_val, best_idx):
        self.scores, self.mu, self.var, self.best_val, self.best_idx = scores, mu, var, float(best_val), int(best_idx)

    def __iter__(self):
        return iter((self.scores, self.mu, self.var, self.best_val, self.best_idx))


_NEI_ACQ = {"ei": "EI", "pi": "PI", "logei": "LogEI"}


class NEIScore:
    """nei's result: score [R] (None without want_scores), mu [R] the mean over the fantasies of m_s, var [R] the noise-free variance,
    best = (value, index) of the arg-max and tau [max(S, 1)] the fantasies' incumbents."""
    __slots__ = ("score", "mu", "var", "best", "tau")

    def __init__(self, score, mu, var, best, tau):
        self.score, self.mu, self.var, self.best, self.tau = score, mu, var, (float(best[0]), int(best[1])), tau

    def __iter__(self):
        return iter((self.score, self.mu, self.var, self.best, self.tau))


def _nei(lib, h, xs, S, seed, acq, jitter_rel, want_scores=True):
    R = xs.shape[1]
    name = _NEI_ACQ[str(acq).lower()]
    sc = np.empty(R) if want_scores else None
    mu, var = np.empty(R), np.empty(R)
    best = Best()
    tau = np.empty(max(int(S), 1))
    check(lib.bohip_gp_nei_fantasies(h, float(jitter_rel), int(S), int(seed), None, _ptr(tau)))   # (kept: the score call rebuilds nothing)
    check(lib.bohip_gp_score_nei(h, _lib.ACQ[name], None, _ptr(xs), R, int(S), int(seed), float(jitter_rel),
                                 _ptr(sc) if want_scores else None, _ptr(mu), _ptr(var), C.byref(best)))
    return NEIScore(sc, mu, var, (best.val, best.idx), tau)


def _nei_fantasies(lib, h, n, S, seed, jitter_rel):
    S1 = max(int(S), 1)
    F, tau = np.empty((S1, n)), np.empty(S1)
    check(lib.bohip_gp_nei_fantasies(h, float(jitter_rel), int(S), int(seed), _ptr(F), _ptr(tau)))
    return F, tau


class LOO:
    """Result of loo(): mu[n], var[n] (the leave-one-out prediction of each noisy observation from the others, mu in the sign the
    model stores y), logp[n] (its log-probability), total (their sum) and z[n] = (y - mu) / sqrt(var), the standardised residuals."""
    __slots__ = ("mu", "var", "logp", "total", "z")

    def __init__(self, mu, var, logp, total, z):
        self.mu, self.var, self.logp, self.total, self.z = mu, var, logp, total, z

    def __iter__(self):
        return iter((self.mu, self.var, self.logp, self.total, self.z))


def _loo(lib, h, y):
    n = y.size
    mu, var, logp, total = np.empty(n), np.empty(n), np.empty(n), C.c_double()
    check(lib.bohip_gp_loo(h, _ptr(mu), _ptr(var), _ptr(logp), C.byref(total)))
    return LOO(mu, var, logp, total.value, (y - mu) / np.sqrt(var))


def _loo_grad(lib, h, nk):
    t, dn, dm = C.c_double(), C.c_double(), C.c_double()
    dk = np.empty(nk)
    check(lib.bohip_gp_loo_grad(h, C.byref(t), C.byref(dn), C.byref(dm), _ptr(dk)))
    return t.value, dn.value, dm.value, dk


def _loo_grad_batch(lib, h, n, Theta, want_grad, want_logp):
    P, nmax = C.c_int64(), C.c_int64()
    check(lib.bohip_gp_mll_batch_dims(h, C.byref(P), C.byref(nmax)))
    Theta = np.ascontiguousarray(np.atleast_2d(np.asarray(Theta, dtype=np.float64)))
    if Theta.shape[1] != P.value:
        raise ValueError(f"Theta must have {P.value} columns [logNoise, mean, ll..., lsigma], got {Theta.shape[1]}")
    H = Theta.shape[0]
    total = np.empty(H)
    G = np.empty((H, P.value)) if want_grad else None
    logp = np.empty((H, n)) if want_logp else None
    pivot = np.zeros(H, dtype=np.int64)
    check(lib.bohip_gp_loo_grad_batch(h, H, _ptr(Theta), _ptr(total), _ptr(G) if want_grad else None, _ptr(logp) if want_logp else None,
                                      pivot.ctypes.data_as(C.POINTER(C.c_int64))))
    return (total, G, pivot, logp) if want_logp else (total, G, pivot)


class EnsembleScore:
    """Result of score_ensemble: scores[R] (the weighted average over the surviving settings), best_val / best_idx (its arg-max
    under score's rule: first maximum, NaN never wins, -Inf / -1 if nothing can win), pivot[H] (int64: 0, or the 1-based pivot at
    which the setting's factorisation failed), each (H x R per-setting scores, or None), mu / var (H x R each, or None), route
    ("device": bohip_gp_score_ens; "host": one refit per setting)."""
    __slots__ = ("scores", "best_val", "best_idx", "pivot", "each", "mu", "var", "route")

    def __init__(self, scores, best_val, best_idx, pivot, each, mu, var, route):
        self.scores, self.best_val, self.best_idx, self.pivot = scores, best_val, best_idx, pivot
        self.each, self.mu, self.var, self.route = each, mu, var, route

    def __iter__(self):
        return iter((self.scores, self.best_val, self.best_idx, self.pivot, self.each, self.mu, self.var))


def ensemble_average(each, weights, pivot):
    """The averaging rule of score_ensemble, both routes: w~ = w / (sum of w over the settings with pivot 0, ascending h), then
    scores = sum_h w~_h each[h], added in ascending h from 0.0; failed settings and settings of weight 0 take no part."""
    each = np.asarray(each, dtype=np.float64)
    H, R = each.shape
    w = np.ones(H) if weights is None else np.asarray(weights, dtype=np.float64)
    total = 0.0
    for h in range(H):
        if pivot[h] == 0:
            total += w[h]
    scores = np.zeros(R)
    for h in range(H):
        wt = w[h] / total if pivot[h] == 0 else 0.0
        if wt != 0.0:
            scores = scores + wt * each[h]
    return scores


def _ens_weights(weights, H):
    if weights is None:
        return None
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel())
    if w.size != H:
        raise ValueError(f"weights must have one entry per row of Theta ({H}), got {w.size}")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0.0) and w.sum() > 0.0):
        raise ValueError("weights must be finite, >= 0 and not all 0")
    return w


def _opt(a):
    return _ptr(a) if a is not None else None


def _ens_prologue(model, who, symbol, acq, params, xs, Theta, weights):
    """What score_ensemble and score_ensemble_grad (`who`; `symbol` its device route) check and shape alike
    -> (xs[d, R], Theta[H, P], w[H] or None, p, pivot[H] of zeros, lib, h); lib is None where the host route has to run: no handle, a
    library without the symbol, or more than nmax observations."""
    if acq not in _lib.ACQ or acq == "ThompsonDraw":
        raise ValueError(f"{who} takes EI, PI, UCB, MI, MaxMean and LogEI, not {acq!r}")
    xs = _cols(xs, model.dim)
    P = 2 + (1 if model.kernel.iso else model.dim) + 1
    Theta = np.ascontiguousarray(np.atleast_2d(np.asarray(Theta, dtype=np.float64)))
    if Theta.shape[1] != P:
        raise ValueError(f"Theta must have {P} columns [logNoise, mean, ll..., lsigma], got {Theta.shape[1]}")
    w = _ens_weights(weights, Theta.shape[0])
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)))
    if p.size < 2:
        p = np.concatenate([p, np.zeros(2 - p.size)])
    lib, h = getattr(model, "_lib", None), getattr(model, "_h", None)
    device = lib is not None and h and hasattr(lib, symbol) and model.nobs <= _lib.FIT_NMAX
    return xs, Theta, w, p, np.zeros(Theta.shape[0], dtype=np.int64), (lib if device else None), h


def _ens_host_route(model, Theta, w, pivot, planes, evaluate):
    """The host route of both: one refit per setting, the model's own parameters put back whatever happens.  `planes` are NaN-filled
    arrays [H, ...], planes[0] the per-setting scores; evaluate() gives one row for each of them at the model's current parameters.  A
    setting that is not finite or whose factorisation fails keeps NaN rows and gets its pivot.  -> (scores, best_val, best_idx)."""
    H, nl = Theta.shape[0], Theta.shape[1] - 3
    saved = (model.kernel.ll.copy(), model.kernel.lsigma, model.logNoise, model.mean)
    try:
        for k in range(H):
            row = Theta[k]
            if not np.all(np.isfinite(row)):
                pivot[k] = 1
                continue
            try:
                model.set_params_(ll=row[2:2 + nl], lsigma=row[2 + nl], logNoise=row[0], beta=row[1])
                for plane, value in zip(planes, evaluate()):
                    plane[k] = value
            except _lib.NotPositiveDefinite:
                piv = model.info(_lib.INFO_PIVOT) if hasattr(model, "info") else 1
                pivot[k] = max(int(piv), 1)
                for plane in planes:
                    plane[k] = np.nan
    finally:
        model.set_params_(ll=saved[0], lsigma=saved[1], logNoise=saved[2], beta=saved[3].beta)
        model.mean = saved[3]
    if not np.any((pivot == 0) & ((w if w is not None else np.ones(H)) > 0.0)):
        raise _lib.NotPositiveDefinite(_lib.E_NOTPD, "the factorisation failed at every hyper-parameter setting")
    scores = ensemble_average(planes[0], w, pivot)
    best_val, best_idx = -math.inf, -1
    for j, v in enumerate(scores):
        if v > best_val:
            best_val, best_idx = float(v), j
    return scores, best_val, best_idx


def score_ensemble(model, acq, params, xs, Theta, weights=None, want_each=False, want_moments=False):
    """ElasticGPE.score_ensemble for any model object: the device route where the model owns a handle whose library has
    bohip_gp_score_ens and holds at most nmax observations, else the host loop over set_params_ + score / predict_f."""
    xs, Theta, w, p, pivot, lib, h = _ens_prologue(model, "score_ensemble", "bohip_gp_score_ens", acq, params, xs, Theta, weights)
    H, R = Theta.shape[0], xs.shape[1]
    if lib is not None:
        scores = np.empty(R)
        each = np.empty((H, R)) if want_each else None
        mu = np.empty((H, R)) if want_moments else None
        var = np.empty((H, R)) if want_moments else None
        best = Best()
        check(lib.bohip_gp_score_ens(h, _lib.ACQ[acq], _ptr(p), H, _ptr(Theta), _opt(w), _ptr(xs), R, _ptr(scores), _opt(each), _opt(mu),
                                     _opt(var), pivot.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(best)))
        return EnsembleScore(scores, best.val, best.idx, pivot, each, mu, var, "device")
    each = np.full((H, R), np.nan)
    mu, var = (np.full((H, R), np.nan), np.full((H, R), np.nan)) if want_moments else (None, None)
    scores, best_val, best_idx = _ens_host_route(
        model, Theta, w, pivot, [each, mu, var] if want_moments else [each],
        lambda: (model.score(acq, p, xs)[0],) + (tuple(model.predict_f(xs)) if want_moments else ()))
    return EnsembleScore(scores, best_val, best_idx, pivot, each if want_each else None, mu, var, "host")


def score_ensemble_grad(model, acq, params, xs, Theta, weights=None, want_each=False):
    """ElasticGPE.score_ensemble_grad for any model object: (EnsembleScore, grad[d, R]) -- and each_grad[H, d, R] with want_each --
    of the acquisition averaged over the rows of Theta.  The device route (bohip_gp_score_ens_grad, include/bohip_ens_grad.h) where
    the model owns a handle whose library has the symbol and holds at most nmax observations; else the host loop over set_params_ +
    score_grad, the model's own parameters put back whatever happens.  Both average each gradient component by ensemble_average's
    rule; a failed setting has NaN rows and takes no part."""
    xs, Theta, w, p, pivot, lib, h = _ens_prologue(model, "score_ensemble_grad", "bohip_gp_score_ens_grad", acq, params, xs, Theta, weights)
    H, R, d = Theta.shape[0], xs.shape[1], model.dim
    if lib is not None:
        scores = np.empty(R)
        grad = np.empty((d, R), order="F")                        # (the library's [R][d] row-major)
        each = np.empty((H, R)) if want_each else None
        eg = np.empty((H, R, d)) if want_each else None
        best = Best()
        check(lib.bohip_gp_score_ens_grad(h, _lib.ACQ[acq], _ptr(p), H, _ptr(Theta), _opt(w), _ptr(xs), R, _ptr(scores), _ptr(grad), _opt(each),
                                          _opt(eg), None, None, pivot.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(best)))
        res = EnsembleScore(scores, best.val, best.idx, pivot, each, None, None, "device")
        return (res, grad, eg.transpose(0, 2, 1)) if want_each else (res, grad)
    each, eg = np.full((H, R), np.nan), np.full((H, d, R), np.nan)

    def evaluate():
        sc, g = model.score_grad(acq, p, xs)
        return sc, np.asarray(g).reshape(d, R)

    scores, best_val, best_idx = _ens_host_route(model, Theta, w, pivot, [each, eg], evaluate)
    grad = np.asfortranarray(ensemble_average(eg.reshape(H, d * R), w, pivot).reshape(d, R))
    res = EnsembleScore(scores, best_val, best_idx, pivot, each if want_each else None, None, None, "host")
    return (res, grad, eg) if want_each else (res, grad)


class JointSample:
    """Result of sample_joint: samples (S x R, or None), best_val[S] / best_idx[S] (arg-max of every draw: strict '>', ties to the
    smallest index), mu[R], jitter (what was added to the diagonal), tries (failed factorisations before the one that went through),
    factor (R x R lower triangular, or None)."""
    __slots__ = ("samples", "best_val", "best_idx", "mu", "jitter", "tries", "factor")

    def __init__(self, samples, best_val, best_idx, mu, jitter, tries, factor):
        self.samples, self.best_val, self.best_idx, self.mu = samples, best_val, best_idx, mu
        self.jitter, self.tries, self.factor = jitter, tries, factor

    def __iter__(self):
        return iter((self.samples, self.best_val, self.best_idx, self.mu, self.jitter, self.tries, self.factor))


def _sample_joint(lib, handle, xs, S, seed, jitter, max_tries, want_samples, want_factor):
    R, S = xs.shape[1], int(S)
    mu = np.empty(R)
    samples = np.empty((S, R)) if want_samples and S > 0 else None
    factor = np.empty((R, R)) if want_factor else None
    out = (Best * max(S, 1))()
    jit, tries = C.c_double(0.0), C.c_int(0)
    check(lib.bohip_gp_sample_joint(handle, _ptr(xs), R, S, int(seed), float(jitter), int(max_tries), _ptr(mu),
                                    _ptr(factor) if factor is not None else None,
                                    _ptr(samples) if samples is not None else None, out, C.byref(jit), C.byref(tries)))
    vals = np.array([out[i].val for i in range(S)])
    idx = np.array([out[i].idx for i in range(S)], dtype=np.int64)
    return JointSample(samples, vals, idx, mu, jit.value, tries.value, factor)


class QEIBatch:
    """Result of qei_batch: idx[q] (int64, -1 where nothing could win), gain[q] (the sample-average gain of every pick; their sum is
    the q-EI estimate of the batch), jitter / tries (as JointSample), samples (S x R, or None)."""
    __slots__ = ("idx", "gain", "jitter", "tries", "samples")

    def __init__(self, idx, gain, jitter, tries, samples):
        self.idx, self.gain, self.jitter, self.tries, self.samples = idx, gain, jitter, tries, samples

    def __iter__(self):
        return iter((self.idx, self.gain, self.jitter, self.tries, self.samples))


def _qei_batch(lib, handle, xs, q, S, seed, tau, jitter, max_tries, want_samples):
    R, S, q = xs.shape[1], int(S), int(q)
    idx = np.full(max(q, 1), -1, dtype=np.int64)
    gain = np.zeros(max(q, 1))
    samples = np.empty((S, R)) if want_samples and S > 0 else None
    jit, tries = C.c_double(0.0), C.c_int(0)
    check(lib.bohip_gp_qei_batch(handle, _ptr(xs), R, S, int(seed), float(jitter), int(max_tries), float(tau), q,
                                 idx.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(gain),
                                 _ptr(samples) if samples is not None else None, C.byref(jit), C.byref(tries)))
    return QEIBatch(idx, gain, jit.value, tries.value, samples)


def _qei_select(lib, handle, samples, tau, q):
    F = np.ascontiguousarray(np.asarray(samples, dtype=np.float64))
    if F.ndim != 2:
        raise ValueError(f"samples must be S x R (one draw per row), got shape {F.shape}")
    q = int(q)
    idx = np.full(max(q, 1), -1, dtype=np.int64)
    gain = np.zeros(max(q, 1))
    check(lib.bohip_gp_qei_select(handle, _ptr(F), F.shape[0], F.shape[1], float(tau), q,
                                  idx.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(gain)))
    return idx, gain


class KGResult:
    """Result of kg: values[E] (the knowledge gradient of every evaluation point, >= 0), nseg[E] (int32: segments of the upper
    envelope beyond the first), mu[R] (the latent posterior mean of the candidates), best_val / best_idx (the arg-max over the
    evaluation points under score's rule: first maximum, NaN never wins, -Inf / -1 if nothing can win)."""
    __slots__ = ("values", "nseg", "mu", "best_val", "best_idx")

    def __init__(self, values, nseg, mu, best_val, best_idx):
        self.values, self.nseg, self.mu, self.best_val, self.best_idx = values, nseg, mu, best_val, best_idx

    def __iter__(self):
        return iter((self.values, self.nseg, self.mu, self.best_val, self.best_idx))


def _kg(lib, handle, xs, n_eval):
    R = xs.shape[1]
    E = R if n_eval is None else int(n_eval)
    values = np.zeros(max(E, 1))
    nseg = np.zeros(max(E, 1), dtype=np.int32)
    mu = np.empty(R)
    best = Best()
    check(lib.bohip_gp_kg(handle, _ptr(xs), R, E, _ptr(values), nseg.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(mu), C.byref(best)))
    return KGResult(values, nseg, mu, best.val, best.idx)


def _kg_lines(lib, handle, a, B):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
    B = np.ascontiguousarray(np.atleast_2d(np.asarray(B, dtype=np.float64)))
    if B.ndim != 2 or B.shape[1] != a.size:
        raise ValueError(f"B must be E x {a.size} (one evaluation point per row), got shape {B.shape}")
    E = B.shape[0]
    values = np.zeros(max(E, 1))
    nseg = np.zeros(max(E, 1), dtype=np.int32)
    check(lib.bohip_kg_lines(handle, _ptr(a), _ptr(B), a.size, E, _ptr(values), nseg.ctypes.data_as(C.POINTER(C.c_int32))))
    return values, nseg


class MESResult:
    """Result of mes: values[R] (MES of every candidate), maxvals[K] (the samples of the maximum), quantiles[3] (y25, y50, y75 of
    the Gumbel fit; NaN in joint mode), mu[R], var[R] (the posterior the values were computed from), best_val / best_idx (the
    arg-max under score's rule: first maximum, NaN never wins, -Inf / -1 if nothing can win), jitter / tries (joint mode)."""
    __slots__ = ("values", "maxvals", "quantiles", "mu", "var", "best_val", "best_idx", "jitter", "tries")

    def __init__(self, values, maxvals, quantiles, mu, var, best_val, best_idx, jitter=0.0, tries=0):
        self.values, self.maxvals, self.quantiles, self.mu, self.var = values, maxvals, quantiles, mu, var
        self.best_val, self.best_idx, self.jitter, self.tries = best_val, best_idx, jitter, tries

    def __iter__(self):
        return iter((self.values, self.maxvals, self.quantiles, self.mu, self.var, self.best_val, self.best_idx))


MES_MODES = {"gumbel": _lib.MES_GUMBEL, "joint": _lib.MES_JOINT}


def _mes(lib, handle, xs, samples, mode, seed, floor, jitter_rel, max_tries):
    if mode not in MES_MODES:
        raise ValueError(f"mode must be one of {sorted(MES_MODES)}, got {mode!r}")
    R, K = xs.shape[1], int(samples)
    values, mu, var = np.empty(max(R, 1)), np.empty(max(R, 1)), np.empty(max(R, 1))
    maxvals, quant = np.empty(max(K, 1)), np.empty(3)
    best, jit, tries = Best(), C.c_double(0.0), C.c_int(0)
    check(lib.bohip_gp_mes(handle, _ptr(xs), R, K, MES_MODES[mode], int(seed), -math.inf if floor is None else float(floor),
                           float(jitter_rel), int(max_tries), _ptr(values), _ptr(maxvals), _ptr(quant), _ptr(mu), _ptr(var),
                           C.byref(best), C.byref(jit), C.byref(tries)))
    return MESResult(values, maxvals, quant, mu, var, best.val, best.idx, jit.value, tries.value)


def _mes_values(lib, handle, mu, var, maxvals, want_grad):
    mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).ravel())
    var = np.ascontiguousarray(np.asarray(var, dtype=np.float64).ravel())
    mv = np.ascontiguousarray(np.asarray(maxvals, dtype=np.float64).ravel())
    if mu.size != var.size:
        raise ValueError("mu and var differ in length")
    values = np.empty(max(mu.size, 1))
    dmu, dvar = (np.empty(max(mu.size, 1)), np.empty(max(mu.size, 1))) if want_grad else (None, None)
    best = Best()
    check(lib.bohip_mes_values(handle, _ptr(mu), _ptr(var), mu.size, _ptr(mv), mv.size, _ptr(values),
                               _ptr(dmu) if want_grad else None, _ptr(dvar) if want_grad else None, C.byref(best)))
    return (values, dmu, dvar, best.val, best.idx) if want_grad else (values, best.val, best.idx)


def _mes_gumbel(lib, handle, mu, var, samples, seed, floor):
    mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).ravel())
    var = np.ascontiguousarray(np.asarray(var, dtype=np.float64).ravel())
    if mu.size != var.size:
        raise ValueError("mu and var differ in length")
    K = int(samples)
    quant, maxvals = np.empty(3), np.empty(max(K, 1))
    check(lib.bohip_mes_gumbel(handle, _ptr(mu), _ptr(var), mu.size, K, int(seed), -math.inf if floor is None else float(floor),
                               _ptr(quant), _ptr(maxvals)))
    return quant, maxvals


# ---- constrained optimisation (include/bohip_con.h) -------------------------------------------------------------
CON_ACQ = {"EI": _lib.ACQ["EI"], "PI": _lib.ACQ["PI"], "LogEI": _lib.ACQ["LogEI"], "Feasibility": _lib.CON_FEASIBILITY}
_ip = C.POINTER(C.c_int)


class ConstrainedScore:
    """Result of ConstrainedGPE.score: scores[R], logfeas[R] (sum_c log P(constraint c holds)), grad[d, R] or None, mu and var
    [(C + 1), R] (row 0 the objective; NaN under "Feasibility"), best_val / best_idx (first maximum, NaN never wins, -Inf / -1)."""
    __slots__ = ("scores", "logfeas", "grad", "mu", "var", "best_val", "best_idx")

    def __init__(self, scores, logfeas, grad, mu, var, best_val, best_idx):
        self.scores, self.logfeas, self.grad, self.mu, self.var = scores, logfeas, grad, mu, var
        self.best_val, self.best_idx = best_val, best_idx

    def __iter__(self):
        return iter((self.scores, self.logfeas, self.grad, self.mu, self.var, self.best_val, self.best_idx))


def _con_args(acq, params, thresholds, senses):
    if acq not in CON_ACQ:
        raise ValueError(f"a constrained score takes one of {sorted(CON_ACQ)}, got {acq!r}: a signed score has no product form")
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)).ravel())
    s = np.ascontiguousarray(np.atleast_1d(np.asarray(senses)).ravel().astype(np.intc))
    if t.size != s.size:
        raise ValueError("thresholds and senses differ in length")
    p = np.ascontiguousarray(np.concatenate([np.atleast_1d(np.asarray(params if params is not None else [], dtype=np.float64)).ravel(),
                                             np.zeros(2)]))
    return CON_ACQ[acq], p, t, s


def con_values(model, acq, params, thresholds, senses, mu, var, want_grad=False):
    """bohip_con_values: the feasibility-weighted score of `acq` ("EI", "PI": a exp(L); "LogEI": a + L; "Feasibility": L) on the
    moments mu, var [(C + 1), R] (row 0 the objective, the others the constraints; L = sum_c log Phi(s_c (mu_c - t_c) / sigma_c)).
    `model` gives the device only.  -> (value[R], logfeas[R], dmu, dvar, best_val, best_idx); dmu and dvar [(C + 1), R] are the
    partials of the score in every model's moments, None without want_grad."""
    aid, p, t, s = _con_args(acq, params, thresholds, senses)
    mu = np.ascontiguousarray(np.atleast_2d(np.asarray(mu, dtype=np.float64)))
    var = np.ascontiguousarray(np.atleast_2d(np.asarray(var, dtype=np.float64)))
    if mu.shape != var.shape or mu.shape[0] != t.size + 1:
        raise ValueError(f"mu and var must both be (C + 1) x R = {t.size + 1} x R, got {mu.shape} and {var.shape}")
    R = mu.shape[1]
    value, logfeas = np.empty(max(R, 1)), np.empty(max(R, 1))
    dmu, dvar = (np.empty((t.size + 1, max(R, 1))), np.empty((t.size + 1, max(R, 1)))) if want_grad else (None, None)
    best = Best()
    check(model._lib.bohip_con_values(model._h, aid, _ptr(p), t.size, _ptr(t), s.ctypes.data_as(_ip), _ptr(mu), _ptr(var), R,
                                      _ptr(value), _ptr(logfeas), _ptr(dmu) if want_grad else None,
                                      _ptr(dvar) if want_grad else None, C.byref(best)))
    return value[:R], logfeas[:R], dmu, dvar, best.val, best.idx


class ConstrainedGPE:
    """An objective model and C constraint models scored together (include/bohip_con.h; an extension: the reference's
    acquisition closes over one model).  Constraint c is feasible where senses[c] * (g_c(x) - thresholds[c]) >= 0.  The members are
    ElasticGPE models of one dimension on one device, each with its own kernel, hyper-parameters and observations; one model may
    serve two constraints (t_lo <= g <= t_hi).  `x`, `y`, `nobs` are the objective's, so the model reads like one model to BOpt."""

    def __init__(self, objective, constraints, thresholds, senses):
        self.objective, self.constraints = objective, list(constraints)
        self.thresholds = np.atleast_1d(np.asarray(thresholds, dtype=np.float64)).ravel().copy()
        self.senses = np.atleast_1d(np.asarray(senses)).ravel().astype(np.int64)
        C_ = len(self.constraints)
        if not 0 <= C_ <= _lib.CON_CMAX:
            raise ValueError(f"0 .. {_lib.CON_CMAX} constraints are supported, got {C_}")
        if self.thresholds.size != C_ or self.senses.size != C_:
            raise ValueError("constraints, thresholds and senses differ in length")
        if not np.all(np.isfinite(self.thresholds)):
            raise ValueError("thresholds must be finite")
        if not np.all(np.abs(self.senses) == 1):
            raise ValueError("senses are +1 (feasible where g >= t) or -1 (feasible where g <= t)")
        for m in self.members:
            if type(m).__name__ == "MultiGPE":
                raise ValueError("ConstrainedGPE members are single-device models: MultiGPE is not supported")
            if m.dim != objective.dim:
                raise ValueError("the members differ in dimension")
            _refuse_site_member(m, "ConstrainedGPE")

    @property
    def members(self):
        return [self.objective] + self.constraints

    dim = property(lambda self: self.objective.dim)
    x = property(lambda self: self.objective.x)
    y = property(lambda self: self.objective.y)
    nobs = property(lambda self: self.objective.nobs)

    def __repr__(self):
        return f"ConstrainedGPE({self.objective!r}, {len(self.constraints)} constraints)"

    def is_feasible(self, g):
        """Whether observed constraint values g [C] or [C, n] satisfy every constraint."""
        g = np.asarray(g, dtype=np.float64)
        t, s = (self.thresholds, self.senses) if g.ndim == 1 else (self.thresholds[:, None], self.senses[:, None])
        return np.all(s * (g - t) >= 0, axis=0) if g.size else np.ones(g.shape[1:], dtype=bool)

    def observed_g(self):
        """The constraints' observations [C, n]; the members' observations must be aligned (update_ keeps them so)."""
        n = self.objective.nobs
        if any(m.nobs != n for m in self.constraints):
            raise ValueError("the members' observations are not aligned: feasibility of an observation needs every member's value")
        return np.stack([np.asarray(m.y, dtype=np.float64) for m in self.constraints]) if self.constraints else np.zeros((0, n))

    def feasible_mask(self):
        return np.asarray(self.is_feasible(self.observed_g()), dtype=bool).reshape(-1)

    def feasible_incumbent(self):
        """The best observed y among the observations whose observed g satisfy every constraint, or None."""
        if self.objective.nobs == 0:
            return None
        ok = self.feasible_mask()
        return float(np.max(np.asarray(self.objective.y)[ok])) if ok.any() else None

    def update_(self, x, y, g):
        """Append observations to every member: x [d, n], y [n], g [C, n] (or [C] for one point)."""
        y = np.atleast_1d(np.asarray(y, dtype=np.float64))
        g = np.asarray(g, dtype=np.float64).reshape(len(self.constraints), y.size)
        self.objective.append_(x, y)
        for c, m in enumerate(self.constraints):
            m.append_(x, g[c])
        return self

    def score(self, acq, params, xs, want_grad=False, want_moments=True):
        """ONE bohip_gp_score_con call: every member's posterior on its own stream, the combine and the arg-max on the device.
        acq: "EI" / "PI" (a exp(L)), "LogEI" (a + L) or "Feasibility" (L alone).  xs is d x R.  -> ConstrainedScore."""
        aid, p, t, s = _con_args(acq, params, self.thresholds, self.senses)
        obj = self.objective
        xs = _cols(xs, obj.dim)
        R, C_ = xs.shape[1], len(self.constraints)
        n = max(R, 1)
        scores, logfeas = np.empty(n), np.empty(n)
        grad = np.empty((obj.dim, n), order="F") if want_grad else None
        mu, var = (np.empty((C_ + 1, n)), np.empty((C_ + 1, n))) if want_moments and R > 0 else (None, None)
        handles = (C.c_void_p * max(C_, 1))(*[m._h for m in self.constraints])
        best = Best()
        check(obj._lib.bohip_gp_score_con(obj._h, aid, _ptr(p), C_, handles, _ptr(t), s.ctypes.data_as(_ip), _ptr(xs), R,
                                          _ptr(scores), _ptr(logfeas), _ptr(grad) if want_grad else None,
                                          _ptr(mu) if mu is not None else None, _ptr(var) if var is not None else None, C.byref(best)))
        return ConstrainedScore(scores[:R], logfeas[:R], grad[:, :R] if want_grad else None, mu, var, best.val, best.idx)

    def close(self):
        for m in self.members:
            m.close()


# ---- two-objective optimisation (include/bohip_mo.h) -----------------------------------------------------------
class MOScore:
    """Result of MultiObjectiveGPE.score: scores[R] (the exact EHVI), grad[d, R] or None, mu and var [2, R] (row m objective m),
    best_value / best_index (first maximum, NaN never wins, -Inf / -1)."""
    __slots__ = ("scores", "grad", "mu", "var", "best_value", "best_index")

    def __init__(self, scores, grad, mu, var, best_value, best_index):
        self.scores, self.grad, self.mu, self.var = scores, grad, mu, var
        self.best_value, self.best_index = best_value, best_index

    best_val = property(lambda self: self.best_value)      # (the names the candidate route of acquire_max reads)
    best_idx = property(lambda self: self.best_index)

    def __iter__(self):
        return iter((self.scores, self.grad, self.mu, self.var, self.best_value, self.best_index))


def _ref2(ref):
    ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).ravel())
    if ref.size != 2:
        raise ValueError(f"the reference point has two coordinates, got {ref.size}")
    return ref


def mo_front(Y, ref):
    """bohip_mo_front (host code: no device is needed): the observations Y [2, n] (both objectives MAXIMISED) that strictly dominate
    `ref` and are not weakly dominated by another observation, ascending in f1 and descending in f2, of equal points one.
    -> (front[2, n_front], hv), hv the hypervolume the front dominates above ref."""
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(2, -1))
    ref = _ref2(ref)
    n = Y.shape[1]
    out = np.empty((2, max(n, 1)))
    nf, hv = C.c_int64(0), C.c_double(0.0)
    check(_lib.load().bohip_mo_front(_ptr(Y), n, _ptr(ref), _ptr(out), out.shape[1], C.byref(nf), C.byref(hv)))
    return np.ascontiguousarray(out[:, :nf.value]), hv.value


def ehvi_values(model, front, ref, mu, var, want_grad=False):
    """bohip_mo_ehvi_values: the exact expected hypervolume improvement over `front` [2, n_front] (as mo_front returns it) above `ref`
    on the moments mu, var [2, R] of two independent posteriors.  `model` gives the device only.
    -> (value[R], dmu, dvar, best_value, best_index); dmu and dvar [2, R] are the partials in the moments, None without want_grad."""
    front = np.ascontiguousarray(np.asarray(front, dtype=np.float64).reshape(2, -1))
    ref = _ref2(ref)
    mu = np.ascontiguousarray(np.atleast_2d(np.asarray(mu, dtype=np.float64)))
    var = np.ascontiguousarray(np.atleast_2d(np.asarray(var, dtype=np.float64)))
    if mu.shape != var.shape or mu.shape[0] != 2:
        raise ValueError(f"mu and var must both be 2 x R, got {mu.shape} and {var.shape}")
    R = mu.shape[1]
    value = np.empty(max(R, 1))
    dmu, dvar = (np.empty((2, max(R, 1))), np.empty((2, max(R, 1)))) if want_grad else (None, None)
    best = Best()
    check(model._lib.bohip_mo_ehvi_values(model._h, _ptr(front), front.shape[1], _ptr(ref), _ptr(mu), _ptr(var), R, _ptr(value),
                                          _ptr(dmu) if want_grad else None, _ptr(dvar) if want_grad else None, C.byref(best)))
    return value[:R], (dmu[:, :R] if want_grad else None), (dvar[:, :R] if want_grad else None), best.val, best.idx


def score_mo(m0, m1, front, ref, xs, want_grad=False, want_moments=True):
    """ONE bohip_gp_score_mo call on two ElasticGPE models (they may be the same model, and may hold different observations): the
    exact EHVI of their posteriors at the columns of xs [d, R] over `front` [2, n_front] above `ref`.  -> MOScore."""
    front = np.ascontiguousarray(np.asarray(front, dtype=np.float64).reshape(2, -1))
    ref = _ref2(ref)
    xs = _cols(xs, m0.dim)
    R = xs.shape[1]
    n = max(R, 1)
    scores = np.empty(n)
    grad = np.empty((m0.dim, n), order="F") if want_grad else None
    mu, var = (np.empty((2, n)), np.empty((2, n))) if want_moments and R > 0 else (None, None)
    best = Best()
    check(m0._lib.bohip_gp_score_mo(m0._h, m1._h, _ptr(front), front.shape[1], _ptr(ref), _ptr(xs), R, _ptr(scores),
                                    _ptr(grad) if want_grad else None, _ptr(mu) if mu is not None else None,
                                    _ptr(var) if var is not None else None, C.byref(best)))
    return MOScore(scores[:R], grad[:, :R] if want_grad else None, mu, var, best.val, best.idx)


class MultiObjectiveGPE:
    """Two objective models scored together by the exact expected hypervolume improvement (include/bohip_mo.h; an
    extension: the reference optimises one objective).  Both objectives are MAXIMISED (BOpt's `sense` flips both).  The members are
    ElasticGPE models of one dimension on one device, each with its own kernel, hyper-parameters and observations.  `ref` is the
    reference point in the model's (maximised) sense; None fixes it ONCE, at the first score, per objective at
    min y - 0.1 (max y - min y) (min y - 1 if that range is 0) of the observations held then, and keeps it in `ref`.
    `x`, `nobs` are the first member's; `y` is [2, n]."""

    def __init__(self, objectives, ref=None):
        objectives = tuple(objectives)
        if len(objectives) != 2:
            raise ValueError(f"MultiObjectiveGPE takes two objectives, got {len(objectives)}")
        for m in objectives:
            if type(m).__name__ == "MultiGPE":
                raise ValueError("MultiObjectiveGPE members are single-device models: MultiGPE is not supported")
        if objectives[0].dim != objectives[1].dim:
            raise ValueError("the members differ in dimension")
        for m in objectives:
            _refuse_site_member(m, "MultiObjectiveGPE")
        self.objectives = objectives
        self.ref = None if ref is None else _ref2(ref).copy()
        if self.ref is not None and not np.all(np.isfinite(self.ref)):
            raise ValueError("the reference point must be finite")

    members = property(lambda self: list(self.objectives))
    dim = property(lambda self: self.objectives[0].dim)
    x = property(lambda self: self.objectives[0].x)
    nobs = property(lambda self: self.objectives[0].nobs)

    def __repr__(self):
        return f"MultiObjectiveGPE({self.objectives[0]!r}, {self.objectives[1]!r}, ref={self.ref})"

    @property
    def y(self):
        """The observations [2, n]; the members' observations must be aligned (update_ keeps them so)."""
        a, b = self.objectives
        if a.nobs != b.nobs:
            raise ValueError("the members' observations are not aligned: a front needs both values of every observation")
        return np.stack([np.asarray(a.y, dtype=np.float64), np.asarray(b.y, dtype=np.float64)])

    def default_ref(self):
        """The default rule on the observations held now (not stored)."""
        Y = self.y
        if Y.shape[1] == 0:
            raise ValueError("the default reference point needs observations")
        lo, hi = Y.min(axis=1), Y.max(axis=1)
        return np.where(hi - lo > 0.0, lo - 0.1 * (hi - lo), lo - 1.0)

    def reference_point(self, fix=False):
        """`ref`, or the default rule's point where none is fixed yet; fix=True stores it (what the first score does)."""
        if self.ref is not None:
            return self.ref
        r = self.default_ref()
        if fix:
            self.ref = r
        return r

    def _front_hv(self):
        return mo_front(self.y, self.reference_point())

    front = property(lambda self: self._front_hv()[0])
    hypervolume = property(lambda self: self._front_hv()[1])

    def front_indices(self):
        """The column of the first observation that equals each front point."""
        Y, F = self.y, self.front
        return np.array([int(np.flatnonzero((Y[0] == F[0, i]) & (Y[1] == F[1, i]))[0]) for i in range(F.shape[1])], dtype=np.int64)

    def update_(self, x, y):
        """Append observations to both members: x [d, n], y [2, n] (or [2] for one point)."""
        y = np.asarray(y, dtype=np.float64)
        if y.shape[0] != 2:
            raise ValueError(f"y has one row per objective, 2 x n; got shape {y.shape}")
        y = y.reshape(2, -1)
        for m, row in zip(self.objectives, y):
            m.append_(x, row)
        return self

    append_ = update_
    append = update_

    def score(self, xs, want_grad=False, want_moments=True):
        """ONE bohip_gp_score_mo call: both members' posteriors on their own streams, the EHVI over the observed front and the
        arg-max on the device.  xs is d x R.  -> MOScore."""
        ref = self.reference_point(fix=True)
        front, _ = mo_front(self.y, ref)
        return score_mo(self.objectives[0], self.objectives[1], front, ref, xs, want_grad, want_moments)

    def close(self):
        for m in self.objectives:
            m.close()


# ---- two to four objectives (include/bohip_mom.h) ----------------------------------------------------------------
def _rows(a, what):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or not 2 <= a.shape[0] <= _lib.MOM_OBJ_MAX:
        raise ValueError(f"{what} has one row per objective, M x n with M in 2..{_lib.MOM_OBJ_MAX}; got shape {a.shape}")
    return np.ascontiguousarray(a)


def _refm(ref, M):
    ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).ravel())
    if ref.size != M:
        raise ValueError(f"the reference point has one coordinate per objective, {M}; got {ref.size}")
    return ref


def mom_front(Y, ref):
    """bohip_mom_front (host code: no device is needed): the observations Y [M, n] (every objective MAXIMISED, M = 2..4) strictly
    above `ref` in every coordinate and not weakly dominated by another observation, in lexicographic ascending order, of equal points
    one.  -> (front[M, n_front], hv), hv the hypervolume the front dominates above ref."""
    Y = _rows(Y, "Y")
    M, n = Y.shape
    ref = _refm(ref, M)
    out = np.empty((M, max(n, 1)))
    nf, hv = C.c_int64(0), C.c_double(0.0)
    check(_lib.load().bohip_mom_front(_ptr(Y), M, n, _ptr(ref), _ptr(out), out.shape[1], C.byref(nf), C.byref(hv)))
    return np.ascontiguousarray(out[:, :nf.value]), hv.value


def mom_boxes(front, ref):
    """bohip_mom_boxes (host code): the decomposition of the region above `ref` that no point of `front` [M, n_front] dominates.
    -> (levels, boxes): levels a list of M arrays (ref_m, the front's distinct values ascending, +Inf); boxes Int32 [2M, n_boxes], row
    m the lower and row M + m the upper level index of every box in objective m."""
    front = _rows(front, "front")
    M, n = front.shape
    ref = _refm(ref, M)
    lib = _lib.load()
    levels, nl, nb = np.empty((M, n + 2)), np.zeros(M, dtype=np.int64), C.c_int64(0)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))   # noqa: E731
    check(lib.bohip_mom_boxes(_ptr(front), M, n, _ptr(ref), _ptr(levels), i64(nl), None, 0, C.byref(nb)))
    boxes = np.empty((2 * M, nb.value), dtype=np.int32)
    check(lib.bohip_mom_boxes(_ptr(front), M, n, _ptr(ref), None, None, boxes.ctypes.data_as(C.POINTER(C.c_int32)), nb.value, None))
    return [levels[m, :nl[m]].copy() for m in range(M)], boxes


def ehvi_values_many(model, front, ref, mu, var, want_grad=False):
    """bohip_mom_ehvi_values: the exact expected hypervolume improvement over `front` [M, n_front] above `ref` on the moments mu, var
    [M, R] of M independent posteriors, as a sum over the front's boxes.  `model` gives the device only.
    -> (value[R], dmu, dvar, best_value, best_index); dmu and dvar [M, R] are the partials in the moments, None without want_grad."""
    mu, var = _rows(np.atleast_2d(mu), "mu"), _rows(np.atleast_2d(var), "var")
    if mu.shape != var.shape:
        raise ValueError(f"mu and var must both be M x R, got {mu.shape} and {var.shape}")
    M, R = mu.shape
    front = np.ascontiguousarray(np.asarray(front, dtype=np.float64).reshape(M, -1))
    ref = _refm(ref, M)
    value = np.empty(max(R, 1))
    dmu, dvar = (np.empty((M, max(R, 1))), np.empty((M, max(R, 1)))) if want_grad else (None, None)
    best = Best()
    check(model._lib.bohip_mom_ehvi_values(model._h, M, _ptr(front), front.shape[1], _ptr(ref), _ptr(mu), _ptr(var), R, _ptr(value),
                                           _ptr(dmu) if want_grad else None, _ptr(dvar) if want_grad else None, C.byref(best)))
    return (value[:R], (np.ascontiguousarray(dmu[:, :R]) if want_grad else None), (np.ascontiguousarray(dvar[:, :R]) if want_grad else None),
            best.val, best.idx)


def score_mom(models, front, ref, xs, want_grad=False, want_moments=True):
    """ONE bohip_gp_score_mom call on 2 to 4 ElasticGPE models (a model may repeat, and they may hold different observations): the
    exact EHVI of their posteriors at the columns of xs [d, R] over `front` [M, n_front] above `ref`.  -> MOScore, mu and var [M, R]."""
    models = list(models)
    M = len(models)
    if not 2 <= M <= _lib.MOM_OBJ_MAX:
        raise ValueError(f"score_mom takes 2 to {_lib.MOM_OBJ_MAX} models, got {M}")
    front = np.ascontiguousarray(np.asarray(front, dtype=np.float64).reshape(M, -1))
    ref = _refm(ref, M)
    m0 = models[0]
    xs = _cols(xs, m0.dim)
    R = xs.shape[1]
    n = max(R, 1)
    scores = np.empty(n)
    grad = np.empty((m0.dim, n), order="F") if want_grad else None
    mu, var = (np.empty((M, n)), np.empty((M, n))) if want_moments and R > 0 else (None, None)
    handles = (C.c_void_p * M)(*[m._h for m in models])
    best = Best()
    check(m0._lib.bohip_gp_score_mom(handles, M, _ptr(front), front.shape[1], _ptr(ref), _ptr(xs), R, _ptr(scores),
                                     _ptr(grad) if want_grad else None, _ptr(mu) if mu is not None else None,
                                     _ptr(var) if var is not None else None, C.byref(best)))
    return MOScore(scores[:R], grad[:, :R] if want_grad else None, mu, var, best.val, best.idx)


class ManyObjectiveGPE(MultiObjectiveGPE):
    """Two to four objective models scored together by the exact expected hypervolume improvement as a sum over the boxes of the
    observed front (include/bohip_mom.h; an extension).  Every objective is MAXIMISED (BOpt's `sense` flips all).  What
    MultiObjectiveGPE says of its members, of `ref` (None: fixed once, at the first score, by the same rule per objective) and of
    `x`, `nobs` holds here; `y` is [M, n], `front` [M, n_front] in lexicographic ascending order.  A subclass, so that whatever
    accepts a MultiObjectiveGPE (acquire_max, BOpt) accepts this model."""

    def __init__(self, objectives, ref=None):
        objectives = tuple(objectives)
        M = len(objectives)
        if not 2 <= M <= _lib.MOM_OBJ_MAX:
            raise ValueError(f"ManyObjectiveGPE takes 2 to {_lib.MOM_OBJ_MAX} objectives, got {M}")
        for m in objectives:
            if type(m).__name__ == "MultiGPE":
                raise ValueError("ManyObjectiveGPE members are single-device models: MultiGPE is not supported")
        if any(m.dim != objectives[0].dim for m in objectives):
            raise ValueError("the members differ in dimension")
        for m in objectives:
            _refuse_site_member(m, "ManyObjectiveGPE")
        self.objectives = objectives
        self.ref = None if ref is None else _refm(ref, M).copy()
        if self.ref is not None and not np.all(np.isfinite(self.ref)):
            raise ValueError("the reference point must be finite")

    n_objectives = property(lambda self: len(self.objectives))

    def __repr__(self):
        return f"ManyObjectiveGPE({', '.join(repr(m) for m in self.objectives)}, ref={self.ref})"

    @property
    def y(self):
        """The observations [M, n]; the members' observations must be aligned (update_ keeps them so)."""
        if len({m.nobs for m in self.objectives}) != 1:
            raise ValueError("the members' observations are not aligned: a front needs every value of every observation")
        return np.stack([np.asarray(m.y, dtype=np.float64) for m in self.objectives])

    def _front_hv(self):
        return mom_front(self.y, self.reference_point())

    def front_indices(self):
        """The column of the first observation that equals each front point."""
        Y, F = self.y, self.front
        return np.array([int(np.flatnonzero(np.all(Y == F[:, i:i + 1], axis=0))[0]) for i in range(F.shape[1])], dtype=np.int64)

    def update_(self, x, y):
        """Append observations to every member: x [d, n], y [M, n] (or [M] for one point)."""
        y = np.asarray(y, dtype=np.float64)
        M = len(self.objectives)
        if y.ndim == 0 or y.shape[0] != M:
            raise ValueError(f"y has one row per objective, {M} x n; got shape {y.shape}")
        y = y.reshape(M, -1)
        for m, row in zip(self.objectives, y):
            m.append_(x, row)
        return self

    append_ = update_
    append = update_

    def score(self, xs, want_grad=False, want_moments=True):
        """ONE bohip_gp_score_mom call: every member's posterior on its own stream, the EHVI over the boxes of the observed front and
        the arg-max on the device.  xs is d x R.  -> MOScore, mu and var [M, R]."""
        ref = self.reference_point(fix=True)
        front, _ = mom_front(self.y, ref)
        return score_mom(self.objectives, front, ref, xs, want_grad, want_moments)


class PosteriorPaths:
    """S sample paths of one model's posterior on the device (bohip_paths, include/bohip_paths.h).  Self-contained: it holds its own copy
    of the observations, hyper-parameters, frequencies and coefficients.
      eval(xs, want_values=True) -> (values S x R or None, best_val[S], best_idx[S])   arg-max per path under score's rule
      eval_grad(xs, path_of=None) -> (f[R], grad d x R)   point j on path path_of[j] (None: path 0)
      coef(s) -> (omega F x d, w[M], u[N])"""

    def __init__(self, lib, handle, dim, S, M, seed):
        self._lib, self.dim, self._p = lib, int(dim), None
        p = C.c_void_p()
        check(lib.bohip_gp_paths_draw(handle, int(S), int(M), int(seed), C.byref(p)))
        self._p = p
        s, m, n, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.bohip_paths_dims(self._p, C.byref(s), C.byref(m), C.byref(n), C.byref(d)))
        self.S, self.M, self.N = s.value, m.value, n.value
        _lib.register(self)

    def _handle(self):
        if not self._p:
            raise _lib.BohipError(_lib.E_STATE, "the paths object is closed")
        return self._p

    def close(self):
        """Release the device object now (idempotent)."""
        p, self._p = getattr(self, "_p", None), None
        if p:
            self._lib.bohip_paths_destroy(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self, xs, want_values=True):
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        vals = np.empty((self.S, R)) if want_values else None
        out = (Best * self.S)()
        check(self._lib.bohip_paths_eval(self._handle(), _ptr(xs), R, _ptr(vals) if want_values else None, out))
        rec = np.frombuffer(out, dtype=[("val", "f8"), ("idx", "i8")])
        return vals, rec["val"].copy(), rec["idx"].copy()

    def eval_grad(self, xs, path_of=None):
        xs = _cols(xs, self.dim)
        R = xs.shape[1]
        f = np.empty(R)
        grad = np.empty((self.dim, R), order="F")
        po = None
        if path_of is not None:
            po = np.ascontiguousarray(np.broadcast_to(np.asarray(path_of, dtype=np.int64), (R,)))
        check(self._lib.bohip_paths_eval_grad(self._handle(), _ptr(xs), R,
                                              po.ctypes.data_as(C.POINTER(C.c_int64)) if po is not None else None, _ptr(f), _ptr(grad)))
        return f, grad

    def coef(self, s):
        om = np.empty((self.M // 2, self.dim))
        w = np.empty(self.M)
        u = np.empty(self.N)
        check(self._lib.bohip_paths_coef(self._handle(), int(s), _ptr(om), _ptr(w), _ptr(u)))
        return om, w, u


# ---- the generic functions of reference src/models/gp.jl ----------------------------------------
def mean_var(model, x):
    """gp.jl:2-5 (vector -> scalars) and :8 (d x R matrix -> vectors)."""
    x = np.asarray(x, dtype=np.float64)
    mu, var = model.predict_f(x)
    if x.ndim == 1:
        return float(mu[0]), float(var[0])
    return mu, var


def myrand(model, x, rng=None, *, seed=None):
    """gp.jl:6-7.  Vector: one draw from N(mu, sigma^2).  Matrix: ONE JOINT draw from N(mu, Sigma_post) over the columns
    (rand(gp, X) = mu + chol(Sigma)·z with jitter added until the factorisation succeeds -- GaussianProcesses.jl
    make_posdef!, UPSTREAM-UNVERIFIED; only the length is pinned by test/acquisitionfunctions.jl:8).
    seed given (matrix x, a model with sample_joint): the same draw made on the device, z from the library's generator keyed by
    `seed` (model.sample_joint, S = 1); without it the covariance is factorised on the host with z from `rng`."""
    x = np.asarray(x, dtype=np.float64)
    if seed is not None and x.ndim == 2 and hasattr(model, "sample_joint"):
        return model.sample_joint(x, 1, int(seed)).samples[0]
    rng = rng if rng is not None else np.random.default_rng()
    if x.ndim == 1:
        mu, var = model.predict_f(x)
        return float(mu[0] + math.sqrt(var[0]) * rng.standard_normal())
    if model.nobs == 0:
        raise RuntimeError("myrand on an empty model")
    mu, cov = model.predict_cov(x)
    z = rng.standard_normal(mu.shape)
    jitter, scale = 0.0, max(float(np.max(np.diag(cov))), np.finfo(float).tiny)
    for _ in range(40):
        try:
            Lc = np.linalg.cholesky(cov + jitter * np.eye(len(mu)))
            return mu + Lc @ z
        except np.linalg.LinAlgError:
            jitter = max(10.0 * jitter, 1e-12 * scale)
    raise np.linalg.LinAlgError("posterior covariance could not be made positive definite")


def dims(model):
    """gp.jl:9 -> (D, nobs)."""
    return model.dim, model.nobs


def maxy(model):
    """gp.jl:10.  A model with replicated sites: the largest RAW evaluation (the reference's maximum(model.y)), not the largest mean."""
    if model.nobs == 0:
        return -math.inf
    return float(np.max(getattr(model, "ymax", model.y)))


def update_(model, x, y):
    """gp.jl:11  update!(model::GPE{<:ElasticArray}, x, y) = append!(model, x, y).  A model made with collapse=True takes the
    repeated columns of the call as one weighted site each (collapse_evaluations)."""
    if getattr(model, "collapse", False):
        return model.append_sites_(*collapse_evaluations(x, y))
    return model.append_(x, y)
