"""BOpt / boptimize_ / optimize: the reference's public loop (src/BayesianOptimization.jl) driven from the host;
"acquisition" and "model update" -- the two timed regions the reference brackets (:185,:194) -- run on the GPU."""
from __future__ import annotations

import enum
import math
import time
import warnings

import numpy as np

from .acquisition import (AbstractAcquisition, Constrained, ExpectedHypervolumeImprovement, ExpectedImprovement, Marginalised, MaxMean, NoisyExpectedImprovement, ThompsonSamplingSimple, _batched_lbfgs_ascent,
                          acquire_batch, acquire_max, acquire_max_pending, acquire_thompson_batch, defaultoptions, setparams_)
from ._lib import NotPositiveDefinite
from .model import ConstrainedGPE, ElasticGPE, Mat52Ard, MeanConst, MultiObjectiveGPE, refuse_weighted, update_
from .utils import (DurationCounter, IterationCounter, ScaledSobolIterator, init_, isdone as _isdone, latin_hypercube_sampling, step_)


class Sense(enum.IntEnum):                                    # :56
    Min = -1
    Max = 1


class Verbosity(enum.IntEnum):                                # :57
    Silent = 0
    Timings = 1
    Progress = 2


Min, Max = Sense.Min, Sense.Max
Silent, Timings, Progress = Verbosity.Silent, Verbosity.Timings, Verbosity.Progress


class ModelOptimizer:                                         # :44
    pass


class NoModelOptimizer(ModelOptimizer):                       # :48-49
    """Don't optimize the model ever."""


class MAPGPOptimizer(ModelOptimizer):
    """src/models/gp.jl:20-52: MAP hyper-parameter fit every ``every`` calls.  Each objective evaluation is a
    full device rebuild (kernel matrix + Cholesky + alpha) plus the analytic gradient 1/2 tr((aa' - cK^-1) dcK)
    formed on the device (bohip_gp_mll_grad); the bounded L-BFGS search itself stays on the host, like the
    reference's NLopt :LD_LBFGS driving GP.update_target_and_dtarget!.

    ``restarts = k > 1`` (an extension: the reference runs ONE search from the current parameters) starts k searches -- the current
    parameters and k - 1 Latin-hypercube points of the bounds, a side without a finite bound replaced by current -/+ ``startwidth``
    (log-parameters) -- and advances them in lock-step, one batched device evaluation of all k per step (bohip_gp_mll_grad_batch);
    ``maxeval`` then counts lock-step evaluations, i.e. per start.  ``seed`` seeds the starts.  The best end point wins, the first on ties.

    ``objective = "mll"`` (the default, the reference's) maximises the log marginal likelihood; ``"loo"`` (an extension) the
    leave-one-out predictive log-probability (Rasmussen & Williams 5.4.2; bohip_gp_loo_grad), in the single search
    and, with ``restarts > 1``, one batched device evaluation of all starts per step up to 512 observations
    (bohip_gp_loo_grad_batch), one set_params_ + loo_grad per start and step above."""

    def __init__(self, every=10, objective="mll", **kwargs):
        if objective not in ("mll", "loo"):
            raise ValueError(f"MAPGPOptimizer: objective must be 'mll' or 'loo', got {objective!r}")
        self.i = 0
        self.every = every
        self.options = {**self.defaultoptions(), **kwargs, "objective": objective}

    @staticmethod
    def defaultoptions():                                     # :48-52
        return dict(domean=True, kern=True, noise=True, lik=True, meanbounds=None, kernbounds=None, noisebounds=None,
                    likbounds=None, method="LD_LBFGS", maxeval=500, restarts=1, startwidth=3.0, seed=None)


class MarginalGPOptimizer(ModelOptimizer):
    """Samples of the hyper-parameter posterior instead of its mode (an extension: the reference fits the MAP point only), for the
    integrated acquisition Marginalised(a) of Snoek, Larochelle & Adams 2012.  Every ``every`` calls, ``samples`` chains of univariate
    slice sampling (Neal 2003, shrinkage) run in lock-step over the free parameters -- every likelihood evaluation is ONE batched
    device call for all chains (_fit_objective's dispatch, value only) -- for ``burn`` + ``thin`` sweeps; each chain's last state is
    one sample.  The priors are flat inside the bounds (the reference's "uniform priors in an interval", src/models/gp.jl:30-33), so
    every free parameter needs FINITE bounds: noisebounds = [lo, hi], meanbounds = [[lo], [hi]], kernbounds = [[lo...], [hi...]]
    (length-scales then log sigma); pass noise / domean / kern = False for what stays fixed (domean=False for a MeanZero model).
    The chains start at the current parameters and Latin-hypercube points of the box, as the multi-start MAP fit does.
    Afterwards model.hyper_samples = (Theta[H, P], weights) in mll_grad_batch's row layout with equal weights, and the model itself is
    set to the sample of highest likelihood and refitted, so everything that reads the model keeps working."""

    def __init__(self, every=10, samples=16, burn=20, thin=1, noisebounds=None, meanbounds=None, kernbounds=None, domean=True,
                 kern=True, noise=True, seed=None):
        if int(samples) < 1 or int(burn) < 0 or int(thin) < 1:
            raise ValueError("samples >= 1, burn >= 0 and thin >= 1 are required")
        for free, name, b in ((noise, "noisebounds", noisebounds), (domean, "meanbounds", meanbounds), (kern, "kernbounds", kernbounds)):
            if free and (b is None or not np.all(np.isfinite(np.concatenate([np.ravel(b[0]), np.ravel(b[1])]).astype(float)))):
                raise ValueError(f"MarginalGPOptimizer: {name} must be given and finite (flat priors need a box); "
                                 f"fix the parameter instead with {'domean' if name == 'meanbounds' else name[:-6]}=False")
        self.i = 0
        self.every = every
        self.options = dict(samples=int(samples), burn=int(burn), thin=int(thin), noisebounds=noisebounds, meanbounds=meanbounds,
                            kernbounds=kernbounds, domean=bool(domean), kern=bool(kern), noise=bool(noise), seed=seed)
        self._rng = np.random.default_rng(seed)
        self.options["rng"] = self._rng


def _slice_sample_batch(logp_batch, X0, lo, hi, sweeps, rng, max_shrink=200):
    """Univariate slice sampling with the shrinkage procedure (Neal 2003, fig. 5 and 8), H chains in lock-step.  X0[p, H]: one
    chain per column; lo, hi: the FINITE box, a coordinate's initial bracket is its whole interval (so no stepping out).
    logp_batch(X[p, H]) -> logp[H] is ONE evaluation of all columns; -inf (or NaN) is a rejected proposal.  The coordinates are
    cycled; in every shrinkage round all chains that have not yet accepted propose together, the others are masked (their column
    is evaluated at its current state and ignored).  Returns (X[p, H], logp[H], trace[sweeps, p, H])."""
    X = np.array(X0, dtype=np.float64, order="C")
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("slice sampling over a box needs finite bounds")
    p, H = X.shape
    f = np.asarray(logp_batch(X), dtype=np.float64).copy()
    trace = np.empty((int(sweeps), p, H))
    for s in range(int(sweeps)):
        for k in range(p):
            logy = f - rng.exponential(size=H)                # log(u f(x)), u ~ U(0, 1)
            L, R = np.full(H, lo[k]), np.full(H, hi[k])
            active = np.ones(H, dtype=bool)
            for _ in range(max_shrink):
                prop = L + rng.random(H) * (R - L)
                Xp = X.copy()
                Xp[k, active] = prop[active]
                fp = np.asarray(logp_batch(Xp), dtype=np.float64)
                with np.errstate(invalid="ignore"):
                    acc = active & (fp > logy) & (fp > -np.inf)
                X[k, acc], f[acc] = prop[acc], fp[acc]
                rej = active & ~acc
                left = rej & (prop < X[k])
                L[left] = prop[left]
                right = rej & ~left
                R[right] = prop[right]
                active = rej
                if not active.any():
                    break
        trace[s] = X
    return X, f, trace


def _marginal_fit(model, opt):
    if model.nobs == 0:
        return
    refuse_weighted(model, "MarginalGPOptimizer (its samples feed the marginalised acquisitions)")
    mean_free = opt["domean"] and isinstance(model.mean, MeanConst)
    x0, lo, hi = [], [], []
    if opt["noise"]:
        x0.append(model.logNoise); lo.append(float(opt["noisebounds"][0])); hi.append(float(opt["noisebounds"][1]))
    if mean_free:
        x0.append(model.mean.beta); lo.append(float(np.ravel(opt["meanbounds"][0])[0])); hi.append(float(np.ravel(opt["meanbounds"][1])[0]))
    nk = 0
    if opt["kern"]:
        kp = np.concatenate([model.kernel.ll, [model.kernel.lsigma]])
        nk = kp.size
        kb = opt["kernbounds"]
        if np.size(kb[0]) != nk or np.size(kb[1]) != nk:
            raise ValueError(f"kernbounds must have {nk} entries per side (length-scales, then log sigma)")
        x0 += kp.tolist(); lo += list(np.ravel(kb[0]).astype(float)); hi += list(np.ravel(kb[1]).astype(float))
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    if lo.size == 0:
        return
    x0 = np.clip(np.asarray(x0, float), lo, hi)

    def apply(x):
        i = 0
        kw = {}
        if opt["noise"]:
            kw["logNoise"] = x[i]; i += 1
        if mean_free:
            kw["beta"] = x[i]; i += 1
        if opt["kern"]:
            kw["ll"] = x[i:i + nk - 1]; kw["lsigma"] = x[i + nk - 1]
        model.set_params_(**kw)

    H, rng = opt["samples"], opt["rng"]
    base = np.concatenate([[model.logNoise, model.mean.beta if isinstance(model.mean, MeanConst) else 0.0], model.kernel.ll,
                           [model.kernel.lsigma]])
    nk_all = model.kernel.ll.size + 1
    idx = ([0] if opt["noise"] else []) + ([1] if mean_free else []) + (list(range(2, 2 + nk_all)) if opt["kern"] else [])
    fit_opt = dict(domean=opt["domean"], noise=opt["noise"], kern=opt["kern"])
    fg = _fit_objective(model, fit_opt, nk, apply, x0.size, H, want_grad=False)
    starts = np.concatenate([x0.reshape(-1, 1), latin_hypercube_sampling(lo, hi, H - 1, rng)], axis=1) if H > 1 else x0.reshape(-1, 1)
    X, f, _ = _slice_sample_batch(lambda Z: fg(Z)[0], starts, lo, hi, opt["burn"] + opt["thin"], rng)
    Theta = np.tile(base, (H, 1))
    Theta[:, idx] = X.T
    model.hyper_samples = (Theta, np.full(H, 1.0 / H))
    f = np.where(np.isfinite(f), f, -np.inf)
    w = int(np.argmax(f))                                     # the first of equal bests
    apply(X[:, w] if np.isfinite(f[w]) else x0)
    model.fit_()
    return float(f[w]), X[:, w].copy()


def optimizemodel_(o, model):                                 # :42-47 and NoModelOptimizer :49
    if isinstance(o, NoModelOptimizer) or o is None:
        return None
    if o.i % o.every == 0:
        # every member of a constrained or two-objective model
        for m in (model.members if isinstance(model, (ConstrainedGPE, MultiObjectiveGPE)) else [model]):
            if isinstance(o, MarginalGPOptimizer):
                _marginal_fit(m, o.options)
            else:
                _map_fit(m, o.options)
    o.i += 1


def _map_fit(model, opt):                                     # :54-77
    from scipy.optimize import minimize

    if model.nobs == 0:
        return
    names, x0, lo, hi = [], [], [], []
    if opt["noise"]:
        names.append("noise"); x0.append(model.logNoise)
        b = opt["noisebounds"] if opt["noisebounds"] is not None else [-math.inf, math.inf]
        lo.append(b[0]); hi.append(b[1])
    if opt["domean"] and isinstance(model.mean, MeanConst):
        names.append("mean"); x0.append(model.mean.beta)
        b = opt["meanbounds"] if opt["meanbounds"] is not None else [[-math.inf], [math.inf]]
        lo.append(np.ravel(b[0])[0]); hi.append(np.ravel(b[1])[0])
    nk = 0
    if opt["kern"]:
        kp = np.concatenate([model.kernel.ll, [model.kernel.lsigma]])
        nk = kp.size
        names += ["kern"] * nk; x0 += kp.tolist()
        b = opt["kernbounds"] if opt["kernbounds"] is not None else [[-math.inf] * nk, [math.inf] * nk]
        lo += list(np.ravel(b[0]).astype(float)); hi += list(np.ravel(b[1]).astype(float))
    x0 = np.clip(np.array(x0, float), lo, hi)

    def apply(x):
        i = 0
        kw = {}
        if opt["noise"]:
            kw["logNoise"] = x[i]; i += 1
        if opt["domean"] and isinstance(model.mean, MeanConst):
            kw["beta"] = x[i]; i += 1
        if opt["kern"]:
            kw["ll"] = x[i:i + nk - 1]; kw["lsigma"] = x[i + nk - 1]
        model.set_params_(**kw)

    loo = opt.get("objective", "mll") == "loo"
    if loo:
        refuse_weighted(model, 'MAPGPOptimizer(objective="loo") (the leave-one-out gradient)')

    def negmll(x):                                            # f = (x, g) -> ... gp.target, gp.dtarget  (:59-64)
        apply(x)
        try:
            m, dn, dm, dk = model.loo_grad() if loo else model.mll_grad()
        except NotPositiveDefinite:                           # not positive definite for these parameters; device
            return 1e300, np.zeros_like(x)                    # failures (E_HIP, E_NODEVICE, ...) propagate
        g = []
        if opt["noise"]:
            g.append(dn)
        if opt["domean"] and isinstance(model.mean, MeanConst):
            g.append(dm)
        if opt["kern"]:
            g += dk.tolist()
        return -m, -np.asarray(g, dtype=float)

    if int(opt.get("restarts", 1)) > 1:
        fg = _fit_objective(model, opt, nk, apply, x0.size, int(opt["restarts"]))
        val, best, _ = _multistart_map(fg, x0, np.asarray(lo, float), np.asarray(hi, float), int(opt["restarts"]), int(opt["maxeval"]),
                                       np.random.default_rng(opt.get("seed")), float(opt.get("startwidth", 3.0)))
        apply(best if np.isfinite(val) else x0)
        model.fit_()
        return val, best
    res = minimize(negmll, x0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                   options=dict(maxfun=int(opt["maxeval"])))
    best = res.x if np.isfinite(res.fun) and res.fun < 1e299 else x0
    apply(best)
    model.fit_()
    return -res.fun, best


def _multistart_map(fg_batch, x0, lo, hi, restarts, maxeval, rng, startwidth=3.0):
    """``restarts`` bounded L-BFGS ascents of the log marginal likelihood in lock-step.  fg_batch(X[p, R]) -> (mll[R], G[p, R]) is ONE
    evaluation of all columns (a failed one: -inf, from which the ascent backtracks).  Start 0 is x0 clipped to the bounds, the others
    a Latin hypercube of the bounds (an infinite side: x0 -/+ startwidth).  Returns (best mll, its x, the end value of every start)."""
    x0 = np.clip(np.asarray(x0, float), lo, hi)
    slo = np.where(np.isfinite(lo), lo, x0 - startwidth)
    shi = np.where(np.isfinite(hi), hi, x0 + startwidth)
    starts = np.concatenate([x0.reshape(-1, 1), latin_hypercube_sampling(slo, shi, restarts - 1, rng)], axis=1)
    f, X = _batched_lbfgs_ascent(fg_batch, starts, lo, hi, maxeval)
    f = np.where(np.isfinite(f), f, -np.inf)
    w = int(np.argmax(f))                                     # the first of equal bests
    return float(f[w]), X[:, w].copy(), f


# When the batched call runs (n observations, H settings): H at least the entry of the first row with n <= its size.
# PROVISIONAL: not from a measured table yet -- one mll_grad costs 0.27 ... 0.39 ms up to N = 500, the kernel
# is estimated at ~0.3 ms at N = 256 and ~2 ms at N = 512 whatever H.  tools/time_mll_batch.py measures both; its table replaces this.
_FIT_BATCH_MIN_H = ((64, 2), (128, 2), (256, 2), (512, 8))


# The same for the leave-one-out objective (loo_grad_batch against set_params_ + loo_grad per column).  Measured
# (profiles/loo_batch_ab.txt, tools/time_loo_batch.py at H = 2, 8, 32): a cell is batched where every batched run beat every loop
# run by more than the spread; the entry is the smallest measured H from which that holds.
_LOO_BATCH_MIN_H = ((64, 2), (128, 2), (256, 8), (512, 32))


def _fit_batched(n, H, nmax, table=_FIT_BATCH_MIN_H):
    if n > nmax:
        return False
    for size, hmin in table:
        if n <= size:
            return H >= hmin
    return False


def _fit_objective(model, opt, nk, apply, p, H, want_grad=True):
    """fg_batch of _multistart_map for a model: the free parameters of the fit sit in the optimisation vector, the fixed ones are
    constants of Theta's rows.  A device model of a size the batched call takes, and wins at, evaluates all columns in one launch;
    otherwise (or for a model without the call) every column is a set_params_ + mll_grad, at any N.  want_grad=False (the slice
    sampler): the same dispatch, value only -- the gradient is None, the batched call forms no inverse and the loop calls mll.
    opt["objective"] == "loo": the leave-one-out log-probability, all columns in one loo_grad_batch where the model has the call
    and _LOO_BATCH_MIN_H says so, otherwise set_params_ + loo_grad (value only: loo) per column."""
    loo = opt.get("objective", "mll") == "loo"
    mean_free = opt["domean"] and isinstance(model.mean, MeanConst)
    base = np.concatenate([[model.logNoise, model.mean.beta if isinstance(model.mean, MeanConst) else 0.0], model.kernel.ll,
                           [model.kernel.lsigma]])
    idx = ([0] if opt["noise"] else []) + ([1] if mean_free else []) + (list(range(2, 2 + nk)) if opt["kern"] else [])
    assert len(idx) == p
    if getattr(model, "weighted", False):                     # replicated sites: the batched kernels know no per-row noise term
        batched = False
    elif loo:
        batched = hasattr(model, "loo_grad_batch") and _fit_batched(model.nobs, H, model.mll_batch_dims()[1], _LOO_BATCH_MIN_H)
    else:
        batched = hasattr(model, "mll_grad_batch") and _fit_batched(model.nobs, H, model.mll_batch_dims()[1])

    def fg_batched(X):
        Theta = np.tile(base, (X.shape[1], 1))
        Theta[:, idx] = X.T
        mll, G, piv = (model.loo_grad_batch if loo else model.mll_grad_batch)(Theta, want_grad)
        return np.where(piv == 0, mll, -np.inf), np.ascontiguousarray(G[:, idx].T) if want_grad else None

    def fg_loop(X):
        f, G = np.full(X.shape[1], -np.inf), np.zeros(X.shape)
        for r in range(X.shape[1]):
            apply(X[:, r])
            try:
                if not want_grad:
                    f[r] = model.loo().total if loo else model.mll()
                    continue
                m, dn, dm, dk = model.loo_grad() if loo else model.mll_grad()
            except NotPositiveDefinite:
                continue
            full = np.concatenate([[dn, dm], dk])
            f[r], G[:, r] = m, full[idx]
        return f, G

    if not want_grad:
        return (lambda X: (fg_batched(X)[0], None)) if batched else (lambda X: (fg_loop(X)[0], None))
    return fg_batched if batched else fg_loop


class BOpt:
    """src/BayesianOptimization.jl:59-136 (same positional arguments, keyword names and validation)."""

    def __init__(self, func, model, acquisition, modeloptimizer, lowerbounds, upperbounds, *, sense=Max,
                 maxiterations=10 ** 4, maxduration=math.inf, acquisitionoptions=None, repetitions=1,
                 verbosity=Progress, initializer_iterations=None, initializer=None, rng=None, batchsize=1, batchoptions=None):
        # batchsize > 1 (an extension, the reference evaluates one point per iteration): an iteration proposes `batchsize` points
        # with acquire_batch(..., batchoptions) and appends all their evaluations in ONE model update.  batchoptions["method"]:
        # "fantasy" (default; Kriging believer / constant liar) or "qei" (ExpectedImprovement only: greedy Monte-Carlo q-EI over
        # joint posterior draws on the device)
        now = time.time()
        lowerbounds = np.asarray(lowerbounds, dtype=np.float64)
        upperbounds = np.asarray(upperbounds, dtype=np.float64)
        if initializer_iterations is None:
            initializer_iterations = 5 * len(lowerbounds)                        # :101
        if initializer is None:
            initializer = ScaledSobolIterator(lowerbounds, upperbounds, initializer_iterations)
        acquisitionoptions = {**defaultoptions(type(model), type(acquisition)), **(acquisitionoptions or {})}   # :105-106
        if maxiterations < len(initializer):
            raise ValueError(f"maxiterations = {maxiterations} < length(initializer) = {len(initializer)}")      # :107-108
        if not maxiterations >= 0:
            raise ValueError("maxiterations < 0")
        if not maxduration >= 0:
            raise ValueError("maxduration < 0")
        if len(lowerbounds) != len(upperbounds):
            raise ValueError("length of lowerbounds does not match length of upperbounds")
        if int(batchsize) != batchsize or batchsize < 1:
            raise ValueError(f"batchsize = {batchsize!r} is not a positive integer")
        if batchsize > 1 and isinstance(acquisition, Marginalised):
            raise ValueError("Marginalised acquisitions propose one point per iteration (batchsize = 1)")
        if batchsize == 1 and batchoptions:
            raise ValueError("batchoptions given with batchsize = 1")
        multi = isinstance(model, MultiObjectiveGPE)
        if multi != isinstance(acquisition, ExpectedHypervolumeImprovement):
            raise ValueError("a MultiObjectiveGPE model goes with the ExpectedHypervolumeImprovement acquisition and the other way "
                             f"round (got {type(model).__name__} with {type(acquisition).__name__})")
        if multi and batchsize > 1:
            raise ValueError("a MultiObjectiveGPE proposes one point per iteration (batchsize = 1)")
        if multi and isinstance(modeloptimizer, MarginalGPOptimizer):
            raise ValueError("MarginalGPOptimizer over a MultiObjectiveGPE is not supported: its samples have no two-objective "
                             "acquisition")
        constrained = isinstance(model, ConstrainedGPE)
        if constrained != isinstance(acquisition, Constrained):
            raise ValueError("a ConstrainedGPE model goes with a Constrained(a) acquisition and the other way round "
                             f"(got {type(model).__name__} with {type(acquisition).__name__}); Marginalised over a "
                             "ConstrainedGPE is not supported")
        if constrained and batchsize > 1:
            raise ValueError("a ConstrainedGPE proposes one point per iteration (batchsize = 1)")
        if constrained and isinstance(modeloptimizer, MarginalGPOptimizer):
            raise ValueError("MarginalGPOptimizer over a ConstrainedGPE is not supported: its samples have no constrained acquisition")
        if not np.all(lowerbounds <= upperbounds):
            raise ValueError("lowerbounds are not pointwise less than or eqal to upperbounds, they were possibly "
                             "passed in the wrong order")
        empty = model.y.size == 0
        if multi:                                                                # (two objectives have a front, not an optimum)
            current_optimum, current_optimizer = None, None
        elif constrained:                                                        # only feasible observations count
            ok = np.zeros(0, dtype=bool) if empty else model.feasible_mask()
            yy = np.where(ok, model.y, -math.inf) if ok.any() else None
            current_optimum = -math.inf * int(sense) if yy is None else int(sense) * float(np.max(yy))
            current_optimizer = np.zeros_like(lowerbounds) if yy is None else np.array(model.x[:, int(np.argmax(yy))])
        else:
            yraw = getattr(model, "ymax", model.y)                               # (replicated sites: the largest raw evaluation of each)
            current_optimum = -math.inf * int(sense) if empty else int(sense) * float(np.max(yraw))   # :117
            current_optimizer = np.zeros_like(lowerbounds) if empty else np.array(model.x[:, int(np.argmax(yraw))])
        self.func, self.sense, self.model = func, Sense(sense), model
        self.acquisition, self.acquisitionoptions, self.modeloptimizer = acquisition, acquisitionoptions, modeloptimizer
        self.lowerbounds, self.upperbounds = lowerbounds, upperbounds
        self.observed_optimum, self.observed_optimizer = current_optimum, current_optimizer
        self.model_optimum, self.model_optimizer = current_optimum, None if multi else current_optimizer.copy()
        self.iterations = IterationCounter(0, 0, maxiterations)
        self.duration = DurationCounter(now, maxduration, now, now + maxduration)
        self.verbosity, self.initializer, self.repetitions = Verbosity(verbosity), initializer, repetitions
        self.rng = rng if rng is not None else np.random.default_rng()
        self.batchsize, self.batchoptions = int(batchsize), dict(batchoptions or {})
        self.timeroutput = {}
        self._ask_pending = np.zeros((len(lowerbounds), 0), order="F")          # ask / tell: the columns that are out for evaluation
        self._ask_init = None                                                   # ... the initializer's iterator, made by the first ask
        self._ask_told = 0                                                      # ... evaluations told so far
        setparams_(acquisition, model)                                          # nlopt_setup :30 (ctor :134)

    # ---- ask / tell (an extension): the caller evaluates, on as many workers as it likes ---------------------------
    def _refuse_ask_tell(self, who):
        from .multigpu import MultiGPE

        for cls in (ConstrainedGPE, MultiObjectiveGPE, MultiGPE):
            if isinstance(self.model, cls):
                raise ValueError(f"BOpt.{who}: a {cls.__name__} with pending evaluations is not built")
        if self.batchsize > 1:
            raise ValueError(f"BOpt.{who}: batchsize = {self.batchsize} with pending evaluations is not built (ask(n) proposes n points)")
        if self.repetitions > 1:
            raise ValueError(f"BOpt.{who}: repetitions = {self.repetitions} with pending evaluations is not built")
        if not hasattr(self.model, "set_pending"):
            raise ValueError(f"BOpt.{who}: {type(self.model).__name__} has no pending set (set_pending)")

    def ask(self, n=1):
        """n points to evaluate next, as a d x n array, while earlier proposals are still out.  While the initializer has points
        left they come from it; after that each point is the maximiser of the acquisition averaged over fantasised outcomes at
        everything that is out (acquire_max_pending with `acquisitionoptions`; its keys "fantasies" and "raise_tau" go there too) and joins the
        model's pending set before the next one is sought, so the n points of one call see each other.  Steps the iteration
        counter once per point.  Report the outcomes with tell, in any order."""
        self._refuse_ask_tell("ask")
        if int(n) != n or n < 1:
            raise ValueError(f"ask: n = {n!r} is not a positive integer")
        if self._ask_init is None:
            self._ask_init = iter(self.initializer) if self.iterations.i == 0 else iter(())
        out = []
        for _ in range(int(n)):
            x = next(self._ask_init, None)
            if x is None:
                self.model.set_pending(self._ask_pending)
                setparams_(self.acquisition, self.model)                         # :184
                with _timeit(self, "acquisition"):
                    _, x = acquire_max_pending(self.acquisition, self.model, self.lowerbounds, self.upperbounds,
                                               self.acquisitionoptions, self.rng, setparams=False)
            x = np.array(x, dtype=np.float64)
            step_(self.iterations)
            self._ask_pending = np.asfortranarray(np.concatenate([self._ask_pending, x.reshape(-1, 1)], axis=1))
            out.append(x)
        self.model.set_pending(self._ask_pending)
        return np.asfortranarray(np.stack(out, axis=1))

    def tell(self, x, y, pending=True):
        """The outcomes y (one per column of x, in the caller's sense) of points that ask handed out.  Each column must equal a
        pending column bit for bit (ValueError otherwise, nothing changed); pending=False takes an unsolicited observation instead.
        Updates the observed optimum, makes ONE model update for all columns, removes the matching pending columns and runs the
        model optimizer at its cadence (once when the initial design is complete, then once per tell)."""
        self._refuse_ask_tell("tell")
        x = np.asarray(x, dtype=np.float64)
        x = x.reshape(-1, 1) if x.ndim == 1 else x
        ys = np.atleast_1d(np.asarray(y, dtype=np.float64)).ravel()
        if x.shape[0] != len(self.lowerbounds) or x.shape[1] != ys.size:
            raise ValueError(f"tell: x must be d x n with one y per column, got x {x.shape} and {ys.size} values")
        keep = list(range(self._ask_pending.shape[1]))
        if pending:
            for j in range(x.shape[1]):
                hit = next((k for k in keep if self._ask_pending[:, k].tobytes() == x[:, j].tobytes()), None)
                if hit is None:
                    raise ValueError(f"tell: column {j} of x is not a pending point (pass pending=False for an unsolicited observation)")
                keep.remove(hit)
        flipped = []
        for j in range(x.shape[1]):
            v = int(self.sense) * float(ys[j])
            if v > int(self.sense) * self.observed_optimum:
                self.observed_optimum, self.observed_optimizer = int(self.sense) * v, np.array(x[:, j])
            flipped.append(v)
        with _timeit(self, "model update"):
            update_(self.model, np.asfortranarray(x), np.array(flipped))
        self._ask_pending = np.asfortranarray(self._ask_pending[:, keep])
        self.model.set_pending(self._ask_pending)
        self._ask_told += x.shape[1]
        if self._ask_told >= len(self.initializer):                                           # (tells of an incomplete initial design fit nothing)
            with _timeit(self, "model hyperparameter optimization"):
                optimizemodel_(self.modeloptimizer, self.model)

    def result(self):
        """What boptimize_ returns, for a run driven by ask / tell: the closing MaxMean search runs on the model itself (pending
        points do not enter it)."""
        self._refuse_ask_tell("result")
        if self.model.nobs > 0 and isinstance(self.acquisition, NoisyExpectedImprovement):
            with _timeit(self, "acquisition"):
                self.model_optimum, self.model_optimizer = _best_site(self.model)
        elif self.model.nobs > 0:
            with _timeit(self, "acquisition"):
                opts = {k: v for k, v in self.acquisitionoptions.items() if k not in ("fantasies", "raise_tau")}
                self.model_optimum, self.model_optimizer = acquire_max(MaxMean(), self.model, self.lowerbounds, self.upperbounds, opts,
                                                                       self.rng)
        self.duration.now = time.time()
        return dict(observed_optimum=self.observed_optimum, observed_optimizer=self.observed_optimizer,
                    model_optimum=int(self.sense) * self.model_optimum, model_optimizer=self.model_optimizer)

    def __repr__(self):                                                          # show :141-157
        s = f"Bayesian Optimization object\n\nmodel:\n{self.model!r}\n\nacquisition:\n{type(self.acquisition).__name__}"
        if self.iterations.i == 0:
            return s + "\n\nNo observation data."
        return (s + f"\n\nobserved optimum: {self.observed_optimum}\nobserved optimizer: {self.observed_optimizer}"
                f"\nmodel optimum: {self.model_optimum}\nmodel optimizer: {self.model_optimizer}"
                f"\niterations: {self.iterations.i}/{self.iterations.N}"
                f"\nduration: {self.duration.now - self.duration.starttime}/{self.duration.duration} s")


def isdone(o):                                                                  # :137
    return _isdone(o.iterations) or _isdone(o.duration)


class _timeit:
    """@mytimeit (src/utils.jl:1-7) with the reference's section names."""

    def __init__(self, o, name):
        self.o, self.name = o, name

    def __enter__(self):
        self.t = time.perf_counter()

    def __exit__(self, *a):
        rec = self.o.timeroutput.setdefault(self.name, [0, 0.0])
        rec[0] += 1
        rec[1] += time.perf_counter() - self.t


def _evaluate_constrained(o, x):
    """func(x) -> (y, g_1, ..., g_C) for a ConstrainedGPE: sense flips y only, and only a feasible observation can be the optimum."""
    with _timeit(o, "function evaluation"):
        out = np.atleast_1d(np.asarray(o.func(x), dtype=np.float64)).ravel()
    C_ = len(o.model.constraints)
    if out.size != C_ + 1:
        raise ValueError(f"func must return (y, g_1, ..., g_C) with C = {C_} constraint values, got {out.size} numbers")
    y, g = int(o.sense) * float(out[0]), out[1:]
    if bool(o.model.is_feasible(g)) and y > int(o.sense) * o.observed_optimum:
        o.observed_optimum = int(o.sense) * y
        o.observed_optimizer = x
    return y, g


def _evaluate_two(o, x):
    """func(x) -> (y_1, y_2) for a MultiObjectiveGPE, (y_1, .., y_M) for a ManyObjectiveGPE: sense flips all; there is no optimum to
    track."""
    with _timeit(o, "function evaluation"):
        out = np.atleast_1d(np.asarray(o.func(x), dtype=np.float64)).ravel()
    M = len(o.model.objectives)
    if M != 2 and out.size != M:
        raise ValueError(f"func must return (y_1, .., y_{M}), the {M} objectives' values, got {out.size} numbers")
    if out.size != 2 and M == 2:
        raise ValueError(f"func must return (y_1, y_2), the two objectives' values, got {out.size} numbers")
    return int(o.sense) * out


def _update_model(o, xs, ys):
    """One model update with the columns xs and what _evaluate_function returned for them."""
    if isinstance(o.model, MultiObjectiveGPE):
        o.model.update_(np.stack(xs, axis=1), np.stack(ys, axis=1))
    elif isinstance(o.model, ConstrainedGPE):
        o.model.update_(np.stack(xs, axis=1), np.array([y for y, _ in ys]), np.stack([g for _, g in ys], axis=1))
    else:
        update_(o.model, np.stack(xs, axis=1), np.array(ys))


def _evaluate_function(o, x):                                                   # :209-216
    if isinstance(o.model, ConstrainedGPE):
        return _evaluate_constrained(o, x)
    if isinstance(o.model, MultiObjectiveGPE):
        return _evaluate_two(o, x)
    with _timeit(o, "function evaluation"):
        y = int(o.sense) * o.func(x)
    if y > int(o.sense) * o.observed_optimum:
        o.observed_optimum = int(o.sense) * y
        o.observed_optimizer = x
    return y


def initialise_model_(o):                                                       # :159-172
    ys, xs = [], []
    for x in o.initializer:
        for _ in range(o.repetitions):
            ys.append(_evaluate_function(o, x))
            xs.append(x)
    o.iterations.i = o.iterations.c = len(ys) // o.repetitions
    with _timeit(o, "model update"):
        _update_model(o, xs, ys)
    with _timeit(o, "model hyperparameter optimization"):
        optimizemodel_(o.modeloptimizer, o.model)


def _batch_iteration(o):
    """One iteration with batchsize > 1: ONE acquire_batch (ThompsonSamplingSimple: ONE acquire_thompson_batch), `repetitions` evaluations of each of its points, ONE model update
    with all columns, one step of the iteration counter."""
    with _timeit(o, "acquisition"):
        if isinstance(o.acquisition, ThompsonSamplingSimple):                    # `batchsize` joint posterior draws, distinct winners
            _, X = acquire_thompson_batch(o.model, o.lowerbounds, o.upperbounds, o.batchsize, o.batchoptions, o.rng)
        else:
            _, X = acquire_batch(o.acquisition, o.model, o.lowerbounds, o.upperbounds, o.batchsize, o.batchoptions, o.rng,
                                 setparams=False)
    step_(o.iterations)
    xs, ys = [], []
    for j in range(X.shape[1]):
        x = np.array(X[:, j])
        for _ in range(o.repetitions):
            ys.append(_evaluate_function(o, x))
            xs.append(x)
    if not xs:                                                                   # (no candidate had a finite score: acquire_batch has warned)
        return
    with _timeit(o, "model update"):
        update_(o.model, np.stack(xs, axis=1), np.array(ys))
    with _timeit(o, "model hyperparameter optimization"):
        optimizemodel_(o.modeloptimizer, o.model)


def _best_site(model):
    """(mean, site): the observed site with the largest posterior mean and that mean -- what a run under NoisyExpectedImprovement
    reports as model_optimum / model_optimizer (the first such site on a tie).  The largest raw observation (observed_optimum) is the
    luckiest noise draw; this is the model's answer to "which of the points I tried is best"."""
    mu, _ = model.predict_f(model.x)
    j = int(np.argmax(mu))
    return float(mu[j]), np.array(model.x[:, j])


def boptimize_(o):
    """boptimize!(o) :176-207.  Re-calling resumes: init! zeroes the per-call counter but keeps the cumulative one."""
    init_(o.duration)
    init_(o.iterations)
    o.timeroutput.clear()
    if o.iterations.i == 0 and len(o.initializer) > 0:
        initialise_model_(o)
    while not isdone(o):
        if o.verbosity >= Progress:
            print(f"{time.strftime('%Y-%m-%dT%H:%M:%S')}\titeration: {o.iterations.i}\tcurrent optimum: {o.observed_optimum}")
        setparams_(o.acquisition, o.model)                                       # :184
        if o.batchsize > 1:
            _batch_iteration(o)
            continue
        with _timeit(o, "acquisition"):
            f, x = acquire_max(o.acquisition, o.model, o.lowerbounds, o.upperbounds, o.acquisitionoptions, o.rng,
                               setparams=False)                                  # :185 (4-argument method: no second setparams!)
        ys = []
        step_(o.iterations)
        for _ in range(o.repetitions):
            ys.append(_evaluate_function(o, x))
        with _timeit(o, "model update"):
            _update_model(o, [x] * o.repetitions, ys)                             # :194-196
        with _timeit(o, "model hyperparameter optimization"):
            optimizemodel_(o.modeloptimizer, o.model)
    with _timeit(o, "acquisition"):
        if isinstance(o.model, ConstrainedGPE):                                   # (no unconstrained model maximum: the feasible optimum stands)
            o.model_optimum, o.model_optimizer = int(o.sense) * o.observed_optimum, np.array(o.observed_optimizer)
        elif o.model.nobs > 0 and isinstance(o.acquisition, NoisyExpectedImprovement):   # (noisy evaluations: the best SITE under the model)
            o.model_optimum, o.model_optimizer = _best_site(o.model)
        elif o.model.nobs > 0 and not isinstance(o.model, MultiObjectiveGPE):     # (two objectives: no single optimum, the result carries the front)
            o.model_optimum, o.model_optimizer = acquire_max(MaxMean(), o.model, o.lowerbounds, o.upperbounds,
                                                             o.acquisitionoptions, o.rng)   # acquire_model_max :200
    o.duration.now = time.time()
    if o.verbosity >= Timings:
        for k, (n, t) in o.timeroutput.items():
            print(f"  {k:40s} calls {n:6d}  {t:10.4f} s")
    if isinstance(o.model, MultiObjectiveGPE):
        return _two_objective_result(o)
    return dict(observed_optimum=o.observed_optimum, observed_optimizer=o.observed_optimizer,
                model_optimum=int(o.sense) * o.model_optimum, model_optimizer=o.model_optimizer)   # :203-206


def _two_objective_result(o):
    """The result of a run with M = 2 (or, on a ManyObjectiveGPE, 2 to 4) objectives: the observed front as x [d, n_front] and y
    [M, n_front] in the caller's sense (in the model's order: ascending in its first objective, lexicographic beyond two), the
    hypervolume it dominates above the model's reference point (`ref`, in the caller's sense too), and None where a single-objective
    run reports an optimum."""
    m = o.model
    if m.nobs == 0:
        front_x, front_y, hv, ref = np.zeros((m.dim, 0)), np.zeros((len(m.objectives), 0)), 0.0, None
    else:
        idx = m.front_indices()
        front_x, front_y, hv = np.array(m.x[:, idx]), int(o.sense) * m.y[:, idx], m.hypervolume
        ref = int(o.sense) * m.reference_point()
    return dict(observed_optimum=None, observed_optimizer=None, model_optimum=None, model_optimizer=None,
                observed_front=dict(x=front_x, y=front_y), hypervolume=hv, ref=ref)


def merge_with_defaults(f, lowerbounds, upperbounds, optkwargs):                # :238-289
    args_keys = ("model", "acquisition", "modeloptimizer")
    kwargs_keys = ("sense", "maxiterations", "maxduration", "acquisitionoptions", "repetitions", "verbosity",
                   "initializer_iterations", "initializer", "batchsize", "batchoptions")
    if not set(optkwargs) <= set(args_keys) | set(kwargs_keys):
        raise ValueError("use of unsupported keyword arguments")                 # ArgumentError :250-251
    if len(lowerbounds) != len(upperbounds):
        raise ValueError("length of lowerbounds does not match length of upperbounds")
    inputdimension = len(lowerbounds)
    params = dict(optkwargs)
    if "model" not in params:                                                    # :259-264
        params["model"] = ElasticGPE(inputdimension, mean=MeanConst(0.0),
                                     kernel=Mat52Ard(np.zeros(inputdimension), 0.0), logNoise=-2.0, capacity=3000)
    if "acquisition" not in params:
        params["acquisition"] = ExpectedImprovement()
    if "modeloptimizer" not in params:                                           # :266-272
        params["modeloptimizer"] = MAPGPOptimizer(every=20, noisebounds=[-4, 3],
                                                  kernbounds=[[-3.0] * inputdimension + [-3.0], [4.0] * inputdimension + [3.0]],
                                                  maxeval=100)
    params.setdefault("maxiterations", 10 ** 3)
    args = (f, *[params[k] for k in args_keys], lowerbounds, upperbounds)
    kwargs = {k: v for k, v in params.items() if k in kwargs_keys}
    return args, kwargs


def optimize(f, lowerbounds, upperbounds, **optkwargs):                         # :230-234
    args, kwargs = merge_with_defaults(f, lowerbounds, upperbounds, optkwargs)
    return boptimize_(BOpt(*args, **kwargs))
