"""Acquisition types and the multi-restart search, mirroring reference src/acquisitionfunctions.jl and
src/acquisition.jl.  The functors keep the reference's formulas verbatim (host versions, used for single
points and documentation); batches are scored on the device through ``model.score``.

Where the reference runs R sequential NLopt ascents (src/acquisition.jl:58-66), ``acquire_max`` scores /
ascends ALL R Latin-hypercube starts together on the GPU:
    method :LD_*  -> batched projected L-BFGS driven by the device's analytic gradient (score_grad)
    method :GN_* / :LN_* -> derivative-free: ``maxeval`` candidates scored in one batch
"""
from __future__ import annotations

import math
import warnings
from types import SimpleNamespace

import numpy as np

from .model import ElasticGPE, dims, maxy, mean_var, myrand
from .utils import latin_hypercube_sampling, normal_cdf, normal_pdf


class AbstractAcquisition:
    acq_id = None

    def params(self):
        return []


def setparams_(a, model):                                     # setparams!(a, model) = nothing :3
    f = getattr(a, "_setparams", None)
    return f(model) if f else None


class ProbabilityOfImprovement(AbstractAcquisition):          # :21-28
    acq_id = "PI"

    def __init__(self, tau=-math.inf):
        self.tau = float(tau)

    def __call__(self, mu, s2):
        if s2 == 0:
            return float(mu > self.tau)
        return normal_cdf(mu - self.tau, s2)

    def _setparams(self, model):                              # :44-46
        self.tau = max(maxy(model), self.tau)
        return self.tau

    def params(self):
        return [self.tau]


class ExpectedImprovement(AbstractAcquisition):               # :40-50
    acq_id = "EI"

    def __init__(self, tau=-math.inf):
        self.tau = float(tau)

    def __call__(self, mu, s2):
        if s2 == 0:
            return mu - self.tau if mu > self.tau else 0.0
        return (mu - self.tau) * normal_cdf(mu - self.tau, s2) + math.sqrt(s2) * normal_pdf(mu - self.tau, s2)

    _setparams = ProbabilityOfImprovement._setparams
    params = ProbabilityOfImprovement.params


class LogExpectedImprovement(AbstractAcquisition):
    """The logarithm of the TEXTBOOK expected improvement, log(Delta Phi(z) + sigma phi(z)), in forms that stay finite and accurate
    for any z = (mu - tau) / sigma (csrc/acq_log.h; Ament et al., NeurIPS 2023).  An extension: the reference has no
    such type, and no default uses it.  Its arg-max is that of the textbook EI and its gradient never vanishes, where
    ExpectedImprovement and its gradient are exactly 0.0 from z ~ -38 down.  `partials` returns (d/dmu, d/dsigma^2)."""
    acq_id = "LogEI"
    SWITCH, CF_DEPTH = -4.0, 40

    def __init__(self, tau=-math.inf):
        self.tau = float(tau)

    @classmethod
    def _parts(cls, z):
        """(log h, Phi / h, phi / h) of h(z) = phi(z) + z Phi(z): direct above SWITCH, Mills' ratio by its continued fraction below."""
        z = np.asarray(z, dtype=np.float64)
        with np.errstate(all="ignore"):
            zz = np.where(z > cls.SWITCH, z, 0.0)
            phi = 0.3989422804014327 * np.exp(-0.5 * (zz * zz))
            Phi = 0.5 * _erfc(-zz / 1.4142135623730951)
            h = phi + zz * Phi
            t = np.where(z > cls.SWITCH, 4.0, -z)
            r = np.zeros_like(t)
            for k in range(cls.CF_DEPTH, 1, -1):
                r = float(k) / (t + r)
            tr = t + r
            c1 = 1.0 / tr
            tc = t + c1
            lo = (-0.5 * (z * z) - 0.9189385332046728 + np.log(c1 / tc), tr, tc * tr)
            hi = (np.log(h), Phi / h, phi / h)
            return tuple(np.where(z > cls.SWITCH, a, b) for a, b in zip(hi, lo))

    def __call__(self, mu, s2):
        mu, s2 = np.asarray(mu, dtype=np.float64), np.asarray(s2, dtype=np.float64)
        with np.errstate(all="ignore"):
            D = mu - self.tau
            s = np.sqrt(np.where(s2 == 0, 1.0, s2))
            v = np.where(s2 == 0, np.where(D > 0, np.log(np.where(D > 0, D, 1.0)), -math.inf), np.log(s) + self._parts(D / s)[0])
        return float(v) if v.ndim == 0 else v

    def partials(self, mu, s2):
        mu, s2 = np.asarray(mu, dtype=np.float64), np.asarray(s2, dtype=np.float64)
        with np.errstate(all="ignore"):
            D = mu - self.tau
            ok = np.where(s2 == 0, 1.0, s2)
            s = np.sqrt(ok)
            _, a, b = self._parts(D / s)
            dmu = np.where(s2 == 0, np.where(D > 0, 1.0 / np.where(D > 0, D, 1.0), 0.0), a / s)
            ds2 = np.where(s2 == 0, 0.0, b / (2.0 * ok))
        return (float(dmu), float(ds2)) if dmu.ndim == 0 else (dmu, ds2)

    _setparams = ProbabilityOfImprovement._setparams          # EI's rule: tau <- max(maxy, tau)
    params = ProbabilityOfImprovement.params


class KnowledgeGradient(AbstractAcquisition):
    """The knowledge gradient over a candidate set (include/bohip_kg.h; Frazier, Powell & Dayanik 2009): the expected
    rise of max_j mu_j over the candidates after ONE noisy observation at the point, computed exactly on the device (model.kg).  An
    extension: the reference has no such type, and no default uses it.  It is not a functor of one point's (mu, sigma^2) -- it ranks
    a point by what observing it would teach about the optimum -- so it has no parameters, no gradient and no place in score /
    ascend / DIRECT: acquisitionfunction takes a d x R candidate matrix, and acquire_max takes the arg-max over `maxeval`
    Latin-hypercube candidates per restart (each set evaluated against itself)."""
    acq_id = "KG"


class MaxValueEntropySearch(AbstractAcquisition):
    """Max-value entropy search over a candidate set (include/bohip_mes.h; Wang & Jegelka 2017): the information the
    observation of a point gives about the VALUE of the optimum, averaged over `samples` draws of the maximum of the posterior over
    the candidates (model.mes).  An extension: the reference has no such type, and no default uses it.  mode "gumbel" fits a Gumbel
    law to three quantiles of the maximum of independent candidates; "joint" takes the row maxima of joint posterior draws.  The
    maximum is that of a SET, so acquisitionfunction takes a d x R candidate matrix, and acquire_max takes the device's arg-max over
    `maxeval` Latin-hypercube candidates per restart; no gradient in x, no place in score / ascend / DIRECT."""
    acq_id = "MES"
    MODES = ("gumbel", "joint")

    def __init__(self, samples=16, mode="gumbel"):
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= 1024:
            raise ValueError(f"samples must be an integer in 1 .. 1024 (BOHIP_MES_KMAX), got {samples!r}")
        if mode not in self.MODES:
            raise ValueError(f"mode must be one of {self.MODES}, got {mode!r}")
        self.samples, self.mode = int(samples), mode


class NoisyExpectedImprovement(AbstractAcquisition):
    """Noisy expected improvement (include/bohip_nei.h; Letham, Karrer, Ottoni & Bakshy 2019, eq. 6): EI -- with
    log=True LogEI's log of the averaged EI -- averaged over S posterior draws of the NOISE-FREE function values at the observed
    sites.  Every draw brings its own incumbent, so the largest raw observation (the luckiest noise draw) plays no part.  S = 0:
    the plug-in form, whose incumbent is the largest posterior mean at the sites.  An extension: the reference has no such type,
    and no default uses it.  It has no parameter that follows the model (setparams_ does nothing) and no gradient in x:
    acquisitionfunction takes a point or a d x R matrix, acquire_max takes the device's arg-max over `maxeval` Latin-hypercube
    candidates per restart.  `seed` fixes the draws, so the acquisition is one deterministic function of x during a search."""
    acq_id = "NEI"

    def __init__(self, S=32, seed=0, log=False, jitter_rel=1e-8):
        if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 0 <= S <= 1024:
            raise ValueError(f"S must be an integer in 0 .. 1024 (BOHIP_NEI_SMAX), got {S!r}")
        if not (jitter_rel > 0 and math.isfinite(jitter_rel)):
            raise ValueError(f"jitter_rel must be positive and finite, got {jitter_rel!r}")
        self.S, self.seed, self.log, self.jitter_rel = int(S), int(seed), bool(log), float(jitter_rel)

    def score(self, model, xs, want_scores=True):
        if not hasattr(model, "nei"):
            raise NotImplementedError(f"{type(model).__name__} has no nei")
        return model.nei(xs, S=self.S, seed=self.seed, acq="logei" if self.log else "ei", jitter_rel=self.jitter_rel,
                         want_scores=want_scores)


class Marginalised(AbstractAcquisition):
    """Marginalised(a): the acquisition `a` averaged over the hyper-parameter samples that MarginalGPOptimizer left on the model
    (model.hyper_samples = (Theta[H, P], weights)): a(x) = sum_h w_h a(x; theta_h), the integrated acquisition of Snoek, Larochelle &
    Adams 2012 (include/bohip_ens.h).  An extension: the reference has no such type, and no default uses it.  `a` is
    one of the functors of (mu, sigma^2): ExpectedImprovement, ProbabilityOfImprovement, UpperConfidenceBound, MutualInformation,
    MaxMean, LogExpectedImprovement.  setparams_ forwards to `a` (tau = max y, UCB's beta schedule, MI's gamma-hat: all taken
    under the model's own, highest-likelihood setting).  VALUE ONLY by default: acquisitionfunction maps a d x R matrix to the
    averaged scores (model.score_ensemble), and acquire_max takes the arg-max over `maxeval` Latin-hypercube candidates per restart.
    With the option "refine": n > 0 the n best candidates are then climbed by the batched L-BFGS ascent on the gradient of the average
    (model.score_ensemble_grad, include/bohip_ens_grad.h).  "refine" belongs to this type alone: every other
    acquisition accepts the key unused (BOpt shares one options record with its MaxMean search)."""
    TAKES = ("EI", "PI", "UCB", "MI", "MaxMean", "LogEI")

    def __init__(self, a):
        if not isinstance(a, AbstractAcquisition) or a.acq_id not in self.TAKES:
            raise ValueError(f"Marginalised takes an acquisition of (mu, sigma^2) -- {', '.join(self.TAKES)} -- not "
                             f"{type(a).__name__}")
        self.a = a
        self.acq_id = a.acq_id

    def _setparams(self, model):
        return setparams_(self.a, model)

    def params(self):
        return self.a.params()


class Constrained(AbstractAcquisition):
    """Constrained(a): the acquisition `a` of the objective weighted by the probability that every constraint of a ConstrainedGPE
    holds (include/bohip_con.h; Gardner et al. 2014, Gelbart, Snoek & Adams 2014).  An extension: the reference's
    acquisition closes over one model.  `a` is ExpectedImprovement or ProbabilityOfImprovement (a exp(L), the classic product) or
    LogExpectedImprovement (a + L, which survives deep infeasibility); L = sum_c log P(constraint c holds).  setparams_ sets tau to
    the best FEASIBLE observation; while there is none the call scores L alone ("Feasibility": Gelbart's rule -- look for a feasible
    point first).  acquisitionfunction takes a d x R matrix; acquire_max takes the device's arg-max over `maxeval` Latin-hypercube
    candidates per restart and, with the option "refine": n > 0, climbs the n best on the gradient route."""
    TAKES = ("EI", "PI", "LogEI")

    def __init__(self, a):
        if not isinstance(a, AbstractAcquisition) or a.acq_id not in self.TAKES:
            raise ValueError(f"Constrained takes ExpectedImprovement, ProbabilityOfImprovement or LogExpectedImprovement, not "
                             f"{type(a).__name__}: a signed score has no product form")
        self.a = a
        self.feasibility_only = False

    @property
    def acq_id(self):
        return "Feasibility" if self.feasibility_only else self.a.acq_id

    def _setparams(self, model):
        inc = model.feasible_incumbent()
        self.feasibility_only = inc is None
        if inc is not None:
            self.a.tau = float(inc)
        return self.a.tau

    def params(self):
        return [0.0] if self.feasibility_only else self.a.params()


class ExpectedHypervolumeImprovement(AbstractAcquisition):
    """The exact expected hypervolume improvement of two objectives over the observed front of a MultiObjectiveGPE
    (include/bohip_mo.h; Emmerich et al. 2016, Yang et al. 2019).  An extension: the reference optimises one objective.
    It has no parameter of its own: the front and the reference point are the model's.  Over a ManyObjectiveGPE (2 to 4 objectives) it
    is the sum over the boxes of the front (include/bohip_mom.h).  acquisitionfunction takes a d x R matrix;
    acquire_max takes the device's arg-max over `maxeval` Latin-hypercube candidates per restart and, with the option "refine": n > 0,
    climbs the n best on the gradient route."""
    acq_id = "EHVI"


def _hyper_samples(model):
    hs = getattr(model, "hyper_samples", None)
    if hs is None:
        raise ValueError("Marginalised needs model.hyper_samples: fit the model with MarginalGPOptimizer (or set "
                         "model.hyper_samples = (Theta, weights)) first")
    return hs


def _erfc(x):
    from scipy.special import erfc                             # (vectorised; math.erfc is its scalar form)

    return erfc(x)


class BrochuBetaScaling:                                      # :66-68
    def __init__(self, delta=0.1):
        self.delta = float(delta)


class NoBetaScaling:                                          # :72
    pass


class UpperConfidenceBound(AbstractAcquisition):              # :81-96
    acq_id = "UCB"

    def __init__(self, scaling=None, beta_t=1.0):
        self.scaling = scaling if scaling is not None else BrochuBetaScaling(0.1)
        self.beta_t = float(beta_t)

    def __call__(self, mu, s2):
        return mu + self.beta_t * math.sqrt(s2)

    def _setparams(self, model):                              # :91-95 (BrochuBetaScaling only)
        if isinstance(self.scaling, BrochuBetaScaling):
            D, nobs = dims(model)
            nobs = 1 if nobs == 0 else nobs
            self.beta_t = math.sqrt(2 * math.log(nobs ** (D / 2 + 2) * math.pi ** 2 / (3 * self.scaling.delta)))
        return self.beta_t

    def params(self):
        return [self.beta_t]


class ThompsonSamplingSimple(AbstractAcquisition):            # :107-108
    acq_id = "Thompson"


class MaxMean(AbstractAcquisition):                           # :110-111
    acq_id = "MaxMean"

    def __call__(self, mu, s2):
        return mu


class MutualInformation(AbstractAcquisition):                 # :126-141
    acq_id = "MI"

    def __init__(self, alpha=1.0, gamma_hat=0.0):
        self.sqrt_alpha = math.sqrt(alpha)
        self.gamma_hat = float(gamma_hat)

    def __call__(self, mu, s2):
        return mu + self.sqrt_alpha * (math.sqrt(s2 + self.gamma_hat) - math.sqrt(self.gamma_hat))

    def _setparams(self, model):                              # :131-140
        D, nobs = dims(model)
        if nobs == 0:
            self.gamma_hat = 0.0
        else:
            last_x = model.x[:, -1]
            _, s2 = mean_var(model, last_x)
            self.gamma_hat += s2
        return self.gamma_hat

    def params(self):
        return [self.sqrt_alpha, self.gamma_hat]


def _need_mo(model):
    if not hasattr(model, "hypervolume"):
        raise ValueError(f"ExpectedHypervolumeImprovement needs a MultiObjectiveGPE, not {type(model).__name__}")


def acquisitionfunction(a, model, rng=None):
    """:4-9, :108, :111.  x (vector or d x R matrix) -> score(s); batches run fused on the device."""
    if isinstance(a, KnowledgeGradient):
        def kg(x):
            x = np.asarray(x, dtype=np.float64)
            if x.ndim != 2:
                raise ValueError("KnowledgeGradient needs a candidate set, a d x R matrix: the knowledge gradient of one point "
                                 "against itself is 0")
            return model.kg(x).values

        return kg
    if isinstance(a, MaxValueEntropySearch):
        def mes(x):
            x = np.asarray(x, dtype=np.float64)
            if x.ndim != 2:
                raise ValueError("MaxValueEntropySearch needs a candidate set, a d x R matrix: the maximum it learns about is that "
                                 "of a set")
            seed = int((rng if rng is not None else np.random.default_rng()).integers(0, 2**63))
            return model.mes(x, samples=a.samples, mode=a.mode, seed=seed).values

        return mes
    if isinstance(a, NoisyExpectedImprovement):
        def nei(x):
            x = np.asarray(x, dtype=np.float64)
            sc = a.score(model, x).score
            return float(sc[0]) if x.ndim == 1 else sc

        return nei
    if isinstance(a, Constrained):
        def constrained(x):
            x = np.asarray(x, dtype=np.float64)
            if x.ndim != 2:
                raise ValueError("Constrained takes a d x R candidate matrix")
            return model.score(a.acq_id, a.params(), x).scores

        return constrained
    if isinstance(a, ExpectedHypervolumeImprovement):
        _need_mo(model)

        def ehvi(x):
            x = np.asarray(x, dtype=np.float64)
            if x.ndim != 2:
                raise ValueError("ExpectedHypervolumeImprovement takes a d x R candidate matrix")
            return model.score(x).scores

        return ehvi
    if isinstance(a, Marginalised):
        def marginal(x):
            x = np.asarray(x, dtype=np.float64)
            Theta, w = _hyper_samples(model)
            sc = model.score_ensemble(a.acq_id, a.params(), x, Theta, w).scores
            return float(sc[0]) if x.ndim == 1 else sc

        return marginal
    if isinstance(a, ThompsonSamplingSimple):
        return lambda x: myrand(model, x, rng)
    if isinstance(a, MaxMean):
        return lambda x: mean_var(model, x)[0]

    def f(x):
        x = np.asarray(x, dtype=np.float64)
        sc, _, _ = model.score(a.acq_id, a.params(), x)
        return float(sc[0]) if x.ndim == 1 else sc

    return f


# ---- src/acquisition.jl ----------------------------------------------------------------------------------
def defaultoptions(model_type, acq_type):                    # :4-9
    if isinstance(acq_type, type) and issubclass(acq_type, (KnowledgeGradient, MaxValueEntropySearch, Constrained,
                                                                     ExpectedHypervolumeImprovement, NoisyExpectedImprovement)):
        return dict(method="LD_LBFGS", restarts=1, maxeval=1024)   # (1024: the smallest candidate chunk a model can have)
    if isinstance(acq_type, type) and issubclass(acq_type, ThompsonSamplingSimple):
        return dict(method="GN_DIRECT_L", restarts=1, maxeval=2000)
    return dict(method="LD_LBFGS", restarts=10, maxeval=2000)


ASC_MAX_BT = 30   # kernels_ascent.hip: trial points per line search


def _batched_lbfgs_ascent(fg, X0, lb, ub, maxeval, ftol_rel=1e-10, xtol_abs=1e-10, history=8, ftol_abs=0.0, xtol_rel=0.0,
                          stopval=math.inf):
    """Lock-step projected L-BFGS ascent of R independent d-dimensional problems (role of NLopt :LD_LBFGS
    with lower/upper bounds, src/acquisition.jl:23-35).  fg(X) -> (f[R], G[d,R]) is ONE device call.
    Returns (f, X) at the best point seen per column."""
    d, R = X0.shape
    lbc, ubc = lb.reshape(-1, 1), ub.reshape(-1, 1)
    X = np.clip(X0, lbc, ubc)
    f, G = fg(X)
    evals = 1
    S, Y = [], []
    active = np.isfinite(f)
    best_f, best_X = f.copy(), X.copy()
    while evals < maxeval and active.any():
        # two-loop recursion, vectorised over columns, in the FREE SUBSPACE of every column: a coordinate on a bound with the gradient
        # pushing outward takes no part (kernels_ascent.hip asc_direction_one: 22-35 passes instead of 228-309 on the headline model,
        # where UCB peaks in the corners of the box; with no bound active the arithmetic is unchanged)
        free = ~(((X <= lbc) & (G < 0)) | ((X >= ubc) & (G > 0)))
        q = np.where(free, G, 0.0)
        al = []
        for s_, y_ in zip(reversed(S), reversed(Y)):
            s_, y_ = np.where(free, s_, 0.0), np.where(free, y_, 0.0)
            sy = np.einsum("dr,dr->r", y_, s_)
            rho = np.where(sy > 1e-14, 1.0 / np.where(sy > 1e-14, sy, 1.0), 0.0)     # a pair without curvature in the free subspace is skipped
            a_ = rho * np.einsum("dr,dr->r", s_, q)
            q -= a_ * y_
            al.append((a_, rho))
        if S:
            s_, y_ = np.where(free, S[-1], 0.0), np.where(free, Y[-1], 0.0)
            sy = np.einsum("dr,dr->r", s_, y_)
            yy = np.maximum(np.einsum("dr,dr->r", y_, y_), 1e-300)
            q *= np.where(sy > 1e-14, sy / yy, 1.0)
        for (a_, rho), s_, y_ in zip(reversed(al), S, Y):
            s_, y_ = np.where(free, s_, 0.0), np.where(free, y_, 0.0)
            b_ = rho * np.einsum("dr,dr->r", y_, q)
            q += (a_ - b_) * s_
        D = q                                                     # ascent direction (maximisation: H * grad)
        # bounds: do not push active constraints outward; fall back to the gradient if not an ascent direction
        blocked = ((X <= lbc) & (D < 0)) | ((X >= ubc) & (D > 0))
        D = np.where(blocked, 0.0, D)
        Gp = np.where(((X <= lbc) & (G < 0)) | ((X >= ubc) & (G > 0)), 0.0, G)
        slope = np.einsum("dr,dr->r", Gp, D)
        bad = ~(slope > 0)
        D[:, bad] = Gp[:, bad]
        slope = np.einsum("dr,dr->r", Gp, D)
        if S:
            step = np.ones(R)
        else:                                                     # the FIRST step (kernels_ascent.hip asc_direction_one): L-BFGS-B's unit step to P(x + g),
            span = (ub - lb)[np.isfinite(ub - lb)]                # (a box without a finite side -- the MAP fit's log-parameters -- keeps the unit step)
            box = np.min(span + 1e-300) if span.size else 0.0
            step = np.maximum(1.0, 0.1 * box / np.maximum(np.sqrt(np.einsum("dr,dr->r", D, D)), 1e-12))   # but never shorter than a tenth of the box
        step = np.where(active & (slope > 0), step, 0.0)
        accepted = ~active | ~(slope > 0)
        Xn, fn, Gn = X.copy(), f.copy(), G.copy()
        for _ in range(ASC_MAX_BT):                               # backtracking Armijo, all columns per device call
            Xt = np.clip(X + step * D, lbc, ubc)
            ft, Gt = fg(Xt)
            evals += 1
            ok = (~accepted) & np.isfinite(ft) & (ft >= f + 1e-4 * np.einsum("dr,dr->r", Gp, Xt - X))
            Xn[:, ok], fn[ok], Gn[:, ok] = Xt[:, ok], ft[ok], Gt[:, ok]
            accepted |= ok
            if accepted.all() or evals >= maxeval:
                break
            step = np.where(accepted, step, step * 0.5)
        s_ = Xn - X
        y_ = -(Gn - G)                                            # curvature pair for maximisation
        df = fn - f
        moved = np.sqrt(np.einsum("dr,dr->r", s_, s_))
        active = active & (df > ftol_rel * np.maximum(np.abs(fn), 1e-300)) & (moved > xtol_abs)
        # NLopt's other stop tests (kernels_ascent.hip asc_goes_on): ftol_abs, xtol_rel per coordinate, stopval
        active = active & (df > ftol_abs) & ~(fn >= stopval)
        if xtol_rel > 0.0:
            active = active & (np.abs(s_) > xtol_rel * np.abs(Xn)).any(axis=0)
        good = np.einsum("dr,dr->r", s_, y_) > 1e-14
        S.append(np.where(good, s_, 0.0)); Y.append(np.where(good, y_, 0.0))
        if len(S) > history:
            S.pop(0); Y.pop(0)
        X, f, G = Xn, fn, Gn
        better = f > best_f
        best_f[better], best_X[:, better] = f[better], X[:, better]
    return best_f, best_X


def _batched_direct_l(f_batch, lb, ub, maxeval, stopval=math.inf, maxtime=0.0):
    """DIviding RECTangles, locally biased (Gablonsky & Kelley 2001) -- the role of NLopt's :GN_DIRECT_L, which the reference uses
    by default for ThompsonSamplingSimple (src/acquisition.jl:7-9: restarts = 1, maxeval = 2000) -- for MAXIMISATION, with ALL the
    new points of one iteration evaluated in ONE device call: f_batch(X[d, n]) -> f[n].
    The rules are those of NLopt's cdirect.c for this algorithm (its `which_alg = 13`): a rectangle's size is its longest side, the
    potentially optimal set is the upper convex hull of (size, best value of that size) from the incumbent's size up with ONE
    rectangle per size (Jones' epsilon = 0), a cube is trisected along every side -- best sampled value first, so the best points
    end up in the largest boxes -- and any other rectangle along its first longest side only.  What is NOT reproduced is NLopt's
    evaluation ORDER inside an iteration (irrelevant for a deterministic objective, a different random stream for a sampled one).
    `maxtime` > 0: NLopt's wall-clock budget in seconds (the reference's test passes it; checked once per iteration).
    Returns (best value, best point, evaluations)."""
    import time

    deadline = time.monotonic() + maxtime if maxtime and maxtime > 0 else math.inf
    lb = np.asarray(lb, float); ub = np.asarray(ub, float)
    d = lb.size
    span = ub - lb
    to_x = lambda U: lb[:, None] + span[:, None] * U              # noqa: E731  unit cube -> box, columns are points
    C = np.full((d, 1), 0.5)                                      # centres (unit cube)
    Lv = np.zeros((d, 1), dtype=np.int64)                         # level per side: side length 3^-level
    F = np.asarray(f_batch(to_x(C)), float).reshape(-1)
    F = np.where(np.isnan(F), -math.inf, F)
    evals = 1
    while evals < maxeval and not (F.max() >= stopval) and time.monotonic() < deadline:
        size = Lv.min(axis=0)                                     # key of the longest side (smaller = larger rectangle)
        keys = np.unique(size)
        best_of = {}
        for k in keys:                                            # one rectangle per size: the best, first on ties
            idx = np.flatnonzero(size == k)
            best_of[int(k)] = int(idx[np.argmax(F[idx])])
        jmax = int(np.argmax(F))
        # upper hull over (diameter, f) from the incumbent's size towards the larger rectangles
        cand = sorted((k for k in best_of if k <= size[jmax]), reverse=True)          # increasing diameter
        hull = []
        for k in cand:
            pt = (3.0 ** (-k), F[best_of[k]], best_of[k])
            while len(hull) >= 2:
                (x1, y1, _), (x2, y2, _) = hull[-2], hull[-1]
                if (y2 - y1) * (pt[0] - x1) <= (pt[1] - y1) * (x2 - x1):             # the middle point is not above the chord
                    hull.pop()
                else:
                    break
            hull.append(pt)
        chosen = [j for _, _, j in hull]                          # (the first one is the incumbent's own size class)
        # new points of this iteration (capped by the evaluation budget)
        plan, cols = [], []
        for j in chosen:
            lv = Lv[:, j]
            kmin = lv.min()
            longest = np.flatnonzero(lv == kmin)
            dims = longest if longest.size == d else longest[:1]   # a cube: every side; otherwise the first longest side
            if evals + len(cols) + 2 * len(dims) > maxeval:
                dims = dims[: max(0, (maxeval - evals - len(cols)) // 2)]
            if len(dims) == 0:
                continue
            delta = 3.0 ** (-(kmin + 1))
            start = len(cols)
            for i in dims:
                for sgn in (+1.0, -1.0):
                    c = C[:, j].copy(); c[i] += sgn * delta
                    cols.append(c)
            plan.append((j, dims, start))
        if not cols:
            break
        Unew = np.array(cols).T
        Fnew = np.asarray(f_batch(to_x(Unew)), float).reshape(-1)
        Fnew = np.where(np.isnan(Fnew), -math.inf, Fnew)
        evals += Fnew.size
        newL = np.empty((d, Fnew.size), dtype=np.int64)
        for j, dims, start in plan:
            w = np.array([max(Fnew[start + 2 * t], Fnew[start + 2 * t + 1]) for t in range(len(dims))])
            order = np.argsort(-w, kind="stable")                 # best sampled value first
            lv = Lv[:, j].copy()
            for t in order:
                i = dims[t]
                lv[i] += 1                                        # the parent shrinks along i; the two children inherit the levels so far
                newL[:, start + 2 * t] = lv
                newL[:, start + 2 * t + 1] = lv
            Lv[:, j] = lv
        C = np.concatenate([C, Unew], axis=1)
        Lv = np.concatenate([Lv, newL], axis=1)
        F = np.concatenate([F, Fnew])
    jb = int(np.argmax(F))
    return float(F[jb]), to_x(C[:, jb:jb + 1])[:, 0], evals


def direct_l_search(f_batch, lb, ub, maxeval, stopval=math.inf, maxtime=0.0):
    """The same search with the bookkeeping in libbohip (csrc/direct_l.h, bohip_direct_ask / _tell): the caller's f_batch scores each
    iteration's points.  Bit-identical to _batched_direct_l (tests/test_direct_l.py), which stays as its NumPy twin; the NumPy
    bookkeeping was 21 of the 27.7 ms of a default Thompson acquire_max at N = 3000.  Returns (best value, best point, evaluations)."""
    import ctypes as C
    from . import _lib

    lib = _lib.load()
    lb = np.ascontiguousarray(lb, dtype=np.float64); ub = np.ascontiguousarray(ub, dtype=np.float64)
    d = lb.size
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    _lib.check(lib.bohip_direct_create(d, lb.ctypes.data_as(dp), ub.ctypes.data_as(dp), int(max(1, maxeval)), float(stopval),
                                       float(maxtime or 0.0), C.byref(h)))
    try:
        X = np.empty((max(2 * d, 64), d))                         # rows = points (d x cap column-major for the library)
        n = C.c_int64()
        while True:
            _lib.check(lib.bohip_direct_ask(h, None, 0, C.byref(n)))         # size of this iteration's batch
            if n.value == 0:
                break
            if n.value > X.shape[0]:
                X = np.empty((2 * n.value, d))
            _lib.check(lib.bohip_direct_ask(h, X.ctypes.data_as(dp), X.shape[0], C.byref(n)))
            F = np.ascontiguousarray(np.asarray(f_batch(X[:n.value].T), dtype=np.float64).reshape(-1))
            _lib.check(lib.bohip_direct_tell(h, F.ctypes.data_as(dp), n.value))
        bf = C.c_double(); bx = np.empty(d); ev = C.c_int64(); it = C.c_int64()
        _lib.check(lib.bohip_direct_best(h, C.byref(bf), bx.ctypes.data_as(dp), C.byref(ev), C.byref(it)))
        return float(bf.value), bx, int(ev.value)
    finally:
        lib.bohip_direct_destroy(h)


# NLopt.Opt properties the reference forwards with setproperty! (src/acquisition.jl:24-27).  The device ascent
# implements the first group; the second is accepted by NLopt but has no counterpart here (a warning says so);
# anything else raises, as setproperty! on an NLopt.Opt does.
_WARNED_METHODS = set()


def _warn_not_a_local_search(method):
    """:LN_* and the non-DIRECT :GN_* methods have no device counterpart: NLopt would run that algorithm (COBYLA, BOBYQA, Nelder-Mead,
    CRS, ISRES ...) from each start, here `maxeval` Latin-hypercube candidates per restart are scored in one batch and the best one is
    returned.  Said once per process and method, since the result is a candidate-set maximum, not that algorithm's."""
    if method in _WARNED_METHODS:
        return
    _WARNED_METHODS.add(method)
    warnings.warn(f"acquire_max: method :{method} is not implemented as such; maxeval Latin-hypercube candidates per restart are "
                  "scored in one device batch instead (use :LD_LBFGS or :GN_DIRECT_L for a search)", stacklevel=3)


# "joint" is this package's own option (not an NLopt property): ThompsonSamplingSimple over a candidate set takes ONE JOINT draw
# of the posterior (model.sample_joint) instead of independent per-candidate draws (model.thompson).  Default False.
# "pathwise" (with "features" = M, default 2048) is this package's own too: ThompsonSamplingSimple searches ONE posterior sample
# path per restart (model.draw_paths), a function that keeps its value wherever it is evaluated again.  Default False.
# "refine" (default 0) is this package's own as well: Marginalised climbs its n best candidates on the gradient of the average.
# Every other acquisition accepts the key and does NOT use it -- their search is chosen by "method" (:LD_LBFGS climbs already) --
# because BOpt hands ONE options record to the acquisition's search and to its closing MaxMean search (acquire_model_max): a
# record written for Marginalised must pass there.
_OPTS_USED = {"method", "restarts", "maxeval", "maxtime", "ftol_rel", "xtol_abs", "ftol_abs", "xtol_rel", "stopval", "joint",
              "pathwise", "features", "refine"}
_OPTS_NLOPT_ONLY = {"initial_step", "population", "vector_storage", "seed", "local_optimizer", "default_initial_step"}


def _check_options(opts):
    for k in opts:
        if k in _OPTS_USED:
            continue
        if k in _OPTS_NLOPT_ONLY:
            warnings.warn(f"acquisition option {k!r} is an NLopt setting the device ascent does not implement; ignored")
        else:
            raise ValueError(f"unknown acquisition option {k!r} (the reference forwards every key to NLopt.Opt, "
                             "which rejects unknown properties)")


def _acquire_max_pathwise(model, lb, ub, method, restarts, maxeval, maxtime, opts, rng):
    """ThompsonSamplingSimple with "pathwise": True.  Every restart draws ONE posterior sample path (model.draw_paths, S = 1, seed
    from `rng`) and maximises that function:
      :GN_DIRECT*  direct_l_search over x -> path(x): every point of the search sees the same draw (the reference's objective
                   x -> myrand(model, x) returns an unrelated draw per evaluation);
      otherwise    `maxeval` Latin-hypercube points scored on the path, arg-max on the device; with an :LD_* method the best
                   `restarts` of them are then refined by the batched L-BFGS ascent on the path's analytic gradient.
    The first maximum over the restarts wins (strict '>')."""
    if not hasattr(model, "draw_paths"):
        raise NotImplementedError(f"{type(model).__name__} has no draw_paths")
    M = int(opts.get("features", 2048))
    gen = rng or np.random.default_rng()
    sval = float(opts.get("stopval", math.inf))
    direct = "DIRECT" in method.upper()
    ascend = method.upper().startswith("LD")
    if not direct and not ascend:
        _warn_not_a_local_search(method)
    maxf, maxx = -math.inf, lb.copy()
    for _ in range(restarts):
        seed = int(gen.integers(0, 2 ** 63 - 1))
        with model.draw_paths(1, M, seed) as path:
            if direct:
                def path_batch(X):
                    return path.eval(X)[0][0]

                f, x, _ = direct_l_search(path_batch, lb, ub, max(1, maxeval), sval, maxtime)
            else:
                starts = latin_hypercube_sampling(lb, ub, max(maxeval, 1), rng)
                vals, bv, bi = path.eval(starts, want_values=ascend)
                if bi[0] < 0:
                    continue
                f, x = float(bv[0]), starts[:, int(bi[0])].copy()
                if ascend:
                    order = np.argsort(-np.where(np.isnan(vals[0]), -math.inf, vals[0]), kind="stable")[:max(1, restarts)]
                    fa, Xa = _batched_lbfgs_ascent(path.eval_grad, np.asfortranarray(starts[:, order]), lb, ub, max(2, maxeval),
                                                   ftol_rel=float(opts.get("ftol_rel", 1e-10)), xtol_abs=float(opts.get("xtol_abs", 1e-10)),
                                                   ftol_abs=float(opts.get("ftol_abs", 0.0)), xtol_rel=float(opts.get("xtol_rel", 0.0)),
                                                   stopval=sval)
                    j = int(np.argmax(np.where(np.isnan(fa), -math.inf, fa)))
                    if fa[j] > f:
                        f, x = float(fa[j]), Xa[:, j].copy()
        if f > maxf:                                              # :62 strict '>'
            maxf, maxx = f, x
    if not np.isfinite(maxf):
        warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
    return maxf, maxx


def _acquire_max_kg(model, lb, ub, restarts, maxeval, rng):
    """KnowledgeGradient: a candidate-set acquisition without a gradient.  Every restart takes `maxeval` Latin-hypercube candidates,
    evaluates the knowledge gradient of each against the whole set in ONE model.kg call (E = R) and takes the device's arg-max.
    The first maximum over the restarts wins (strict '>')."""
    if not hasattr(model, "kg"):
        raise NotImplementedError(f"{type(model).__name__} has no kg")
    maxf, maxx = -math.inf, lb.copy()
    for _ in range(restarts):
        xs = latin_hypercube_sampling(lb, ub, max(maxeval, 1), rng)
        res = model.kg(xs)
        if res.best_idx >= 0 and res.best_val > maxf:             # :62 strict '>'
            maxf, maxx = float(res.best_val), xs[:, int(res.best_idx)].copy()
    if not np.isfinite(maxf):
        warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
    return maxf, maxx


def _acquire_max_mes(a, model, lb, ub, restarts, maxeval, rng):
    """MaxValueEntropySearch: a candidate-set acquisition without a gradient in x.  Every restart takes `maxeval` Latin-hypercube
    candidates and ONE model.mes call with the device's arg-max; the call's seed is drawn from `rng` after the candidates.  The
    first maximum over the restarts wins (strict '>')."""
    if not hasattr(model, "mes"):
        raise NotImplementedError(f"{type(model).__name__} has no mes")
    gen = rng if rng is not None else np.random.default_rng()
    maxf, maxx = -math.inf, lb.copy()
    for _ in range(restarts):
        xs = latin_hypercube_sampling(lb, ub, max(maxeval, 1), rng)
        res = model.mes(xs, samples=a.samples, mode=a.mode, seed=int(gen.integers(0, 2**63)))
        if res.best_idx >= 0 and res.best_val > maxf:             # :62 strict '>'
            maxf, maxx = float(res.best_val), xs[:, int(res.best_idx)].copy()
    if not np.isfinite(maxf):
        warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
    return maxf, maxx


def _acquire_max_nei(a, model, lb, ub, restarts, maxeval, rng):
    """NoisyExpectedImprovement: no gradient in x.  Every restart scores `maxeval` Latin-hypercube candidates in ONE model.nei call
    and takes the device's arg-max; the fantasies are built once (the seed is the acquisition's).  The first maximum over the
    restarts wins (strict '>')."""
    maxf, maxx = -math.inf, lb.copy()
    for _ in range(restarts):
        xs = latin_hypercube_sampling(lb, ub, max(maxeval, 1), rng)
        val, idx = a.score(model, xs, want_scores=False).best
        if idx >= 0 and val > maxf:                               # :62 strict '>'
            maxf, maxx = float(val), xs[:, int(idx)].copy()
    if not np.isfinite(maxf):
        warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
    return maxf, maxx


def _acquire_max_marginal(a, model, lb, ub, restarts, maxeval, rng, opts=None):
    """Marginalised(a).  Every restart scores `maxeval` Latin-hypercube candidates under all hyper-parameter samples in ONE
    model.score_ensemble call and takes its arg-max record.  The first maximum over the restarts wins (strict '>').
    "refine": n > 0 (default 0: the candidate stage alone, the same calls and draws as without the option): the n highest-scoring
    distinct candidates of all restarts then start ONE batched L-BFGS ascent inside the box, fg = one model.score_ensemble_grad call
    per step, at most `maxeval` evaluations, the tolerances of the other acquisitions; the best ascended point replaces the candidate
    maximum only where it is strictly better, so the result is never worse than with refine = 0."""
    Theta, w = _hyper_samples(model)
    if not hasattr(model, "score_ensemble"):
        raise NotImplementedError(f"{type(model).__name__} has no score_ensemble")
    opts = opts or {}
    refine = int(opts.get("refine", 0) or 0)
    if refine > 0 and not hasattr(model, "score_ensemble_grad"):
        raise NotImplementedError(f"{type(model).__name__} has no score_ensemble_grad")
    maxf, maxx = -math.inf, lb.copy()
    seen_x, seen_f = [], []
    for _ in range(restarts):
        xs = latin_hypercube_sampling(lb, ub, max(maxeval, 1), rng)
        res = model.score_ensemble(a.acq_id, a.params(), xs, Theta, w)
        if res.best_idx >= 0 and res.best_val > maxf:             # :62 strict '>'
            maxf, maxx = float(res.best_val), xs[:, int(res.best_idx)].copy()
        if refine > 0:
            seen_x.append(xs)
            seen_f.append(np.asarray(res.scores, dtype=np.float64))
    if refine > 0 and np.isfinite(maxf):
        X, f = np.concatenate(seen_x, axis=1), np.concatenate(seen_f)
        starts, taken = [], set()
        for j in np.argsort(-np.where(np.isnan(f), -math.inf, f), kind="stable"):
            key = X[:, j].tobytes()
            if np.isfinite(f[j]) and key not in taken:
                taken.add(key)
                starts.append(X[:, j])
                if len(starts) == refine:
                    break
        p = a.params()

        def fg(Z):
            r, g = model.score_ensemble_grad(a.acq_id, p, Z, Theta, w)[:2]
            return np.asarray(r.scores, dtype=np.float64), np.asarray(g, dtype=np.float64)

        fa, Xa = _batched_lbfgs_ascent(fg, np.asfortranarray(np.stack(starts, axis=1)), lb, ub, max(2, maxeval),
                                       ftol_rel=float(opts.get("ftol_rel", 1e-10)), xtol_abs=float(opts.get("xtol_abs", 1e-10)),
                                       ftol_abs=float(opts.get("ftol_abs", 0.0)), xtol_rel=float(opts.get("xtol_rel", 0.0)),
                                       stopval=float(opts.get("stopval", math.inf)))
        j = int(np.argmax(np.where(np.isnan(fa), -math.inf, fa)))
        if fa[j] > maxf:                                          # strict '>': never worse than the candidate maximum
            maxf, maxx = float(fa[j]), Xa[:, j].copy()
    if not np.isfinite(maxf):
        warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
    return maxf, maxx


def _acquire_max_constrained(a, model, lb, ub, restarts, maxeval, rng, opts=None):
    """Constrained(a) over a ConstrainedGPE.  Every restart scores `maxeval` Latin-hypercube candidates in ONE model.score call and
    takes its arg-max record; the first maximum over the restarts wins (strict '>').  "refine": n > 0 (default 0: the candidate stage
    alone): the n highest-scoring distinct candidates then start ONE batched L-BFGS ascent inside the box, fg = one gradient-route
    model.score call per step; the best ascended point replaces the candidate maximum only where it is strictly better."""
    acq, p = a.acq_id, a.params()
    return _acquire_max_candidates(lambda xs, want_grad=False: model.score(acq, p, xs, want_grad=want_grad), lb, ub, restarts,
                                   maxeval, rng, opts)


def _acquire_max_mo(model, lb, ub, restarts, maxeval, rng, opts=None):
    """ExpectedHypervolumeImprovement over a MultiObjectiveGPE: _acquire_max_constrained's two stages on model.score(xs), ONE
    bohip_gp_score_mo call per restart and, with "refine": n > 0, one gradient-route call per step of the ascent."""
    return _acquire_max_candidates(lambda xs, want_grad=False: model.score(xs, want_grad=want_grad), lb, ub, restarts, maxeval, rng,
                                   opts)


def _acquire_max_candidates(score, lb, ub, restarts, maxeval, rng, opts=None):
    """The Latin-hypercube candidate route of a score over several models: score(xs, want_grad) -> a result with scores, grad [d, R],
    best_val, best_idx (see _acquire_max_constrained)."""
    opts = opts or {}
    refine = int(opts.get("refine", 0) or 0)
    maxf, maxx = -math.inf, lb.copy()
    seen_x, seen_f = [], []
    for _ in range(restarts):
        xs = latin_hypercube_sampling(lb, ub, max(maxeval, 1), rng)
        res = score(xs)
        if res.best_idx >= 0 and res.best_val > maxf:             # :62 strict '>'
            maxf, maxx = float(res.best_val), xs[:, int(res.best_idx)].copy()
        if refine > 0:
            seen_x.append(xs)
            seen_f.append(np.asarray(res.scores, dtype=np.float64))
    if refine > 0 and np.isfinite(maxf):
        X, f = np.concatenate(seen_x, axis=1), np.concatenate(seen_f)
        starts, taken = [], set()
        for j in np.argsort(-np.where(np.isnan(f), -math.inf, f), kind="stable"):
            key = X[:, j].tobytes()
            if np.isfinite(f[j]) and key not in taken:
                taken.add(key)
                starts.append(X[:, j])
                if len(starts) == refine:
                    break

        def fg(Z):
            r = score(Z, want_grad=True)
            return np.asarray(r.scores, dtype=np.float64), np.asarray(r.grad, dtype=np.float64)

        fa, Xa = _batched_lbfgs_ascent(fg, np.asfortranarray(np.stack(starts, axis=1)), lb, ub, max(2, maxeval),
                                       ftol_rel=float(opts.get("ftol_rel", 1e-10)), xtol_abs=float(opts.get("xtol_abs", 1e-10)),
                                       ftol_abs=float(opts.get("ftol_abs", 0.0)), xtol_rel=float(opts.get("xtol_rel", 0.0)),
                                       stopval=float(opts.get("stopval", math.inf)))
        j = int(np.argmax(np.where(np.isnan(fa), -math.inf, fa)))
        if fa[j] > maxf:                                          # strict '>': never worse than the candidate maximum
            maxf, maxx = float(fa[j]), Xa[:, j].copy()
    if not np.isfinite(maxf):
        warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
    return maxf, maxx


def acquire_max(a, model, lowerbounds, upperbounds, options, rng=None, setparams=True):
    """src/acquisition.jl:48-68: R Latin-hypercube starts (utils.jl:96-120), local search from each, keep the
    best under strict '>' (first maximum wins).  Returns (maxf, maxx).
    setparams=True is the 5-argument method (:48-51: nlopt_setup calls setparams!, :30); the BO loop has already
    called setparams! (src/BayesianOptimization.jl:184) and uses the 4-argument method on its prepared optimiser
    (:185), i.e. setparams=False -- MutualInformation's update is not idempotent."""
    lb = np.asarray(lowerbounds, dtype=np.float64)
    ub = np.asarray(upperbounds, dtype=np.float64)
    opts = options if isinstance(options, dict) else dict(vars(options))
    _check_options(opts)
    if setparams:
        setparams_(a, model)                                      # nlopt_setup :30
    method = str(opts.get("method", "LD_LBFGS")).lstrip(":")
    restarts = int(opts.get("restarts", 10))
    maxeval = int(opts.get("maxeval", 2000))
    maxtime = float(opts.get("maxtime", 0.0) or 0.0)
    maxf, maxx = -math.inf, lb.copy()                             # :55-56
    if model.nobs == 0 or restarts <= 0:
        return maxf, maxx
    if isinstance(a, KnowledgeGradient):                          # (`method` has nothing to select between: accepted, not used)
        return _acquire_max_kg(model, lb, ub, restarts, maxeval, rng)
    if isinstance(a, MaxValueEntropySearch):                      # (`method` is accepted, not used)
        return _acquire_max_mes(a, model, lb, ub, restarts, maxeval, rng)
    if isinstance(a, NoisyExpectedImprovement):                   # (`method` is accepted, not used)
        return _acquire_max_nei(a, model, lb, ub, restarts, maxeval, rng)
    if isinstance(a, Constrained):                                # (`method` is accepted, not used; "refine" adds the ascent)
        if not hasattr(model, "feasible_incumbent"):
            raise ValueError(f"Constrained needs a ConstrainedGPE, not {type(model).__name__}")
        return _acquire_max_constrained(a, model, lb, ub, restarts, maxeval, rng, opts)
    if isinstance(a, ExpectedHypervolumeImprovement):             # (`method` is accepted, not used; "refine" adds the ascent)
        _need_mo(model)
        return _acquire_max_mo(model, lb, ub, restarts, maxeval, rng, opts)
    if isinstance(a, Marginalised):                               # (`method` is accepted, not used; "refine" adds the ascent)
        return _acquire_max_marginal(a, model, lb, ub, restarts, maxeval, rng, opts)
    derivative = len(method) > 1 and method[1] == "D" and not isinstance(a, ThompsonSamplingSimple)   # :31
    if bool(opts.get("pathwise", False)):
        if not isinstance(a, ThompsonSamplingSimple):
            raise ValueError("option 'pathwise' applies to ThompsonSamplingSimple only")
        return _acquire_max_pathwise(model, lb, ub, method, restarts, maxeval, maxtime, opts, rng)
    if "DIRECT" in method.upper() and not derivative:
        # :GN_DIRECT_L (the reference's default for ThompsonSamplingSimple, src/acquisition.jl:7-9) and its siblings: dividing
        # rectangles with every iteration's new points in one device call.  DIRECT ignores the start point, so `restarts` runs are
        # `restarts` repetitions (identical for a deterministic acquisition, fresh draws for a sampled one), as with NLopt.
        sval = float(opts.get("stopval", math.inf))
        thompson = isinstance(a, ThompsonSamplingSimple)
        gen = (rng or np.random.default_rng()) if thompson else None
        fused = hasattr(model, "direct_max")                      # device model: the whole search is ONE library call
        if thompson:
            def f_batch(X):                                       # x -> myrand(model, x), one draw per point (src/acquisitionfunctions.jl:108)
                mu, var = model.predict_f(X)
                return np.asarray(mu) + np.sqrt(np.maximum(np.asarray(var), 0.0)) * gen.standard_normal(np.size(mu))
        else:
            def f_batch(X):
                return model.score(a.acq_id, a.params(), X)[0]
        for _ in range(restarts):
            if fused:                                             # (the draws come from the library's counter-based generator,
                seed = int(gen.integers(0, 2 ** 63 - 1)) if thompson else 0   #  keyed by a seed taken from `rng`)
                f, x, _, _ = model.direct_max("ThompsonDraw" if thompson else a.acq_id, None if thompson else a.params(), lb, ub,
                                              max(1, maxeval), sval, maxtime, seed)
            else:
                f, x, _ = direct_l_search(f_batch, lb, ub, max(1, maxeval), sval, maxtime)
            if f > maxf:                                          # :62 strict '>'
                maxf, maxx = f, x
            if not thompson:
                break                                             # deterministic objective: every repetition is the same run
        if not np.isfinite(maxf):
            warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
        return maxf, maxx
    if isinstance(a, ThompsonSamplingSimple):
        _warn_not_a_local_search(method)
        # `maxeval` candidates per restart, arg-max on the device.  Default: model.thompson, every candidate drawn INDEPENDENTLY
        # from its own marginal (mu_j + sigma_j z_j).  "joint": True: model.sample_joint, ONE JOINT draw of the posterior over the
        # candidates (mu + chol(Sigma) z, the reference's myrand(model, X::Matrix)), whose arg-max is a draw of the maximiser.
        n = max(maxeval, 1)
        joint = bool(opts.get("joint", False))
        for _ in range(restarts):
            starts = latin_hypercube_sampling(lb, ub, n, rng)
            seed = int((rng or np.random.default_rng()).integers(0, 2 ** 63 - 1))
            if joint:
                js = model.sample_joint(starts, 1, seed, want_samples=False)
                bv, bi = js.best_val, js.best_idx
            else:
                bv, bi = model.thompson(starts, 1, seed=seed)
            if bi[0] >= 0 and bv[0] > maxf:
                maxf, maxx = float(bv[0]), starts[:, int(bi[0])].copy()
        return maxf, maxx
    acq, p = a.acq_id, a.params()
    if derivative:
        starts = latin_hypercube_sampling(lb, ub, restarts, rng)
        # maxeval: NLopt counts objective evaluations per start; the batched ascent spends one evaluation of EVERY
        # start per device pass, so the same number bounds the passes.  No other cap.
        iters = max(2, maxeval)

        ftol, xtol = float(opts.get("ftol_rel", 1e-10)), float(opts.get("xtol_abs", 1e-10))
        # ftol_abs / xtol_rel / stopval with NLopt's defaults (off); the reference's own test passes ftol_abs = eps() (test/acquisition.jl:6,9)
        fabs_, xrel, sval = float(opts.get("ftol_abs", 0.0)), float(opts.get("xtol_rel", 0.0)), float(opts.get("stopval", math.inf))
        if hasattr(model, "ascend"):                              # device model: the whole search runs in libbohip
            if hasattr(model, "set_maxtime"):
                model.set_maxtime(maxtime)                        # NLopt maxtime: per optimize call = per acquire_max here
            if hasattr(model, "set_ascent_stop"):
                model.set_ascent_stop(fabs_, xrel, sval)
            f, X, bf, bi, bx, _ = model.ascend(acq, p, lb, ub, starts, iters, ftol, xtol)
            if bi >= 0:
                return float(bf), np.array(bx)
            warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
            return maxf, maxx

        def fg(X):                                                # host restatement of the same search (test models)
            return model.score_grad(acq, p, X)

        f, X = _batched_lbfgs_ascent(fg, starts, lb, ub, iters, ftol_rel=ftol, xtol_abs=xtol, ftol_abs=fabs_, xtol_rel=xrel,
                                     stopval=sval)
    else:
        _warn_not_a_local_search(method)
        n = max(restarts, min(maxeval * restarts, 1 << 20))
        X = latin_hypercube_sampling(lb, ub, n, rng)
        f, _, _ = model.score(acq, p, X)
    for j in range(X.shape[1]):                                   # :58-66, strict '>' => first maximum wins
        if f[j] > maxf:
            maxf, maxx = float(f[j]), X[:, j].copy()
    if not np.isfinite(maxf):
        warnings.warn("acquisition returned no finite value; keeping the lower bounds as maximiser")
    return maxf, maxx


_PENDING_REFUSED = (KnowledgeGradient, MaxValueEntropySearch, Marginalised, Constrained, ExpectedHypervolumeImprovement,
                    ThompsonSamplingSimple, NoisyExpectedImprovement)


def acquire_max_pending(a, model, lowerbounds, upperbounds, options, rng=None, setparams=True):
    """acquire_max for a model with pending evaluations (model.set_pending; an extension): the acquisition is
    averaged over fantasised outcomes at the pending points (Snoek, Larochelle & Adams 2012, section 3.2), so the proposal keeps
    away from what is already out for evaluation.  With an empty pending set it returns acquire_max(...) itself.  Otherwise every
    restart scores `maxeval` Latin-hypercube candidates in ONE model.score_pending call and takes its arg-max record; the call's seed
    is drawn from `rng` after the candidates; the first maximum over the restarts wins (strict '>').  There is no gradient in x, so
    "method" and "refine" are accepted and not used.  Options: those of acquire_max plus "fantasies" (default 16; 0: the Kriging
    believer) and "raise_tau" (default True: the incumbent of EI / PI / LogEI follows each fantasy)."""
    opts = dict(options if isinstance(options, dict) else vars(options))
    fantasies = int(opts.pop("fantasies", 16))
    raise_tau = bool(opts.pop("raise_tau", True))
    pending = getattr(model, "pending", None)
    if pending is None or np.shape(pending)[1] == 0:
        return acquire_max(a, model, lowerbounds, upperbounds, opts, rng, setparams)
    if isinstance(a, _PENDING_REFUSED):
        raise ValueError(f"{type(a).__name__} with pending evaluations is not built")
    if not hasattr(model, "score_pending"):
        raise ValueError(f"{type(model).__name__} with pending evaluations is not built")
    lb = np.asarray(lowerbounds, dtype=np.float64)
    ub = np.asarray(upperbounds, dtype=np.float64)
    _check_options(opts)
    if setparams:
        setparams_(a, model)
    restarts = int(opts.get("restarts", 10))
    maxeval = int(opts.get("maxeval", 2000))
    if model.nobs == 0 or restarts <= 0:
        return -math.inf, lb.copy()
    gen = rng if rng is not None else np.random.default_rng()
    acq, p = a.acq_id, a.params()

    def score(xs):
        return model.score_pending(acq, p, xs, fantasies=fantasies, seed=int(gen.integers(0, 2 ** 63 - 1)), raise_tau=raise_tau)

    return _acquire_max_candidates(score, lb, ub, restarts, maxeval, rng, {**opts, "refine": 0})


_BATCH_OPTS = {"candidates", "xs", "fantasy", "raise_tau", "method", "draws", "pathwise", "features"}
_BATCH_FANTASIES = ("believer", "liar_max", "liar_min", "liar_mean")
_BATCH_METHODS = ("fantasy", "qei")


def acquire_batch(a, model, lowerbounds, upperbounds, q, options=None, rng=None, setparams=True):
    """q points to evaluate in parallel -- an extension: the reference's iteration is one acquire_max and `repetitions`
    evaluations of ONE point (src/BayesianOptimization.jl:185-196).  options: "candidates" Latin-hypercube points (default 4096)
    or an explicit d x R "xs"; "method":
      "fantasy" (default)  greedy arg-max over the candidates under the posterior conditioned on the fantasised observations of
          the earlier picks (model.select_batch; the model itself is not changed).  "fantasy" in {"believer" (y_f = mu),
          "liar_max", "liar_min", "liar_mean" (a constant taken from model.y)}; "raise_tau" (EI / PI: the incumbent follows the
          fantasies).  Every pick is scored by a one-point acquisition.
      "qei"  the batch is scored as a batch: greedy Monte-Carlo q-EI, qEI(B) = E[max(max_{j in B} f_j - tau, 0)], over "draws"
          (default 256) JOINT posterior draws that stay on the device (model.qei_batch; seed from `rng`).  The acquisition must
          be ExpectedImprovement, and only its tau (after setparams_) is used: with q = 1 the value estimates the TEXTBOOK EI,
          Delta Phi(z) + sigma phi(z), whereas the reference's ExpectedImprovement functor computes Delta Phi(z) + phi(z).
          "pathwise": True takes the draws from posterior sample paths instead (model.draw_paths with "features" = M random
          features, default 2048, evaluated over the candidates, then model.qei_select): no R x R factorisation, so "candidates"
          may exceed one chunk.  The values returned are the picks' marginal gains; their sum is the batch's q-EI estimate.
    Returns (values[q'], X d x q') with q' <= q: picks that could not win (no finite score / no gain left) are dropped."""
    lb = np.asarray(lowerbounds, dtype=np.float64)
    ub = np.asarray(upperbounds, dtype=np.float64)
    opts = dict(options or {})
    for k in opts:
        if k not in _BATCH_OPTS:
            raise ValueError(f"unknown batch option {k!r} (known: {sorted(_BATCH_OPTS)})")
    q = int(q)
    if q < 1:
        raise ValueError(f"batch size q = {q} < 1")
    if lb.size != ub.size:
        raise ValueError("length of lowerbounds does not match length of upperbounds")
    method = opts.get("method", "fantasy")
    if method not in _BATCH_METHODS:
        raise ValueError(f"batch method must be one of {_BATCH_METHODS}, got {method!r}")
    qei = method == "qei"
    if qei:
        if "fantasy" in opts or "raise_tau" in opts:
            raise ValueError("batch options 'fantasy' and 'raise_tau' belong to method 'fantasy': q-EI conditions on no fantasy, "
                             "its draws are joint")
        if not isinstance(a, ExpectedImprovement):
            raise ValueError(f"batch method 'qei' is the batch form of expected improvement and takes its incumbent tau from an "
                             f"ExpectedImprovement acquisition, got {type(a).__name__}")
        pathwise = bool(opts.get("pathwise", False))
        if not pathwise and "features" in opts:
            raise ValueError("batch option 'features' needs 'pathwise': True")
        draws = int(opts.get("draws", 256))
        if draws < 1:
            raise ValueError(f"options['draws'] = {draws} < 1")
        need = ("draw_paths", "qei_select") if pathwise else ("qei_batch",)
    else:
        for k in ("draws", "pathwise", "features"):
            if k in opts:
                raise ValueError(f"batch option {k!r} needs 'method': 'qei'")
        need = ("select_batch",)
    fantasy = opts.get("fantasy", "believer")
    if fantasy not in _BATCH_FANTASIES:
        raise ValueError(f"fantasy must be one of {_BATCH_FANTASIES}, got {fantasy!r}")
    if isinstance(a, ThompsonSamplingSimple):
        raise ValueError("acquire_batch needs a deterministic acquisition (ThompsonSamplingSimple draws its own batch: model.thompson)")
    for name in need:
        if not hasattr(model, name):
            raise NotImplementedError(f"{type(model).__name__} has no {name}")
    if "xs" in opts and opts["xs"] is not None:
        xs = np.asarray(opts["xs"], dtype=np.float64)
        if xs.ndim != 2 or xs.shape[0] != lb.size:
            raise ValueError(f"options['xs'] must be {lb.size} x R (one point per column), got shape {xs.shape}")
    else:
        ncand = int(opts.get("candidates", 4096))
        if ncand < 1:
            raise ValueError(f"options['candidates'] = {ncand} < 1")
        xs = latin_hypercube_sampling(lb, ub, ncand, rng)
    if q > xs.shape[1]:
        raise ValueError(f"batch size q = {q} exceeds the {xs.shape[1]} candidates")
    if model.nobs == 0:
        raise RuntimeError("acquire_batch on an empty model")
    if setparams:
        setparams_(a, model)
    if qei:
        seed = int((rng or np.random.default_rng()).integers(0, 2 ** 63 - 1))
        if pathwise:
            with model.draw_paths(draws, int(opts.get("features", 2048)), seed) as paths:
                F, _, _ = paths.eval(xs)
            idx, val = model.qei_select(F, a.tau, q)
        else:
            res = model.qei_batch(xs, q, draws, seed, tau=a.tau)
            idx, val = res.idx, res.gain
        keep = idx >= 0
        if not keep.all():
            warnings.warn(f"acquire_batch: only {int(keep.sum())} of {q} picks had a gain above zero")
        return val[keep], np.asfortranarray(xs[:, idx[keep]])
    y = np.asarray(model.y)
    fv = {"believer": "believer", "liar_max": float(y.max()), "liar_min": float(y.min()), "liar_mean": float(y.mean())}[fantasy]
    idx, val, _, _ = model.select_batch(a.acq_id, a.params(), xs, q, fantasy=fv, raise_tau=bool(opts.get("raise_tau", False)))
    keep = idx >= 0
    if not keep.all():
        warnings.warn(f"acquire_batch: only {int(keep.sum())} of {q} picks had a finite score")
    return val[keep], np.asfortranarray(xs[:, idx[keep]])


def _distinct_picks(samples):
    """Greedy distinct arg-max over the rows of an S x R sample matrix: draw s takes its best candidate not already taken by draws
    0..s-1 (strict '>' from -Inf, ties -> smallest index, NaN never wins).  -1 where no candidate is left that could win."""
    F = np.asarray(samples, dtype=np.float64)
    taken = np.zeros(F.shape[1], dtype=bool)
    out = np.full(F.shape[0], -1, dtype=np.int64)
    for s in range(F.shape[0]):
        f = np.where(taken | np.isnan(F[s]), -math.inf, F[s])
        j = int(np.argmax(f)) if f.size else -1               # (argmax: the first maximum)
        if j >= 0 and f[j] > -math.inf:
            out[s] = j
            taken[j] = True
    return out


_THOMPSON_BATCH_OPTS = {"candidates", "xs", "pathwise", "features", "refine", "maxeval"}


def acquire_thompson_batch(model, lowerbounds, upperbounds, q, options=None, rng=None):
    """q points to evaluate in parallel by Thompson sampling -- an extension, as acquire_batch is.  ONE model.sample_joint call
    with S = q joint posterior draws over a candidate set ("candidates" Latin-hypercube points, default 4096, or an explicit
    d x R "xs"); draw s takes its best candidate not already taken by draws 0..s-1 (_distinct_picks).  The draws' seed comes from
    `rng`.  Returns (values[q'], X d x q'), q' <= q (a draw with no finite value left is dropped).
    "pathwise": True (default False): the q draws are posterior sample PATHS (model.draw_paths, S = q, "features" = M random
    features, default 2048) evaluated over the candidates in one call -- no R x R factorisation, so "candidates" may exceed one
    chunk -- and, with "refine" (default True), every pick is then ascended on ITS OWN path (eval_grad with path_of; at most
    "maxeval" passes, default 200) inside the box; a refined point replaces its pick only where its path value is higher and the
    point is not already in the batch (two paths may climb to the same corner of the box)."""
    lb = np.asarray(lowerbounds, dtype=np.float64)
    ub = np.asarray(upperbounds, dtype=np.float64)
    opts = dict(options or {})
    for k in opts:
        if k not in _THOMPSON_BATCH_OPTS:
            raise ValueError(f"unknown Thompson batch option {k!r} (known: {sorted(_THOMPSON_BATCH_OPTS)})")
    q = int(q)
    if q < 1:
        raise ValueError(f"batch size q = {q} < 1")
    if lb.size != ub.size:
        raise ValueError("length of lowerbounds does not match length of upperbounds")
    pathwise = bool(opts.get("pathwise", False))
    if not pathwise and any(k in opts for k in ("features", "refine", "maxeval")):
        raise ValueError("Thompson batch options 'features', 'refine' and 'maxeval' need 'pathwise': True")
    if not hasattr(model, "draw_paths" if pathwise else "sample_joint"):
        raise NotImplementedError(f"{type(model).__name__} has no {'draw_paths' if pathwise else 'sample_joint'}")
    if "xs" in opts and opts["xs"] is not None:
        xs = np.asarray(opts["xs"], dtype=np.float64)
        if xs.ndim != 2 or xs.shape[0] != lb.size:
            raise ValueError(f"options['xs'] must be {lb.size} x R (one point per column), got shape {xs.shape}")
    else:
        ncand = int(opts.get("candidates", 4096))
        if ncand < 1:
            raise ValueError(f"options['candidates'] = {ncand} < 1")
        xs = latin_hypercube_sampling(lb, ub, ncand, rng)
    if q > xs.shape[1]:
        raise ValueError(f"batch size q = {q} exceeds the {xs.shape[1]} candidates")
    if model.nobs == 0:
        raise RuntimeError("acquire_thompson_batch on an empty model")
    seed = int((rng or np.random.default_rng()).integers(0, 2 ** 63 - 1))
    if pathwise:
        with model.draw_paths(q, int(opts.get("features", 2048)), seed) as paths:
            F, _, _ = paths.eval(xs)
            idx = _distinct_picks(F)
            keep = idx >= 0
            if not keep.all():
                warnings.warn(f"acquire_thompson_batch: only {int(keep.sum())} of {q} draws had a finite value left")
            rows = np.flatnonzero(keep)
            vals, X = F[rows, idx[rows]].copy(), np.asfortranarray(xs[:, idx[rows]])
            if bool(opts.get("refine", True)) and rows.size:
                fa, Xa = _batched_lbfgs_ascent(lambda Z: paths.eval_grad(Z, rows), X, lb, ub, max(2, int(opts.get("maxeval", 200))))
                for s in np.flatnonzero(fa > vals):               # (two paths may climb to the same point, e.g. a corner of the box:
                    others = np.delete(X, s, axis=1)              #  the batch stays distinct, the later one keeps its pick)
                    if not np.any(np.all(others == Xa[:, [s]], axis=0)):
                        X[:, s], vals[s] = Xa[:, s], fa[s]
        return vals, X
    F = model.sample_joint(xs, q, seed).samples
    idx = _distinct_picks(F)
    keep = idx >= 0
    if not keep.all():
        warnings.warn(f"acquire_thompson_batch: only {int(keep.sum())} of {q} draws had a finite value left")
    rows = np.flatnonzero(keep)
    return F[rows, idx[rows]], np.asfortranarray(xs[:, idx[rows]])


def acquire_model_max(o, options=None):                           # :45-47
    return acquire_max(MaxMean(), o.model, o.lowerbounds, o.upperbounds, options or o.acquisitionoptions, o.rng)
