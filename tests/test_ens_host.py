"""The marginalised acquisition without a GPU: the ABI of include/bohip_ens.h in every table that binds it, the slice sampler on an
analytic target, score_ensemble's host route against the NumPy twin (tests/ens_reference.py) on a duck-typed model, and the plumbing
of Marginalised / MarginalGPOptimizer through acquisitionfunction / acquire_max."""
import ctypes as C
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ens_reference as er   # noqa: E402
from conftest import ROOT, synth   # noqa: E402
from matern_reference import KERNELS, MaternGP, first_argmax   # noqa: E402
from test_kg_host import LB, UB, StubModel   # noqa: E402

WANT = {"bohip_gp_score_ens"}


def test_ens_header_exports_ctypes_and_julia_agree():
    """include/bohip_ens.h <-> exports <-> _lib.ENS_SIGNATURES <-> julia/BOHipEns.jl: the same symbol, the same types argument by
    argument, in none of the other headers' tables (the pattern of tests/test_kg_host.py)."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_ens.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "double": "double", "double*": "ptr(double)", "int64_t*": "ptr(int64)",
               "bohip_best*": "ptr(best)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.ENS_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES, _lib.ACQ_SIGNATURES, _lib.KG_SIGNATURES):
        assert not WANT & set(other)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    main_syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & main_syms and len(main_syms) == 62 == len(_lib.SIGNATURES)
    assert "EXTENSION" in raw and "Snoek" in raw
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_double: "double", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int64): "ptr(int64)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)",
                "Ptr{Int64}": "ptr(int64)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipEns.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.ENS_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
        assert len(args) == 14
    assert 'include("BOHipEns.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)
    mk = open(os.path.join(ROOT, "bayesianoptimization.jl_amd", "csrc", "Makefile")).read()
    assert "kernels_ens.hip" in mk and "bohip_ens.h" in mk


def test_null_handle_is_reported_and_nothing_runs_without_a_device():
    import bohip
    from bohip import _lib

    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    th, xs, p = np.zeros(4), np.zeros(2), np.zeros(2)
    best = _lib.Best()
    rc = lib.bohip_gp_score_ens(None, _lib.ACQ["EI"], p.ctypes.data_as(dp), 1, th.ctypes.data_as(dp), None, xs.ctypes.data_as(dp), 1,
                                None, None, None, None, None, C.byref(best))
    assert rc == _lib.E_ARG and b"null" in lib.bohip_last_error()
    if lib.bohip_device_count() == 0:                             # no device: there is no model to call score_ensemble on, and no
        with pytest.raises(bohip.BohipError) as e:                # quiet host substitute for one
            bohip.ElasticGPE(2)
        assert e.value.code == _lib.E_NODEVICE and "no CPU fallback" in str(e.value)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
MEAN = np.array([0.3, -0.2])
COV = np.array([[1.0, 0.6], [0.6, 0.5]])
PREC = np.linalg.inv(COV)
BOX_LO, BOX_HI = np.array([-8.0, -8.0]), np.array([8.0, 8.0])       # >= 7.7 standard deviations from the mean on every side


def gauss_logp(X):
    D = X - MEAN[:, None]
    return -0.5 * np.einsum("ih,ij,jh->h", D, PREC, D)


def run_sampler(seed=11, H=512, sweeps=40):
    from bohip.bopt import _slice_sample_batch

    rng = np.random.default_rng(seed)
    X0 = rng.uniform(-3.0, 3.0, (2, H))
    calls = []

    def logp(X):
        calls.append(X.shape)
        return gauss_logp(X)

    X, f, trace = _slice_sample_batch(logp, X0, BOX_LO, BOX_HI, sweeps, rng)
    return X, f, trace, calls


def test_slice_sampler_reproduces_a_correlated_gaussian():
    H = 512
    X, f, trace, calls = run_sampler(H=H)
    assert trace.shape == (40, 2, H) and np.array_equal(trace[-1], X)
    assert all(c == (2, H) for c in calls)                        # every evaluation is one call for all H chains
    np.testing.assert_array_equal(f, gauss_logp(X))
    assert np.all(trace >= BOX_LO[None, :, None]) and np.all(trace <= BOX_HI[None, :, None])
    # 512 independent draws of N(MEAN, COV): se(mean_i) = sqrt(COV_ii / n), se(cov_ij) = sqrt((COV_ii COV_jj + COV_ij^2) / n)
    n = float(H)
    se_mean = np.sqrt(np.diag(COV) / n)
    se_cov = np.sqrt((np.outer(np.diag(COV), np.diag(COV)) + COV ** 2) / n)
    got_mean, got_cov = X.mean(axis=1), np.cov(X)
    print("mean z", (got_mean - MEAN) / se_mean, "cov z", (got_cov - COV) / se_cov)
    assert np.all(np.abs(got_mean - MEAN) <= 5.0 * se_mean)
    assert np.all(np.abs(got_cov - COV) <= 5.0 * se_cov)
    X2, f2, trace2, _ = run_sampler(H=H)                          # the same seed: the same bytes
    np.testing.assert_array_equal(X, X2)
    np.testing.assert_array_equal(f, f2)
    np.testing.assert_array_equal(trace, trace2)


def test_slice_sampler_never_leaves_the_support():
    from bohip.bopt import _slice_sample_batch

    lo, hi = np.array([-1.0, 0.0]), np.array([1.0, 2.0])

    def logp(X):
        inside = np.all((X >= lo[:, None]) & (X <= hi[:, None]), axis=0)
        return np.where(inside, gauss_logp(X), -np.inf)

    rng = np.random.default_rng(5)
    X0 = lo[:, None] + rng.random((2, 64)) * (hi - lo)[:, None]
    X, f, trace = _slice_sample_batch(logp, X0, BOX_LO, BOX_HI, 25, rng)
    assert np.all(trace >= lo[None, :, None]) and np.all(trace <= hi[None, :, None]) and np.all(np.isfinite(f))
    assert np.ptp(trace[-1], axis=1).min() > 0.5                  # ... and it moves
    with pytest.raises(ValueError, match="finite"):
        _slice_sample_batch(logp, X0, np.array([-np.inf, 0.0]), hi, 1, rng)


# ---- score_ensemble's host route --------------------------------------------------------------------------------------------------
class DuckModel:
    """What score_ensemble's host route needs of a model, on MaternGP: no handle, so the device route cannot be taken.  A setting
    whose logNoise is below -30 raises NotPositiveDefinite, as a failed refit would."""

    def __init__(self, kern, X, y, t):
        self.kern, self.X, self.y, self.dim = kern, X, y, X.shape[1]
        self.kernel = SimpleNamespace(ll=np.array(t[2:-1], dtype=float), lsigma=float(t[-1]), iso=KERNELS[kern][1])
        self.logNoise, self.mean = float(t[0]), SimpleNamespace(beta=float(t[1]))
        self.sets = 0

    @property
    def nobs(self):
        return self.y.size

    def set_params_(self, ll=None, lsigma=None, logNoise=None, beta=None):
        self.sets += 1
        self.kernel.ll, self.kernel.lsigma = np.array(ll, dtype=float), float(lsigma)
        self.logNoise, self.mean = float(logNoise), SimpleNamespace(beta=float(beta))

    def _gp(self):
        from bohip import NotPositiveDefinite

        if self.logNoise < -30:
            raise NotPositiveDefinite(-2, "pivot 1")
        return MaternGP(self.kern, self.X, self.y, self.kernel.ll, self.kernel.lsigma, self.logNoise, self.mean.beta)

    def score(self, acq, params, xs, want_scores=True):
        sc = self._gp().score(acq, list(params), np.asarray(xs).T)
        return (sc,) + first_argmax(sc)

    def predict_f(self, xs):
        return self._gp().predict(np.asarray(xs).T)


def host_case():
    kern, N, d, R = "Mat52Ard", 20, 3, 9
    X, y, Xs = synth(N, d, R, seed=3)
    c = np.concatenate([[-1.5, 0.2], np.full(d, -0.6), [0.3]])
    Theta = c + np.random.default_rng(2).uniform(-1, 1, (4, c.size))
    return kern, X, y, Xs, c, Theta


@pytest.mark.parametrize("acq,params", [("EI", None), ("UCB", [2.5]), ("MI", [1.0, 0.3]), ("MaxMean", [])])
def test_host_route_equals_the_twin_and_restores_the_model(acq, params):
    from bohip.model import score_ensemble

    kern, X, y, Xs, c, Theta = host_case()
    params = [float(np.median(y))] if params is None else params
    m = DuckModel(kern, X, y, c)
    mean0 = m.mean
    w = np.array([0.5, 1.0, 0.0, 2.5])
    for weights in (None, w):
        res = score_ensemble(m, acq, params, Xs.T, Theta, weights=weights, want_each=True, want_moments=True)
        ref = er.score_ens(kern, X, y, Theta, acq, params, Xs, weights)
        assert res.route == "host" and np.all(res.pivot == 0)
        np.testing.assert_array_equal(res.scores, ref["scores"])
        np.testing.assert_array_equal(res.each, ref["each"])
        np.testing.assert_array_equal(res.mu, ref["mu"])
        np.testing.assert_array_equal(res.var, ref["var"])
        assert (res.best_val, res.best_idx) == (ref["best_val"], ref["best_idx"])
        assert np.array_equal(m.kernel.ll, c[2:-1]) and (m.kernel.lsigma, m.logNoise) == (c[-1], c[0]) and m.mean is mean0
    plain = score_ensemble(m, acq, params, Xs.T, Theta)
    assert plain.each is None and plain.mu is None and plain.var is None


def test_host_route_reports_a_failed_row_and_still_restores():
    from bohip import NotPositiveDefinite
    from bohip.model import score_ensemble

    kern, X, y, Xs, c, Theta = host_case()
    p = [float(np.median(y))]
    m = DuckModel(kern, X, y, c)
    bad = Theta.copy()
    bad[1, 0] = -40.0                                             # raises in the model
    bad[3, 2] = np.nan                                            # never reaches it
    res = score_ensemble(m, "EI", p, Xs.T, bad, want_each=True, want_moments=True)
    assert res.pivot.tolist() == [0, 1, 0, 1]
    assert np.all(np.isnan(res.each[[1, 3]])) and np.all(np.isnan(res.mu[[1, 3]])) and np.all(np.isnan(res.var[[1, 3]]))
    ref = er.score_ens(kern, X, y, Theta[[0, 2]], "EI", p, Xs)
    np.testing.assert_array_equal(res.scores, ref["scores"])
    assert np.array_equal(m.kernel.ll, c[2:-1]) and (m.kernel.lsigma, m.logNoise, m.mean.beta) == (c[-1], c[0], c[1])

    class Broken(DuckModel):
        def score(self, *a, **k):
            raise RuntimeError("device lost")

    b = Broken(kern, X, y, c)
    with pytest.raises(RuntimeError, match="device lost"):
        score_ensemble(b, "EI", p, Xs.T, Theta)
    assert np.array_equal(b.kernel.ll, c[2:-1]) and (b.kernel.lsigma, b.logNoise, b.mean.beta) == (c[-1], c[0], c[1])
    allbad = Theta.copy()
    allbad[:, 0] = -40.0
    with pytest.raises(NotPositiveDefinite):
        score_ensemble(m, "EI", p, Xs.T, allbad)
    with pytest.raises(ValueError, match="weights"):
        score_ensemble(m, "EI", p, Xs.T, Theta, weights=[1.0, -1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="columns"):
        score_ensemble(m, "EI", p, Xs.T, Theta[:, :-1])
    with pytest.raises(ValueError, match="not 'ThompsonDraw'"):
        score_ensemble(m, "ThompsonDraw", p, Xs.T, Theta)


# ---- construction errors and routes ------------------------------------------------------------------------------------------------
def test_construction_errors():
    import bohip
    from bohip.acquisition import (ExpectedImprovement, KnowledgeGradient, Marginalised, ThompsonSamplingSimple, UpperConfidenceBound,
                                   acquire_max, acquisitionfunction, setparams_)

    ok = dict(noisebounds=[-4.0, 1.0], meanbounds=[[-2.0], [2.0]], kernbounds=[[-3.0, -3.0, -2.0], [2.0, 2.0, 2.0]])
    o = bohip.MarginalGPOptimizer(every=5, samples=8, burn=5, seed=1, **ok)
    assert (o.every, o.i, o.options["samples"], o.options["burn"]) == (5, 0, 8, 5)
    for key, val in (("noisebounds", [-math.inf, 1.0]), ("meanbounds", [[-2.0], [math.inf]]), ("kernbounds", None),
                     ("kernbounds", [[-3.0, -math.inf, -2.0], [2.0, 2.0, 2.0]])):
        with pytest.raises(ValueError, match=key):
            bohip.MarginalGPOptimizer(**{**ok, key: val})
    bohip.MarginalGPOptimizer(domean=False, noisebounds=ok["noisebounds"], kernbounds=ok["kernbounds"])   # a fixed parameter needs no box
    for a in (ThompsonSamplingSimple(), KnowledgeGradient(), "EI"):
        with pytest.raises(ValueError, match="Marginalised takes"):
            Marginalised(a)
    a = Marginalised(UpperConfidenceBound())
    assert bohip.Marginalised is Marginalised and a.acq_id == "UCB" and "VALUE ONLY" in Marginalised.__doc__
    m = StubModel(d=2, n=7)
    assert setparams_(a, m) == setparams_(UpperConfidenceBound(), m) == a.params()[0]   # forwarded to the wrapped functor
    e = Marginalised(ExpectedImprovement())
    setparams_(e, m)
    assert e.params() == [6.0]                                    # tau = max y
    for call in (lambda: acquire_max(e, m, LB, UB, {"restarts": 1, "maxeval": 4}, np.random.default_rng(0)),
                 lambda: acquisitionfunction(e, m)(np.zeros((2, 3)))):
        with pytest.raises(ValueError, match="MarginalGPOptimizer"):
            call()


class EnsStub(StubModel):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.hyper_samples = (np.zeros((3, 5)), np.full(3, 1.0 / 3.0))

    def score_ensemble(self, acq, params, xs, Theta, weights=None, want_each=False, want_moments=False):
        from bohip.model import EnsembleScore

        self.calls.append(("score_ensemble", acq, list(params), xs.shape, Theta.shape, None if weights is None else len(weights)))
        sc = np.sin(5 * xs[0]) + xs[1]
        return EnsembleScore(sc, float(sc.max()), int(np.argmax(sc)), np.zeros(3, dtype=np.int64), None, None, None, "stub")


def test_marginalised_takes_the_candidate_set_route_and_the_others_keep_theirs():
    import warnings

    from bohip.acquisition import ExpectedImprovement, Marginalised, acquire_max, acquisitionfunction
    from bohip.utils import latin_hypercube_sampling

    m = EnsStub()
    acquire_max(ExpectedImprovement(), m, LB, UB, {"method": "LD_LBFGS", "restarts": 3, "maxeval": 50}, np.random.default_rng(1))
    assert m.calls == [("ascend", "EI", [2.0], (2, 3), 50, 1e-10, 1e-10)]
    m = EnsStub()
    sc = acquisitionfunction(ExpectedImprovement(0.25), m)(np.zeros((2, 5)))
    assert m.calls == [("score", "EI", [0.25], (2, 5))] and sc.shape == (5,)
    a = Marginalised(ExpectedImprovement(0.25))
    for method in ("LD_LBFGS", "GN_DIRECT_L", "LN_COBYLA"):       # accepted, not used, no warning
        m = EnsStub()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            fmax, xmax = acquire_max(a, m, LB, UB, {"method": method, "restarts": 2, "maxeval": 12}, np.random.default_rng(7))
        assert m.calls == [("score_ensemble", "EI", [2.0], (2, 12), (3, 5), 3)] * 2     # (tau <- max y = 2 by setparams)
        rng = np.random.default_rng(7)
        best = (-math.inf, None)
        for _ in range(2):
            cand = latin_hypercube_sampling(LB, UB, 12, rng)
            r = EnsStub().score_ensemble("EI", [2.0], cand, np.zeros((3, 5)))
            if r.best_val > best[0]:
                best = (r.best_val, cand[:, r.best_idx])
        assert fmax == best[0] and np.array_equal(xmax, best[1])
    m = EnsStub()
    vals = acquisitionfunction(a, m)(np.zeros((2, 4)))
    assert vals.shape == (4,) and m.calls[-1][0] == "score_ensemble"
    assert acquire_max(a, EnsStub(n=0), LB, UB, {"restarts": 1})[0] == -math.inf      # an empty model: nothing to do
