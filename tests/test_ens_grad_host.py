"""The gradient of the marginalised acquisition without a GPU: the ABI of include/bohip_ens_grad.h in every table that binds it, the
NumPy twin (tests/ens_grad_reference.py) against central differences of tests/ens_reference.py's scores, score_ensemble_grad's host
route against the twin on a duck-typed model, and the plumbing of the "refine" option through acquire_max."""
import ctypes as C
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ens_grad_reference as eg   # noqa: E402
import ens_reference as er   # noqa: E402
from conftest import ROOT, synth   # noqa: E402
from matern_reference import KERNELS   # noqa: E402
from test_ens_host import DuckModel, EnsStub, host_case   # noqa: E402
from test_kg_host import LB, UB   # noqa: E402

WANT = {"bohip_gp_score_ens_grad"}


def test_ens_grad_header_exports_ctypes_and_julia_agree():
    """include/bohip_ens_grad.h <-> exports <-> _lib.ENS_GRAD_SIGNATURES <-> julia/BOHipEnsGrad.jl: the same symbol, the same types
    argument by argument, in none of the other headers' tables (the pattern of tests/test_ens_host.py)."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_ens_grad.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "double": "double", "double*": "ptr(double)", "int64_t*": "ptr(int64)",
               "bohip_best*": "ptr(best)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.ENS_GRAD_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES, _lib.ACQ_SIGNATURES, _lib.KG_SIGNATURES,
                  _lib.ENS_SIGNATURES):
        assert not WANT & set(other)
    for name in ("bohip.h", "bohip_ens.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", text))
        assert not WANT & syms
        assert len(syms) == (62 if name == "bohip.h" else 1)
    assert len(_lib.SIGNATURES) == 62 and set(_lib.ENS_SIGNATURES) == {"bohip_gp_score_ens"}
    assert "EXTENSION" in raw and "Snoek" in raw
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_double: "double", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int64): "ptr(int64)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)",
                "Ptr{Int64}": "ptr(int64)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipEnsGrad.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.ENS_GRAD_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
        assert len(args) == 16
    assert "function score_ensemble_grad" in src
    assert 'include("BOHipEnsGrad.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)
    mk = open(os.path.join(ROOT, "bayesianoptimization.jl_amd", "csrc", "Makefile")).read()
    assert "kernels_ens.hip" in mk and "bohip_ens_grad.h" in mk
    dp = C.POINTER(C.c_double)                                    # a null handle is reported, nothing runs
    th, xs, p, g = np.zeros(4), np.zeros(2), np.zeros(2), np.zeros(2)
    best = _lib.Best()
    fn = _lib.load().bohip_gp_score_ens_grad
    rc = fn(None, _lib.ACQ["EI"], p.ctypes.data_as(dp), 1, th.ctypes.data_as(dp), None, xs.ctypes.data_as(dp), 1, None, g.ctypes.data_as(dp),
            None, None, None, None, None, C.byref(best))
    assert rc == _lib.E_ARG and b"null" in _lib.load().bohip_last_error()


# ---- the twin against central differences of the value twin --------------------------------------------------------------------------
ACQS = [("EI", None), ("PI", None), ("UCB", [2.5]), ("MI", [1.0, 0.3]), ("MaxMean", []), ("LogEI", None)]
STEP = 1e-3   # in a box of side 1 with length-scales e^-1.6 .. e^0.4


def smooth_points(kern, X, y, Theta, tau, want=4):
    """Points of the unit box, by seed from the twin alone, where every setting has sigma^2 > 0 and |z| < 6 -- and, so that the
    differences see no kink, keeps a distance of 8 steps from every observation (Matérn 1/2 is not differentiable there)."""
    rng = np.random.default_rng(123)
    out = []
    models = [er.row_model(kern, X, y, t) for t in Theta]
    while len(out) < want:
        x = rng.random(X.shape[1])
        if np.min(np.abs(x[None, :] - X).max(axis=1)) < 8 * STEP:
            continue
        mv = [m.predict(x[None, :]) for m in models]
        if all(v[0] > 1e-6 and abs(mu[0] - tau) / math.sqrt(v[0]) < 6.0 for mu, v in mv):
            out.append(x)
    return np.array(out)


@pytest.mark.parametrize("kern", list(KERNELS))
def test_twin_gradient_against_central_differences(kern):
    """The yardstick before the device is held to it.  f = ens_reference.score_ens's averaged score.  With D(s) the central
    difference of step s, D(h) = f' + c h^2 + O(h^4) and D(2h) = f' + 4 c h^2 + O(h^4), so (4 D(h) - D(2h)) / 3 = f' + O(h^4) and the
    h^2 term it removes, |D(2h) - D(h)| / 3, bounds what is left many times over (the O(h^4) term is smaller by (h / length-scale)^2).
    Rounding: the twin computes the same scores by two routes (a triangular solve per point in score_grad, one for all points in
    score_ens); the largest difference between the two at these points, `noise` (never taken below 8 eps max|f|), is a sample of the
    error one score carries.  Four scores with errors e_i enter (4 D(h) - D(2h)) / 3 with weights 2 / (3 h), 2 / (3 h), 1 / (12 h),
    1 / (12 h): at most 1.5 noise / h; four times that is allowed, since a sample is not a bound."""
    N, d, H = 17, 3, 3
    X, y, _ = synth(N, d, 1, seed=41)
    Theta = np.concatenate([[-1.5, 0.2], np.full(1 if KERNELS[kern][1] else d, -0.6), [0.3]])
    Theta = Theta + np.random.default_rng(9).uniform(-1, 1, (H, Theta.size))
    w = np.array([0.5, 1.0, 2.5])
    tau = float(np.median(y))
    pts = smooth_points(kern, X, y, Theta, tau)
    for acq, p in ACQS:
        p = [tau] if p is None else p
        ref = eg.score_ens_grad(kern, X, y, Theta, acq, p, pts, w)
        val = er.score_ens(kern, X, y, Theta, acq, p, pts, w)["scores"]
        np.testing.assert_allclose(ref["scores"], val, rtol=1e-10, atol=1e-13)
        noise = max(np.abs(ref["scores"] - val).max(), 8 * np.finfo(float).eps * np.abs(val).max())
        for i, x in enumerate(pts):
            for k in range(d):
                e = np.zeros(d)
                e[k] = STEP
                f = er.score_ens(kern, X, y, Theta, acq, p, np.array([x + e, x - e, x + 2 * e, x - 2 * e]), w)["scores"]
                d1, d2 = (f[0] - f[1]) / (2 * STEP), (f[2] - f[3]) / (4 * STEP)
                rich = (4.0 * d1 - d2) / 3.0
                bound = abs(d2 - d1) / 3.0 + 6.0 * noise / STEP
                err = abs(ref["grad"][i, k] - rich)
                assert err <= bound, (kern, acq, i, k, ref["grad"][i, k], rich, err / bound)


# ---- score_ensemble_grad's host route ------------------------------------------------------------------------------------------------
class DuckGradModel(DuckModel):
    def score_grad(self, acq, params, xs):
        sc, g = self._gp().score_grad(acq, list(params), np.asarray(xs).T)
        return sc, np.asfortranarray(g.T)


@pytest.mark.parametrize("acq,params", [("EI", None), ("PI", None), ("UCB", [2.5]), ("MI", [1.0, 0.3]), ("MaxMean", [])])
def test_host_route_equals_the_twin_and_restores_the_model(acq, params):
    from bohip.model import score_ensemble_grad

    kern, X, y, Xs, c, Theta = host_case()
    params = [float(np.median(y))] if params is None else params
    m = DuckGradModel(kern, X, y, c)
    mean0 = m.mean
    for weights in (None, np.array([0.5, 1.0, 0.0, 2.5])):           # (a row of weight 0 takes no part)
        res, grad, each_grad = score_ensemble_grad(m, acq, params, Xs.T, Theta, weights=weights, want_each=True)
        ref = eg.score_ens_grad(kern, X, y, Theta, acq, params, Xs, weights)
        assert res.route == "host" and np.all(res.pivot == 0) and grad.shape == (3, 9) and each_grad.shape == (4, 3, 9)
        np.testing.assert_array_equal(res.scores, ref["scores"])
        np.testing.assert_array_equal(res.each, ref["each"])
        np.testing.assert_array_equal(each_grad, ref["each_grad"].transpose(0, 2, 1))
        np.testing.assert_array_equal(grad, ref["grad"].T)
        assert (res.best_val, res.best_idx) == (ref["best_val"], ref["best_idx"])
        assert np.array_equal(m.kernel.ll, c[2:-1]) and (m.kernel.lsigma, m.logNoise) == (c[-1], c[0]) and m.mean is mean0
    if weights is not None:
        two = eg.score_ens_grad(kern, X, y, Theta[[0, 1, 3]], acq, params, Xs, weights[[0, 1, 3]])
        np.testing.assert_array_equal(grad, two["grad"].T)
    res, grad = score_ensemble_grad(m, acq, params, Xs.T, Theta)
    assert res.each is None and grad.shape == (3, 9)


def test_host_route_reports_a_failed_row_and_still_restores():
    from bohip import NotPositiveDefinite
    from bohip.model import score_ensemble_grad

    kern, X, y, Xs, c, Theta = host_case()
    p = [float(np.median(y))]
    m = DuckGradModel(kern, X, y, c)
    bad = Theta.copy()
    bad[1, 0] = -40.0                                             # raises in the model
    bad[3, 2] = np.nan                                            # never reaches it
    res, grad, each_grad = score_ensemble_grad(m, "EI", p, Xs.T, bad, want_each=True)
    assert res.pivot.tolist() == [0, 1, 0, 1]
    assert np.all(np.isnan(res.each[[1, 3]])) and np.all(np.isnan(each_grad[[1, 3]])) and np.all(np.isfinite(each_grad[[0, 2]]))
    ref = eg.score_ens_grad(kern, X, y, Theta[[0, 2]], "EI", p, Xs)
    np.testing.assert_array_equal(res.scores, ref["scores"])
    np.testing.assert_array_equal(grad, ref["grad"].T)
    assert np.array_equal(m.kernel.ll, c[2:-1]) and (m.kernel.lsigma, m.logNoise, m.mean.beta) == (c[-1], c[0], c[1])

    class Broken(DuckGradModel):
        def score_grad(self, *a, **k):
            raise RuntimeError("device lost")

    b = Broken(kern, X, y, c)
    with pytest.raises(RuntimeError, match="device lost"):
        score_ensemble_grad(b, "EI", p, Xs.T, Theta)
    assert np.array_equal(b.kernel.ll, c[2:-1]) and (b.kernel.lsigma, b.logNoise, b.mean.beta) == (c[-1], c[0], c[1])
    allbad = Theta.copy()
    allbad[:, 0] = -40.0
    with pytest.raises(NotPositiveDefinite):
        score_ensemble_grad(m, "EI", p, Xs.T, allbad)
    with pytest.raises(ValueError, match="weights"):
        score_ensemble_grad(m, "EI", p, Xs.T, Theta, weights=[1.0, -1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="columns"):
        score_ensemble_grad(m, "EI", p, Xs.T, Theta[:, :-1])
    with pytest.raises(ValueError, match="not 'ThompsonDraw'"):
        score_ensemble_grad(m, "ThompsonDraw", p, Xs.T, Theta)


# ---- plumbing of "refine" --------------------------------------------------------------------------------------------------------------
PEAK = np.array([0.37, 0.61])


class BumpStub(EnsStub):
    """The averaged score is the concave bump 2 - |x - PEAK|^2, its gradient analytic."""

    def score_ensemble(self, acq, params, xs, Theta, weights=None, want_each=False, want_moments=False):
        from bohip.model import EnsembleScore

        self.calls.append(("score_ensemble", acq, list(params), xs.shape, Theta.shape, None if weights is None else len(weights)))
        sc = 2.0 - ((xs - PEAK[:, None]) ** 2).sum(axis=0)
        return EnsembleScore(sc, float(sc.max()), int(np.argmax(sc)), np.zeros(3, dtype=np.int64), None, None, None, "stub")

    def score_ensemble_grad(self, acq, params, xs, Theta, weights=None, want_each=False):
        from bohip.model import EnsembleScore

        self.calls.append(("score_ensemble_grad", acq, list(params), xs.shape, Theta.shape, None if weights is None else len(weights)))
        sc = 2.0 - ((xs - PEAK[:, None]) ** 2).sum(axis=0)
        res = EnsembleScore(sc, float(sc.max()), int(np.argmax(sc)), np.zeros(3, dtype=np.int64), None, None, None, "stub")
        return res, -2.0 * (xs - PEAK[:, None])


def test_refine_zero_is_the_candidate_route_and_refine_climbs():
    from bohip.acquisition import ExpectedImprovement, Marginalised, acquire_max, defaultoptions

    a = Marginalised(ExpectedImprovement(0.25))
    assert defaultoptions(BumpStub, Marginalised) == dict(method="LD_LBFGS", restarts=10, maxeval=2000)      # unchanged
    base = {"method": "LD_LBFGS", "restarts": 2, "maxeval": 12}
    runs = {}
    for name, extra in (("none", {}), ("zero", {"refine": 0}), ("four", {"refine": 4})):
        m = BumpStub()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            runs[name] = acquire_max(a, m, LB, UB, {**base, **extra}, np.random.default_rng(7)), m.calls
    want = [("score_ensemble", "EI", [2.0], (2, 12), (3, 5), 3)] * 2
    assert runs["none"][1] == want == runs["zero"][1]             # refine = 0: exactly today's calls ...
    assert runs["none"][0][0] == runs["zero"][0][0] and np.array_equal(runs["none"][0][1], runs["zero"][0][1])   # ... and result
    (f4, x4), calls4 = runs["four"]
    assert calls4[:2] == want and len(calls4) > 2                 # the same candidate stage, the same draws, then the ascent
    assert all(c == ("score_ensemble_grad", "EI", [2.0], (2, 4), (3, 5), 3) for c in calls4[2:])
    assert len(calls4) - 2 <= 12                                  # at most maxeval evaluations per start
    f0 = runs["none"][0][0]
    assert f4 > f0 and np.all(x4 >= LB) and np.all(x4 <= UB)      # strictly above the candidate maximum, inside the box
    assert f4 == 2.0 - ((x4 - PEAK) ** 2).sum() and np.abs(x4 - PEAK).max() < 1e-6
    m = BumpStub()                                                # a peak outside the box: the ascent stops on the boundary
    fb, xb = acquire_max(a, m, LB, np.array([0.3, 0.5]), {**base, "refine": 3}, np.random.default_rng(7))
    np.testing.assert_allclose(xb, [0.3, 0.5], atol=1e-9)
    with pytest.raises(ValueError, match="unknown acquisition option"):
        acquire_max(a, BumpStub(), LB, UB, {**base, "refines": 4}, np.random.default_rng(7))
    with pytest.raises(NotImplementedError, match="score_ensemble_grad"):
        acquire_max(a, EnsStub(), LB, UB, {**base, "refine": 4}, np.random.default_rng(7))
    assert [c[0] for c in EnsStub().calls] == []


def test_refine_is_accepted_unused_by_the_other_acquisitions():
    """BOpt hands one options record to the acquisition's search and to its closing MaxMean search, so a record with "refine" must
    pass everywhere; only Marginalised acts on it, and its docstring says so."""
    from bohip.acquisition import ExpectedImprovement, Marginalised, MaxMean, acquire_max

    for a in (ExpectedImprovement(0.25), MaxMean()):
        calls = []
        for extra in ({}, {"refine": 4}):
            m = EnsStub()
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                acquire_max(a, m, LB, UB, {"restarts": 3, "maxeval": 50, **extra}, np.random.default_rng(1))
            calls.append(m.calls)
        assert calls[0] == calls[1] and [c[0] for c in calls[0]] == ["ascend"]
    assert "accepts the key unused" in Marginalised.__doc__


# ---- the seeds of the device's ascent test, on the host route with the twin ------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 8])
def test_the_ascent_seeds_rise_strictly_without_a_device(d):
    """tests/test_ens_grad_gpu.py::test_refine_climbs_above_the_candidate_maximum asks the device for a rise above both score tolerances
    at these seeds; here the same search runs on the host route (set_params_ + score / score_grad on the twin), so that the claim
    cannot go stale: refine = 4 ends strictly above refine = 0 by more than 100 times the two tolerances together."""
    from bohip.acquisition import Marginalised, NoBetaScaling, UpperConfidenceBound, acquire_max
    from bohip.model import score_ensemble, score_ensemble_grad
    from test_ens_gpu import score_tols
    from test_ens_grad_gpu import ASCENT, ascent_problem
    from test_fit_gpu import centre

    kern, X, y, Theta = ascent_problem(d)
    w = np.full(4, 0.25)
    m = DuckGradModel(kern, X, y, centre(kern, d))
    m.hyper_samples, m.x = (Theta, w), X.T
    m.score_ensemble = lambda *a, **k: score_ensemble(m, *a, **k)
    m.score_ensemble_grad = lambda *a, **k: score_ensemble_grad(m, *a, **k)
    a = Marginalised(UpperConfidenceBound(NoBetaScaling(), 2.0))
    lb, ub = np.zeros(d), np.ones(d)
    opts = dict(restarts=1, maxeval=256)
    f0, x0 = acquire_max(a, m, lb, ub, opts, np.random.default_rng(ASCENT[d]), setparams=False)
    f4, x4 = acquire_max(a, m, lb, ub, {**opts, "refine": 4}, np.random.default_rng(ASCENT[d]), setparams=False)

    def tol(x):
        ref = er.score_ens(kern, X, y, Theta, "UCB", a.params(), x[None, :], w)
        return float((w[:, None] * score_tols(ref["models"], ref["each"])).sum(axis=0)[0])

    print(f"d={d}: refine=0 f {f0:.12g}, refine=4 f {f4:.12g}, rise {f4 - f0:.3g}, tolerances {tol(x0):.3g} {tol(x4):.3g}")
    assert np.all(x4 >= lb) and np.all(x4 <= ub)
    assert f4 - f0 > 100.0 * (tol(x0) + tol(x4))
