"""Constrained optimisation without a GPU: the ABI of include/bohip_con.h in every table that binds it, the NumPy twin
(tests/con_reference.py) against mpmath -- z from -40 to +10 on both sides of the switch, sigma^2 = 0 on both sides of the
threshold -- the twin's gradient against central differences, and the plumbing of Constrained / ConstrainedGPE through setparams_,
acquisitionfunction, acquire_max and BOpt on duck-typed members whose score is the twin."""
import ctypes as C
import functools
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import con_reference as cr   # noqa: E402
from conftest import ROOT, synth   # noqa: E402
from matern_reference import MaternGP   # noqa: E402

WANT = {"bohip_gp_predict_grad", "bohip_con_values", "bohip_gp_score_con"}
EPS = np.finfo(np.float64).eps


def test_con_header_exports_ctypes_and_julia_agree():
    """include/bohip_con.h <-> exports <-> _lib.CON_SIGNATURES <-> julia/BOHipCon.jl: the same symbols, the same types argument by
    argument, none of them in the other headers' tables; bohip.h keeps its 62."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_con.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "double": "double", "double*": "ptr(double)", "int*": "ptr(int)",
               "bohip_best*": "ptr(best)", "bohip_gp*": "ptr(void)", "bohip_gp**": "ptr(ptr(void))"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.CON_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES, _lib.ACQ_SIGNATURES,
                  _lib.KG_SIGNATURES, _lib.ENS_SIGNATURES, _lib.ENS_GRAD_SIGNATURES, _lib.MES_SIGNATURES):
        assert not WANT & set(other)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    main_syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & main_syms and len(main_syms) == 62 == len(_lib.SIGNATURES)
    assert "EXTENSION" in raw and "Gardner" in raw and "Gelbart" in raw
    assert int(re.search(r"#define\s+BOHIP_CON_CMAX\s+(\d+)", raw).group(1)) == 16 == _lib.CON_CMAX == cr.CMAX
    assert int(re.search(r"#define\s+BOHIP_CON_FEASIBILITY\s+\((-?\d+)\)", raw).group(1)) == -1 == _lib.CON_FEASIBILITY
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_double: "double", C.c_void_p: "ptr(void)", C.POINTER(C.c_void_p): "ptr(ptr(void))",
          C.POINTER(C.c_double): "ptr(double)", C.POINTER(C.c_int): "ptr(int)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)", "Ptr{Ptr{Cvoid}}": "ptr(ptr(void))",
                "Ptr{Float64}": "ptr(double)", "Ptr{Cint}": "ptr(int)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipCon.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.CON_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipCon.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert int(re.search(r"const CON_CMAX = (\d+)", src).group(1)) == 16
    for name in ("function predict_grad(", "function con_values(", "function score_constrained("):
        assert name in src, name


# ---- the twin against 50 digits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acq", cr.FORMS)
@pytest.mark.parametrize("C_", [0, 1, 5])
def test_twin_against_mpmath(acq, C_):
    """Every form, both senses, z in [-40, 10] with the switch and 0 on the grid, sigma^2 = 0 above, below and on the threshold, NaN
    moments: the twin within 2 x WORST of the 50-digit evaluator relative to max(1, |ref|), non-finite results equal."""
    shares = {}
    for R in (1, 257):
        thr, s, mu, var = cr.crafted(C_, R, seed=7 * C_ + R)
        f, L, pm, pv = cr.combine(acq, [0.3], thr, s, mu, var)
        fr, Lr, pmr, pvr = cr.mp_table(acq, [0.3], thr, s, mu, var)
        for name, got, ref, key in (("value", f, fr, "value"), ("dmu", pm, pmr, "dmu"), ("dvar", pv, pvr, "dvar")):
            shares[name] = max(shares.get(name, 0.0), cr.worst_share(got, ref, 2 * cr.WORST[key]))
        ok = np.isfinite(Lr)
        assert cr.worst_share(L[ok], Lr[ok], 2 * cr.WORST["value"]) <= 1.0
        if R > 1 and C_:
            assert L[7] == -np.inf and np.all(pm[1:, 7] == 0.0) and np.all(pv[:, 7] == 0.0)       # sigma^2 = 0 on the wrong side
            assert f[7] == (0.0 if acq in cr.PRODUCT else -np.inf)
            assert np.isnan(f[12]) and np.all(np.isnan(pm[:, 12]))                                # a NaN variance of a constraint
        if R > 1 and acq != "Feasibility":
            assert np.isnan(f[11]) and np.all(np.isnan(pv[:, 11]))                                # a NaN mean of the objective
        bv, bi = cr.record(f)
        assert bi < 0 or (np.isfinite(f[bi]) or f[bi] == np.inf)
        assert not np.any(np.isnan(pm[:, np.isfinite(f)])) and not np.any(np.isnan(pv[:, np.isfinite(f)]))
    print(f"{acq} C={C_}: worst share of 2 x WORST {shares}")
    assert max(shares.values()) <= 1.0, shares


@functools.lru_cache(maxsize=None)
def many_ref(acq, C_, R=257):
    """crafted_near's moments and the 50-digit table of one case (tests/test_limits_gpu.py shares the recipe)."""
    thr, s, mu, var = cr.crafted_near(C_, R, seed=7 * C_ + R)
    out = (thr, s, mu, var) + cr.mp_table(acq, [0.3], thr, s, mu, var)
    for a in out:
        a.setflags(write=False)
    return out


def live_share(fr):
    """The share of candidates whose 50-digit score is finite and not 0."""
    return float(np.mean(np.isfinite(fr) & (fr != 0.0)))


@pytest.mark.parametrize("acq", cr.FORMS)
@pytest.mark.parametrize("C_", [6, 15, 16])
def test_twin_against_mpmath_many_constraints(acq, C_):
    """More than 5 constraints, on crafted_near's grid (L within a few units of 0, the hard entries in every row): the twin within
    2 x WORST_MANY of the 50-digit evaluator -- the measurement WORST_MANY records.  Under the product forms at least half of the
    candidates have a finite score that is not 0, so the comparison is not 0 against 0."""
    thr, s, mu, var, fr, Lr, pmr, pvr = many_ref(acq, C_)
    assert all(thr[c] != thr[c + 1] and s[c] != s[c + 1] for c in range(C_ - 1)) and len(set(thr.tolist())) == C_
    f, L, pm, pv = cr.combine(acq, [0.3], thr, s, mu, var)
    shares = {k: cr.worst_share(got, ref, 2 * cr.WORST_MANY[k]) for k, got, ref in (("value", f, fr), ("dmu", pm, pmr), ("dvar", pv, pvr))}
    ok = np.isfinite(Lr)
    shares["logfeas"] = cr.worst_share(L[ok], Lr[ok], 2 * cr.WORST_MANY["value"])
    print(f"{acq} C={C_}: worst share of 2 x WORST_MANY {shares}; {live_share(fr):.2f} of the scores are finite and not 0")
    assert max(shares.values()) <= 1.0, shares
    assert live_share(fr) >= 0.5
    for c in range(C_):                                                         # the hard entries sit in every row, 5 to 15 included
        k = [(16 * c + i) % 257 for i in range(7)]
        assert L[k[4 if s[c] > 0 else 3]] == -np.inf and np.isnan(f[k[6]]) and Lr[k[0]] < -700.0
    assert not np.any(np.isnan(pm[:, np.isfinite(f)])) and not np.any(np.isnan(pv[:, np.isfinite(f)]))


def test_feasibility_with_one_constraint_is_log_pi():
    """BOHIP_CON_FEASIBILITY with C = 1, sense +1 and t = tau is log of ProbabilityOfImprovement, in a form that does not underflow."""
    rng = np.random.default_rng(3)
    mu, var = rng.normal(size=200), 10.0 ** rng.uniform(-4, 1, 200)
    f, L, _, _ = cr.combine("Feasibility", [], [0.2], [1], np.stack([mu, mu]), np.stack([var, var]))
    pi = cr.objective("PI", [0.2], mu, var)[0]
    ok = pi > 1e-3                                  # (1 + erf cancels in PI's own tail: its logarithm is a yardstick only away from it)
    assert ok.sum() > 100
    np.testing.assert_allclose(f[ok], np.log(pi[ok]), rtol=0, atol=1e-12)
    deep = cr.combine("Feasibility", [], [0.0], [1], np.array([[0.0], [-40.0]]), np.array([[1.0], [1.0]]))[0]
    assert np.isfinite(deep[0]) and deep[0] < -800.0


# ---- the twin's gradient against central differences -------------------------------------------------------------------------------
STEP = 1e-3
KERNS = ("Mat52Ard", "SEArd", "Mat12Iso")


def members(d=3):
    out = []
    for m, (kern, n) in enumerate(zip(KERNS, (17, 9, 17))):
        X, y, _ = synth(n, d, 1, seed=50 + m)
        ll = np.full(1 if kern.endswith("Iso") else d, -0.6 + 0.2 * m)
        out.append(MaternGP(kern, X, y - (0.5 if m else 0.0), ll, 0.3 - 0.1 * m, -1.5, 0.2 if m == 0 else 0.0))
    return out


def smooth_points(models, tau, thr, want=4):
    """Points of the unit box, by seed from the twin alone, where every member has sigma^2 > 0 and |z| < 6 and which keep 8 steps
    from every observation (Matérn 1/2 is not differentiable there)."""
    rng = np.random.default_rng(123)
    out = []
    while len(out) < want:
        x = rng.random(models[0].d)
        if min(np.min(np.abs(x[None, :] - m.X).max(axis=1)) for m in models) < 8 * STEP:
            continue
        mv = [m.predict(x[None, :]) for m in models]
        if all(v[0] > 1e-6 and abs(mu[0] - t) / math.sqrt(v[0]) < 6.0 for (mu, v), t in zip(mv, [tau] + list(thr))):
            out.append(x)
    return np.array(out)


@pytest.mark.parametrize("acq", cr.FORMS)
def test_twin_gradient_against_central_differences(acq):
    """Richardson's (4 D(h) - D(2h)) / 3 of the twin's own score, the recipe of test_ens_grad_host: what is left is bounded by
    |D(2h) - D(h)| / 3, rounding by 6 noise / h, noise the difference between the score by two routes (one solve for all points,
    MaternGP.predict per point) and never below 8 eps max|f|."""
    models = members()
    thr, senses = [-0.1, 0.4], [1, -1]
    tau = float(np.median(models[0].y))
    pts = smooth_points(models, tau, thr)
    ref = cr.score_con(models, acq, [tau], thr, senses, pts)

    def by_predict(P):
        mv = [m.predict(P) for m in models]
        return cr.combine(acq, [tau], thr, senses, np.array([a for a, _ in mv]), np.array([b for _, b in mv]))[0]

    val = by_predict(pts)
    np.testing.assert_allclose(ref["scores"], val, rtol=1e-9, atol=1e-12)
    noise = max(np.abs(ref["scores"] - val).max(), 8 * EPS * np.abs(val).max())
    d = pts.shape[1]
    for i, x in enumerate(pts):
        for k in range(d):
            e = np.zeros(d)
            e[k] = STEP
            f = by_predict(np.array([x + e, x - e, x + 2 * e, x - 2 * e]))
            d1, d2 = (f[0] - f[1]) / (2 * STEP), (f[2] - f[3]) / (4 * STEP)
            rich = (4.0 * d1 - d2) / 3.0
            bound = abs(d2 - d1) / 3.0 + 6.0 * noise / STEP
            err = abs(ref["grad"][i, k] - rich)
            assert err <= bound, (acq, i, k, ref["grad"][i, k], rich, err / bound)


# ---- plumbing on duck-typed members ---------------------------------------------------------------------------------------------------
class Duck:
    """What ConstrainedGPE and BOpt read of a member: dim, x, y, nobs, append_ -- and the twin's model of its observations."""

    def __init__(self, d, kern="SEArd"):
        self.dim, self.kern = d, kern
        self._x, self._y = np.zeros((d, 0)), np.zeros(0)

    x = property(lambda self: self._x)
    y = property(lambda self: self._y)
    nobs = property(lambda self: self._y.size)

    def append_(self, x, y):
        x = np.asarray(x, dtype=np.float64).reshape(self.dim, -1)
        self._x, self._y = np.concatenate([self._x, x], axis=1), np.concatenate([self._y, np.atleast_1d(y)])

    def gp(self):
        return MaternGP(self.kern, self._x.T, self._y, np.full(self.dim, -0.7), 0.0, -2.0, 0.0)


def twin_model(d, C_, thr, senses):
    """A ConstrainedGPE over Duck members whose score is con_reference.score_con (what the device call computes)."""
    from bohip.model import ConstrainedGPE, ConstrainedScore

    class TwinCon(ConstrainedGPE):
        calls = []

        def score(self, acq, params, xs, want_grad=False, want_moments=True):
            self.calls.append((acq, list(params), np.shape(xs), want_grad))
            ms = [None if (acq == "Feasibility" and i == 0) else m.gp() for i, m in enumerate(self.members)]
            tw = cr.score_con(ms, acq, list(params), self.thresholds, self.senses, np.asarray(xs).T, want_grad)
            return ConstrainedScore(tw["scores"], tw["logfeas"], tw["grad"].T if want_grad else None, tw["mu"], tw["var"],
                                    tw["best_val"], tw["best_idx"])

    return TwinCon(Duck(d), [Duck(d) for _ in range(C_)], thr, senses)


def test_incumbent_rule_and_the_feasibility_fallback():
    import bohip

    m = twin_model(2, 2, [0.0, 1.0], [1, -1])
    a = bohip.Constrained(bohip.ExpectedImprovement())
    assert m.feasible_incumbent() is None
    m.update_(np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]), [5.0, 3.0, 4.0], [[-1.0, 0.5, -0.2], [0.0, 2.0, 0.5]])
    assert m.feasible_incumbent() is None and not m.feasible_mask().any()      # 0: g1 < 0; 1: g2 > 1; 2: g1 < 0
    bohip.setparams_(a, m)
    assert a.feasibility_only and a.acq_id == "Feasibility"
    m.update_(np.array([[0.7], [0.8]]), [1.5], [[0.0], [1.0]])                  # on both thresholds: feasible
    m.update_(np.array([[0.9], [0.1]]), [1.0], [[2.0], [-3.0]])
    assert m.feasible_incumbent() == 1.5 and list(m.feasible_mask()) == [False, False, False, True, True]
    bohip.setparams_(a, m)
    assert not a.feasibility_only and a.acq_id == "EI" and a.params() == [1.5] and a.a.tau == 1.5
    assert m.nobs == 5 and m.x.shape == (2, 5) and all(c.nobs == 5 for c in m.constraints)
    f = bohip.acquisitionfunction(a, m)
    xs = np.random.default_rng(0).random((2, 7))
    np.testing.assert_array_equal(f(xs), m.score("EI", [1.5], xs).scores)
    with pytest.raises(ValueError):
        f(xs[:, 0])
    assert bohip.defaultoptions(type(m), type(a)) == dict(method="LD_LBFGS", restarts=1, maxeval=1024)


def test_refusals():
    import bohip
    from bohip.model import ConstrainedGPE

    for bad in (bohip.UpperConfidenceBound(), bohip.MutualInformation(), bohip.MaxMean(), bohip.ThompsonSamplingSimple(),
                bohip.KnowledgeGradient(), "EI"):
        with pytest.raises(ValueError):
            bohip.Constrained(bad)
    for ok in (bohip.ExpectedImprovement(), bohip.ProbabilityOfImprovement(), bohip.LogExpectedImprovement()):
        assert bohip.Constrained(ok).acq_id == ok.acq_id
    with pytest.raises(ValueError):
        ConstrainedGPE(Duck(2), [Duck(2)], [0.0, 1.0], [1])                      # lengths
    with pytest.raises(ValueError):
        ConstrainedGPE(Duck(2), [Duck(2)], [np.inf], [1])
    with pytest.raises(ValueError):
        ConstrainedGPE(Duck(2), [Duck(2)], [0.0], [0])
    with pytest.raises(ValueError):
        ConstrainedGPE(Duck(2), [Duck(3)], [0.0], [1])
    with pytest.raises(ValueError):
        ConstrainedGPE(Duck(2), [Duck(2)] * 17, np.zeros(17), np.ones(17))
    m = twin_model(2, 1, [0.0], [1])
    lo, hi = [0.0, 0.0], [1.0, 1.0]
    kw = dict(verbosity=bohip.Silent, maxiterations=6, initializer_iterations=3)
    with pytest.raises(ValueError, match="Constrained"):
        bohip.BOpt(lambda x: (0.0, 0.0), m, bohip.ExpectedImprovement(), bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="Constrained"):
        bohip.BOpt(lambda x: (0.0, 0.0), m, bohip.Marginalised(bohip.ExpectedImprovement()), bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="Constrained"):
        bohip.BOpt(lambda x: 0.0, Duck(2), bohip.Constrained(bohip.ExpectedImprovement()), bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="batchsize"):
        bohip.BOpt(lambda x: (0.0, 0.0), m, bohip.Constrained(bohip.ExpectedImprovement()), bohip.NoModelOptimizer(), lo, hi,
                   batchsize=2, **kw)
    o = bohip.BOpt(lambda x: 0.0, m, bohip.Constrained(bohip.ExpectedImprovement()), bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="g_1"):
        bohip.boptimize_(o)                                                      # func must return (y, g_1)

    class MultiGPE(Duck):
        pass

    with pytest.raises(ValueError, match="MultiGPE"):
        ConstrainedGPE(Duck(2), [MultiGPE(2)], [0.0], [1])


@pytest.mark.parametrize("sense", ["Max", "Min"])
def test_bopt_on_the_twin(sense):
    """A short loop on the twin: sense = Min flips y only (g and the thresholds keep their sign), every proposal is in the box, the
    first searches are feasibility-only while no feasible point exists, and the recorded optimum counts feasible points only."""
    import bohip

    sgn = 1.0 if sense == "Max" else -1.0
    seen = []

    def func(x):                                    # best value at (0.8, 0.8), feasible inside the disc |x - (0.3, 0.3)| <= 0.35
        y = -sgn * ((x[0] - 0.8) ** 2 + (x[1] - 0.8) ** 2)
        g = 0.35 ** 2 - ((x[0] - 0.3) ** 2 + (x[1] - 0.3) ** 2)
        seen.append((np.array(x), y, g))
        return y, g

    m = twin_model(2, 1, [0.0], [1])
    a = bohip.Constrained(bohip.LogExpectedImprovement())
    init = np.array([[0.9, 0.05, 0.95], [0.9, 0.95, 0.1]])                      # three infeasible points
    o = bohip.BOpt(func, m, a, bohip.NoModelOptimizer(), [0.0, 0.0], [1.0, 1.0], sense=getattr(bohip, sense), maxiterations=9,
                   verbosity=bohip.Silent, initializer=[init[:, j] for j in range(3)], initializer_iterations=3,
                   acquisitionoptions=dict(maxeval=128, refine=2), rng=np.random.default_rng(5))
    assert a.feasibility_only
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = bohip.boptimize_(o)
    X = np.array([s[0] for s in seen])
    assert len(seen) == 9 and np.all(X >= 0.0) and np.all(X <= 1.0)
    np.testing.assert_array_equal(m.y, sgn * np.array([s[1] for s in seen]))    # y flipped under Min ...
    np.testing.assert_array_equal(m.constraints[0].y, np.array([s[2] for s in seen]))   # ... g never
    assert m.calls[0][0] == "Feasibility" and m.calls[0][2] == (2, 128)
    feas = [s for s in seen if s[2] >= 0.0]
    assert feas, "the feasibility-only searches found no feasible point"
    best = max(feas, key=lambda s: sgn * s[1])
    assert res["observed_optimum"] == best[1] and np.array_equal(res["observed_optimizer"], best[0])
    assert any(c[0] == "LogEI" for c in m.calls) and any(c[3] for c in m.calls)   # the objective's turn, and the gradient route
    infeasible_better = [s for s in seen if s[2] < 0.0 and sgn * s[1] > sgn * best[1]]
    assert infeasible_better, "the initial design holds better infeasible points: the optimum must not count them"


def test_acquire_max_refine_never_below_the_candidates():
    import bohip

    m = twin_model(2, 1, [0.0], [1])
    rng = np.random.default_rng(2)
    X = rng.random((2, 12))
    m.update_(X, np.sin(3 * X).sum(0), [0.3 - np.abs(X - 0.5).sum(0)])
    a = bohip.Constrained(bohip.ExpectedImprovement())
    f0, x0 = bohip.acquire_max(a, m, [0.0, 0.0], [1.0, 1.0], dict(maxeval=64, restarts=1), np.random.default_rng(9))
    f1, x1 = bohip.acquire_max(a, m, [0.0, 0.0], [1.0, 1.0], dict(maxeval=64, restarts=1, refine=3), np.random.default_rng(9))
    assert f1 >= f0 and np.all(x1 >= 0.0) and np.all(x1 <= 1.0)
    assert [c[3] for c in m.calls].count(False) == 2 and m.calls[0][2] == (2, 64)
