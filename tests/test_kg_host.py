"""The knowledge gradient without a GPU: the ABI of include/bohip_kg.h in every table that binds it, the NumPy twin of the march
(tests/kg_reference.py kg_march) against the independent sorted-hull form (kg_hull) and on crafted lines, and the plumbing of
KnowledgeGradient through acquisitionfunction / defaultoptions / acquire_max against a recording stub model."""
import ctypes as C
import math
import os
import re
import sys
from decimal import Decimal, getcontext

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_reference as kr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_kg", "bohip_kg_lines"}
EPS = np.finfo(np.float64).eps


def test_kg_header_exports_ctypes_and_julia_agree():
    """include/bohip_kg.h <-> exports <-> _lib.KG_SIGNATURES <-> julia/BOHipKG.jl: the same symbols, the same types argument by
    argument, none of them in the other headers' tables (tests/test_qei_host.py does this for q-EI)."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_kg.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "double": "double", "double*": "ptr(double)", "int32_t*": "ptr(int32)",
               "bohip_best*": "ptr(best)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.KG_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES, _lib.ACQ_SIGNATURES):
        assert not WANT & set(other)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    main_syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & main_syms and len(main_syms) == 62 == len(_lib.SIGNATURES)
    assert "EXTENSION" in raw and "Frazier" in raw
    assert int(re.search(r"#define\s+BOHIP_KG_RMAX\s+(\d+)", raw).group(1)) == _lib.KG_RMAX == 8192
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_double: "double", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int32): "ptr(int32)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)",
                "Ptr{Int32}": "ptr(int32)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipKG.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.KG_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipKG.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert int(re.search(r"const KG_RMAX = (\d+)", src).group(1)) == 8192
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_null_handle_and_bad_sizes_are_reported_before_any_device_work():
    from bohip import _lib

    full = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a, B, kg, nseg = np.zeros(2), np.zeros(4), np.zeros(2), np.zeros(2, dtype=np.int32)
    pa, pB, pk, pn = a.ctypes.data_as(dp), B.ctypes.data_as(dp), kg.ctypes.data_as(dp), nseg.ctypes.data_as(ip)
    assert full.bohip_kg_lines(None, pa, pB, 2, 2, pk, pn) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()
    assert full.bohip_gp_kg(None, pB, 2, 2, pk, pn, None, None) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()
    for R, E, word in [(0, 1, b"at least 1"), (2, 0, b"at least 1"), (-1, -1, b"at least 1"), (2, 3, b"E exceeds")]:
        assert full.bohip_kg_lines(None, pa, pB, R, E, pk, pn) == _lib.E_ARG
        assert word in full.bohip_last_error()
        assert full.bohip_gp_kg(None, pB, R, E, pk, pn, None, None) == _lib.E_ARG
        assert word in full.bohip_last_error()


# ---- the twin against the sorted hull -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 64, 300, 1000])
def test_march_agrees_with_the_sorted_hull_on_random_lines(R):
    """|kg_march - kg_hull| <= 64 eps (max|a| + max|b|): the hull form's own cancellation against max a.  Continuous random lines have
    no exact multi-line crossing, so nseg is the hull's vertex count minus one."""
    rng = np.random.default_rng(500 + R)
    worst = 0.0
    for trial in range(8):
        a = rng.standard_normal(R) * rng.uniform(0.1, 2.0)
        b = rng.standard_normal(R) * rng.uniform(0.1, 2.0)
        kg, nseg = kr.kg_march(a, b)
        hv, nv = kr.kg_hull(a, b)
        bound = 64 * EPS * (np.abs(a).max() + np.abs(b).max())
        worst = max(worst, abs(kg - hv) / bound)
        assert abs(kg - hv) <= bound, (R, trial, kg, hv)
        assert nseg == nv - 1 and kg >= 0.0
        if R > 1:                                                         # a Monte-Carlo look at the definition itself: 5 standard errors
            Z = np.random.default_rng(trial).standard_normal(4000)
            env = (a[:, None] + b[:, None] * Z[None, :]).max(axis=0) - a.max()
            assert abs(env.mean() - kg) <= 5.0 * env.std(ddof=1) / math.sqrt(Z.size) + 1e-12
    print(f"R = {R}: worst |march - hull| / bound = {worst:.3f}")


def test_crafted_lines():
    nan, inf = math.nan, math.inf
    assert kr.kg_march([0, 0, 0], [-1, 0, 1]) == (0.7978845608028654, 1)                  # 2 phi(0): the middle line is never on top
    assert kr.kg_march([1.0, 3.0, 2.0], [0.5, 0.5, 0.5]) == (0.0, 0)                      # equal slopes
    assert kr.kg_march([2.5], [-0.3]) == (0.0, 0)                                         # one line
    kg, nseg = kr.kg_march([0, 1, 0], [-1, 0, 1])
    assert nseg == 2 and kg == pytest.approx(0.16663094117537258, rel=4 * EPS)
    assert kg == pytest.approx(kr.kg_hull([0, 1, 0], [-1, 0, 1])[0], abs=64 * EPS * 2)
    base = kr.kg_march([0, 1, 0], [-1, 0, 1])
    assert kr.kg_march([0, nan, 1, 5.0, 0, inf, 7.0], [-1, 9.0, 0, nan, 1, 0.5, -inf]) == base     # NaN / Inf lines are ignored
    assert kr.kg_march([nan, 1.0], [0.0, inf]) == (0.0, 0)                                # ... and none is left
    b = np.linspace(-1.0, 1.0, 257)
    kg, nseg = kr.kg_march(-b * b, b)                                                     # the parabola: every line is live
    assert nseg == 256 and kg == pytest.approx(kr.kg_hull(-b * b, b)[0], abs=64 * EPS * 2)
    q = np.round(np.random.default_rng(3).standard_normal((2, 200)) * 4) / 4              # quarter-rounded: ties everywhere
    kg, nseg = kr.kg_march(q[0], q[1])
    assert kg == pytest.approx(kr.kg_hull(q[0], q[1])[0], abs=64 * EPS * (np.abs(q[0]).max() + np.abs(q[1]).max()))
    perm = np.random.default_rng(4).permutation(200)                                      # the order of the lines does not matter
    assert kr.kg_march(q[0][perm], q[1][perm]) == (kg, nseg)


def deep_tail_value(s, t):
    """s h(-t) in 60 digits, by the asymptotic series h(-t) = phi(t) sum_k (-1)^k (2k + 1)!! / t^(2k + 2) -- not the continued
    fraction the library uses.  At t = 40 the terms fall until k ~ 800; 30 of them leave a remainder below 1e-57 of the sum."""
    getcontext().prec = 60
    t = Decimal(t)
    tot, term = Decimal(0), Decimal(1) / (t * t)
    for k in range(30):
        tot += term
        term *= -Decimal(2 * k + 3) / (t * t)
    phi = (-(t * t) / 2).exp() / (Decimal(2) * Decimal("3.14159265358979323846264338327950288419716939937510582097494")).sqrt()
    return Decimal(s) * phi * tot


def test_deep_tail_keeps_its_relative_accuracy():
    """a = (0, -40 s), b = (0, s): one crossing at z = 40, KG = s h(-40) with h(-40) ~ 9.1e-352, below the smallest double.  The two
    halves of the exponential keep the product alive: at s = 1e100 the value is ~9.1e-252.  Bound: libm's exp (< 1 ulp) enters
    twice and ten roundings follow, < 16 eps; the continued fraction at depth 40 is converged far below eps at t = 40."""
    s = 1e100
    kg, nseg = kr.kg_march([0.0, -40.0 * s], [0.0, s])
    want = deep_tail_value(s, 40)
    assert nseg == 1 and 0.0 < kg < math.inf
    assert abs(Decimal(kg) - want) / want < Decimal(16 * EPS)
    kg11, _ = kr.kg_march([0.0, -11.0], [0.0, 1.0])                                       # a KG of 1e-29, through the same form
    want11 = deep_tail_value(1.0, 11)                                                     # (series remainder at t = 11: < 1e-18 of the sum)
    assert 1e-30 < kg11 < 1e-28 and abs(Decimal(kg11) - want11) / want11 < Decimal(16 * EPS)
    h4 = kr.kg_term(1.0, -4.0)                                                            # the two forms meet at the switch
    assert kr.kg_term(1.0, math.nextafter(-4.0, 0.0)) == pytest.approx(h4, rel=1e-13)


# ---- the plumbing against a stub model ------------------------------------------------------------------------------------------
class StubModel:
    """Records its calls.  kg answers with the twin on lines made from the candidates themselves."""

    def __init__(self, d=2, n=3):
        self.dim = d
        self.x = np.zeros((d, n), order="F")
        self.y = np.arange(n, dtype=float)
        self.calls = []

    @property
    def nobs(self):
        return self.y.size

    def kg(self, xs, n_eval=None):
        from bohip.model import KGResult

        self.calls.append(("kg", xs.shape, n_eval))
        a, R = np.sin(3 * xs[0]), xs.shape[1]
        vals = np.array([kr.kg_march(a, np.cos(2 * xs[1] + e))[0] for e in range(R)])
        return KGResult(vals, np.zeros(R, dtype=np.int32), a, float(vals.max()), int(np.argmax(vals)))

    def score(self, acq, params, xs, want_scores=True):
        self.calls.append(("score", acq, list(params), np.asarray(xs).shape))
        n = np.asarray(xs).shape[1] if np.asarray(xs).ndim == 2 else 1
        return np.arange(n, dtype=float), float(n - 1), n - 1

    def ascend(self, acq, params, lb, ub, starts, maxeval=2000, ftol_rel=1e-10, xtol_abs=1e-10):
        self.calls.append(("ascend", acq, list(params), starts.shape, maxeval, ftol_rel, xtol_abs))
        return np.zeros(starts.shape[1]), starts, 1.5, 0, starts[:, 0].copy(), 1


LB, UB = np.zeros(2), np.ones(2)


def test_knowledge_gradient_plumbing():
    import bohip
    from bohip.acquisition import (ExpectedImprovement, KnowledgeGradient, acquire_max, acquisitionfunction, defaultoptions)
    from bohip.utils import latin_hypercube_sampling

    a = KnowledgeGradient()
    assert a.acq_id == "KG" and a.params() == [] and "extension" in KnowledgeGradient.__doc__
    assert bohip.KnowledgeGradient is KnowledgeGradient and "KG" not in bohip._lib.ACQ          # not a functor id of the kernels
    assert defaultoptions(StubModel, KnowledgeGradient) == dict(method="LD_LBFGS", restarts=1, maxeval=1024)
    assert defaultoptions(StubModel, ExpectedImprovement) == dict(method="LD_LBFGS", restarts=10, maxeval=2000)
    m = StubModel()
    f = acquisitionfunction(a, m)
    xs = np.asfortranarray(np.random.default_rng(0).random((2, 9)))
    vals = f(xs)
    assert vals.shape == (9,) and m.calls == [("kg", (2, 9), None)]
    with pytest.raises(ValueError, match="candidate set"):
        f(xs[:, 0])
    m = StubModel()
    for method in ("LD_LBFGS", "GN_DIRECT_L", "LN_COBYLA"):                                     # accepted, not used, no warning
        m.calls.clear()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            fmax, xmax = acquire_max(a, m, LB, UB, {"method": method, "restarts": 2, "maxeval": 12}, np.random.default_rng(7))
        assert m.calls == [("kg", (2, 12), None), ("kg", (2, 12), None)]
        rng = np.random.default_rng(7)
        best = (-math.inf, None)
        for _ in range(2):                                                                      # the first maximum over the restarts
            cand = latin_hypercube_sampling(LB, UB, 12, rng)
            r = StubModel().kg(cand)
            if r.best_val > best[0]:
                best = (r.best_val, cand[:, r.best_idx])
        assert fmax == best[0] and np.array_equal(xmax, best[1])
        assert np.all(xmax >= LB) and np.all(xmax <= UB)
    lacking = type("Bare", (), {"nobs": 3, "y": np.zeros(3)})()
    with pytest.raises(NotImplementedError, match="has no kg"):
        acquire_max(a, lacking, LB, UB, {"restarts": 1, "maxeval": 4})
    assert acquire_max(a, StubModel(n=0), LB, UB, {"restarts": 1})[0] == -math.inf              # an empty model: nothing to do


def test_existing_acquisitions_keep_their_routes():
    from bohip.acquisition import ExpectedImprovement, acquire_max, acquisitionfunction

    m = StubModel()
    acquire_max(ExpectedImprovement(), m, LB, UB, {"method": "LD_LBFGS", "restarts": 3, "maxeval": 50}, np.random.default_rng(1))
    assert m.calls == [("ascend", "EI", [2.0], (2, 3), 50, 1e-10, 1e-10)]
    m = StubModel()
    xs = np.zeros((2, 5))
    sc = acquisitionfunction(ExpectedImprovement(0.25), m)(xs)
    assert m.calls == [("score", "EI", [0.25], (2, 5))] and sc.shape == (5,)
    assert acquisitionfunction(ExpectedImprovement(0.25), m)(xs[:, 0]) == 0.0
