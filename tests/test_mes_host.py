"""Max-value entropy search without a GPU: the ABI of include/bohip_mes.h in every table that binds it, the NumPy twin
(tests/mes_reference.py) against mpmath -- the functor over gamma in [-60, 38], the quantiles against roots bisected at 50 digits and
against the closed form of R = 1 -- one statistical look at the definition, and the plumbing of MaxValueEntropySearch through
acquisitionfunction / defaultoptions / acquire_max against a recording stub model."""
import ctypes as C
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mes_reference as mr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_mes", "bohip_mes_values", "bohip_mes_gumbel"}
EPS = np.finfo(np.float64).eps


def test_mes_header_exports_ctypes_and_julia_agree():
    """include/bohip_mes.h <-> exports <-> _lib.MES_SIGNATURES <-> julia/BOHipMES.jl: the same symbols, the same types argument by
    argument, none of them in the other headers' tables; bohip.h keeps its 62."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_mes.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "uint64_t": "uint64", "double": "double", "double*": "ptr(double)", "int*": "ptr(int)",
               "bohip_best*": "ptr(best)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.MES_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES, _lib.ACQ_SIGNATURES,
                  _lib.KG_SIGNATURES, _lib.ENS_SIGNATURES, _lib.ENS_GRAD_SIGNATURES):
        assert not WANT & set(other)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    main_syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & main_syms and len(main_syms) == 62 == len(_lib.SIGNATURES)
    assert "EXTENSION" in raw and "Wang & Jegelka" in raw
    defs = {k: int(v) for k, v in re.findall(r"#define\s+BOHIP_MES_(\w+)\s+(\d+)", raw)}
    assert defs == {"KMAX": 1024, "RMAX": 524288, "GUMBEL": 0, "JOINT": 1}
    assert (_lib.MES_KMAX, _lib.MES_RMAX, _lib.MES_GUMBEL, _lib.MES_JOINT) == (1024, 524288, 0, 1) == (mr.KMAX, mr.RMAX, 0, 1)
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_uint64: "uint64", C.c_double: "double", C.c_void_p: "ptr(void)",
          C.POINTER(C.c_double): "ptr(double)", C.POINTER(C.c_int): "ptr(int)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "UInt64": "uint64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)",
                "Ptr{Float64}": "ptr(double)", "Ptr{Cint}": "ptr(int)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipMES.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.MES_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipMES.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert int(re.search(r"const MES_KMAX = (\d+)", src).group(1)) == 1024
    assert int(re.search(r"const MES_RMAX = (\d+)", src).group(1)) == 524288
    for name in ("function mes(", "function mes_values(", "function mes_gumbel(", "struct MaxValueEntropySearch",
                 "function acquire_max_device(a::MaxValueEntropySearch"):
        assert name in src, name
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_null_handle_and_bad_sizes_are_reported_before_any_device_work():
    from bohip import _lib

    full = _lib.load()
    dp = C.POINTER(C.c_double)
    z = np.zeros(4)
    p = z.ctypes.data_as(dp)
    inf = math.inf
    gp_mes = lambda R, K, mode=0, floor=-inf: full.bohip_gp_mes(None, p, R, K, mode, 0, floor, 0.0, 0, p, None, None, None, None, None,   # noqa: E731
                                                                None, None)
    for call, word in [(lambda: gp_mes(0, 1), b"at least 1"), (lambda: gp_mes(2, 0), b"at least 1"), (lambda: gp_mes(2, 2, mode=7), b"unknown mode"),
                       (lambda: gp_mes(2, 2), b"null"),
                       (lambda: full.bohip_mes_values(None, p, p, 0, p, 1, p, None, None, None), b"at least 1"),
                       (lambda: full.bohip_mes_values(None, p, p, 2, p, 1, p, None, None, None), b"null"),
                       (lambda: full.bohip_mes_gumbel(None, p, p, 2, 0, 0, -inf, p, p), b"at least 1"),
                       (lambda: full.bohip_mes_gumbel(None, p, p, 2, 2, 0, -inf, p, p), b"null")]:
        assert call() == _lib.E_ARG
        assert word in full.bohip_last_error()


# ---- the twin against mpmath ----------------------------------------------------------------------------------------------------
GAMMAS = np.concatenate([np.linspace(-60.0, 38.0, 197), [4.0, -4.0, 0.0, 1e-9, -1e-9, math.nextafter(-4.0, 0.0), math.nextafter(-4.0, -8.0),
                                                         -3.999, -4.001, 12.0, 37.5]])


def test_functor_against_mpmath():
    """u within 1e-13 relative and du/dgamma within 1e-12 over gamma in [-60, 38] (absolute floor 1e-300 where they underflow), the
    two forms that meet at -4 included; the partials through the chain rule."""
    import mpmath as mp

    u, d, lam = mr.u_of_gamma(GAMMAS)
    worst_u = worst_d = 0.0
    for g, a, b in zip(GAMMAS, u, d):
        wu, wd = mr.mp_u(float(g)), mr.mp_dudg(float(g))
        worst_u = max(worst_u, float(abs(mp.mpf(float(a)) - wu) / (abs(wu) + mp.mpf(1e-287))))
        worst_d = max(worst_d, float(abs(mp.mpf(float(b)) - wd) / (abs(wd) + mp.mpf(1e-288))))
        assert a >= 0.0 and b <= 0.0
    print(f"twin against mpmath: worst relative error u {worst_u:.3e}, du/dgamma {worst_d:.3e}")
    assert worst_u <= 1e-13 and worst_d <= 1e-12
    assert mr.u_of_gamma(np.array([-4.0]))[0][0] == pytest.approx(1.9089, abs=1e-4)
    assert mr.u_of_gamma(np.array([math.nextafter(-4.0, 0.0)]))[0][0] == pytest.approx(mr.u_of_gamma(np.array([-4.0]))[0][0], rel=1e-13)
    # through (mu, s2, m): gamma = (m - mu) / sigma, du/dmu = -u' / sigma, du/ds2 = -u' gamma / (2 s2)
    mu, s2, m = 0.75, 0.25, np.array([-1.25, 0.75, 2.0, 20.75])
    uu, dmu, ds2 = mr.terms(mu, s2, m)
    for k, mk in enumerate(m):
        g = (mk - mu) / 0.5
        want = mr.mp_dudg(g)
        assert uu[k] == pytest.approx(float(mr.mp_u(g)), rel=1e-13, abs=1e-300)
        assert dmu[k] == pytest.approx(float(-want / 0.5), rel=1e-12, abs=1e-300)
        assert ds2[k] == pytest.approx(float(-want * g / (2 * s2)), rel=1e-12, abs=1e-300)
        h = 1e-6                                                           # ... and against differences of the twin's own values
        fd = (mr.terms(mu + h, s2, mk)[0] - mr.terms(mu - h, s2, mk)[0]) / (2 * h)
        assert dmu[k] == pytest.approx(float(fd), rel=1e-6, abs=1e-12)
        fd = (mr.terms(mu, s2 + h, mk)[0] - mr.terms(mu, s2 - h, mk)[0]) / (2 * h)
        assert ds2[k] == pytest.approx(float(fd), rel=1e-6, abs=1e-12)


def test_functor_edges_and_the_mean_over_max_values():
    nan, inf = math.nan, math.inf
    assert [float(v) for v in mr.terms(0.3, 0.0, 0.7)] == [0.0, 0.0, 0.0]
    for mu, s2, m in [(nan, 1.0, 0.0), (0.0, nan, 0.0), (0.0, 1.0, nan), (inf, 1.0, 0.0), (0.0, inf, 0.0), (0.0, 1.0, inf), (0.0, 1.0, -inf),
                      (0.0, -1.0, 0.0)]:
        assert all(math.isnan(float(v)) for v in mr.terms(mu, s2, m)), (mu, s2, m)
    mu, var, mv = np.array([0.0, 0.5, 1.0]), np.array([1.0, 0.25, 0.0]), np.array([1.5, 0.75, 2.0])
    val, dmu, dvar = mr.values(mu, var, mv)
    for j in range(3):
        u = [float(mr.terms(mu[j], var[j], m)[0]) for m in mv]
        assert val[j] == ((0.0 + u[0]) + u[1] + u[2]) / 3.0                # ascending k from +0.0, one division
    assert val[2] == 0.0 and mr.record(val) == (float(val.max()), int(np.argmax(val)))
    assert mr.record([nan, nan]) == (-inf, -1) and mr.record([nan, -inf, 2.0, 2.0]) == (2.0, 2) and mr.record([-inf]) == (-inf, -1)
    assert np.isnan(mr.values(mu, var, [1.0, inf])[0]).all()
    # MES is not a monotone function of EI's ingredients: at a fixed gap it rises with sigma
    assert mr.values([0.0, 0.0], [0.25, 1.0], [1.0])[0][1] > mr.values([0.0, 0.0], [0.25, 1.0], [1.0])[0][0]


# ---- the quantiles ------------------------------------------------------------------------------------------------------------
def test_log_cdf_and_the_bracket():
    import mpmath as mp

    g = np.array([-60.0, -12.5, -4.0, math.nextafter(-4.0, 0.0), -1.0, 0.0, 1e-9, 3.0, 9.0, 20.0, 38.0])
    got = mr.logcdf(g)
    with mp.workdps(60):
        for x, v in zip(g, got):
            want = mr.mp_logcdf(mp.mpf(float(x)))
            assert abs(mp.mpf(float(v)) - want) <= 1e-13 * abs(want) + mp.mpf(1e-300), x
    rng = np.random.default_rng(8)
    for R in (1, 2, 17, 300, 4096):                                        # the bracket needs no expansion
        mu, var = rng.standard_normal(R) * 3.0, rng.uniform(1e-4, 4.0, R)
        lo, hi = mr.bracket(mu, var)
        assert mr.S(lo, mu, var) < mr.LOGP[0] and mr.S(hi, mu, var) > mr.LOGP[2]
    assert mr.S(hi, mu, var) > -mr.RMAX * 2.87e-7 > -0.151 and -0.151 > mr.LOGP[2]
    assert mr.bracket([1.0, 3.0, math.nan], [0.0, 0.0, 1.0]) == (3.0, 3.0)
    assert mr.S(2.9, [1.0, 3.0], [0.0, 0.0]) == -math.inf and mr.S(3.0, [1.0, 3.0], [0.0, 0.0]) == 0.0


@pytest.mark.parametrize("R", [1, 2, 7, 64])
def test_quantiles_against_roots_bisected_at_50_digits(R):
    rng = np.random.default_rng(100 + R)
    for scale, offset in ((1.0, 0.0), (1e-3, 1e3)):
        mu, var = offset + scale * rng.standard_normal(R), scale * scale * rng.uniform(0.01, 2.0, R)
        q, (lo, hi) = mr.quantiles(mu, var)
        roots = np.array([float(mr.mp_root(mu, var, p, lo, hi)) for p in mr.P])
        bound = mr.quantile_bounds(mu, var, roots)
        share = np.abs(q - roots) / bound
        print(f"R = {R}, scale {scale}: |y_p - root_p| / bound = {share}")
        assert np.all(share <= 1.0)
        if R == 1:                                                          # the closed form y_p = mu + sigma Phi^-1(p)
            want = mu[0] + math.sqrt(var[0]) * np.array([-0.6744897501960817, 0.0, 0.6744897501960817])
            assert np.all(np.abs(q - want) <= bound + 4 * EPS * np.abs(want))


def test_max_values_and_the_degenerate_cases():
    from bohip import _lib

    lib = _lib.load()
    u = mr.uniforms(9, 40)
    assert np.all((u > 0.0) & (u <= 1.0))
    for k in (0, 1, 39):                                                    # the first uniform of bohip_thompson_normal(seed, k, 0): the
        z = lib.bohip_thompson_normal(9, k, 0)                              # normal's radius gives it back
        assert abs(z) <= math.sqrt(-2.0 * math.log(u[k])) * (1 + 4 * EPS)
    mu, var = np.array([0.0, 0.4, -0.3]), np.array([1.0, 0.5, 2.0])
    q, mv = mr.maxvals(mu, var, 8, 3)
    b = (q[2] - q[0]) / mr.GUMBEL_DEN
    assert mr.GUMBEL_DEN == pytest.approx(math.log(math.log(4)) - math.log(math.log(4 / 3)), rel=2 * EPS)
    assert mr.LOGLOG2 == pytest.approx(math.log(math.log(2)), rel=2 * EPS)
    np.testing.assert_array_equal(mv, (q[1] + b * mr.LOGLOG2) - b * np.log(-np.log(mr.uniforms(3, 8))))
    assert np.array_equal(mr.maxvals(mu, var, 8, 3, floor=1.0)[1], np.maximum(mv, 1.0))
    q0, m0 = mr.maxvals([1.0, 3.0, 2.0], [0.0, 0.0, 0.0], 4, 1)              # every sigma is 0
    assert q0.tolist() == [3.0] * 3 and m0.tolist() == [3.0] * 4
    assert mr.maxvals([1.0, 3.0], [0.0, 0.0], 2, 1, floor=5.0)[1].tolist() == [5.0, 5.0]
    # the Gumbel law of the fit, F(y) = exp(-exp(-(y - a) / b)), has the median and the inter-quartile range it was fitted to
    a = q[1] + b * mr.LOGLOG2
    inv = lambda p: a - b * math.log(-math.log(p))   # noqa: E731
    assert inv(0.5) == pytest.approx(q[1], rel=1e-14) and inv(0.75) - inv(0.25) == pytest.approx(q[2] - q[0], rel=1e-13)


def test_median_of_the_maximum_statistically():
    """The definition itself: y50 of 64 independent candidates against the empirical median of 20000 draws of their maximum.  The
    standard error of a sample median is 1 / (2 f(y50) sqrt(n)), f the density of the maximum: S'(y50) exp(S(y50)) = S'(y50) / 2."""
    rng = np.random.default_rng(2024)
    mu, var = rng.standard_normal(64), rng.uniform(0.05, 1.5, 64)
    q, _ = mr.quantiles(mu, var)
    draws = (mu[None, :] + np.sqrt(var)[None, :] * rng.standard_normal((20000, 64))).max(axis=1)
    se = 1.0 / (2.0 * (mr.S_prime(q[1], mu, var) * 0.5) * math.sqrt(draws.size))
    print(f"y50 = {q[1]:.5f}, empirical median {np.median(draws):.5f}, standard error {se:.5f}")
    assert abs(np.median(draws) - q[1]) <= 4.0 * se
    for p, y in zip(mr.P, q):                                               # and the other two, as shares
        assert abs(np.mean(draws <= y) - p) <= 4.0 * math.sqrt(p * (1 - p) / draws.size)


# ---- the plumbing against a stub model ------------------------------------------------------------------------------------------
class StubModel:
    """Records its calls.  mes answers with the twin on a posterior made from the candidates themselves."""

    def __init__(self, d=2, n=3):
        self.dim = d
        self.x = np.zeros((d, n), order="F")
        self.y = np.arange(n, dtype=float)
        self.calls = []

    @property
    def nobs(self):
        return self.y.size

    def mes(self, xs, samples=16, mode="gumbel", seed=0, floor=None, jitter_rel=1e-12, max_tries=40):
        from bohip.model import MESResult

        self.calls.append(("mes", xs.shape, samples, mode, seed))
        mu, var = np.sin(3 * xs[0]), 0.1 + np.cos(2 * xs[1]) ** 2
        q, mv = mr.maxvals(mu, var, samples, seed % 1000)
        vals = mr.values(mu, var, mv)[0]
        bv, bi = mr.record(vals)
        return MESResult(vals, mv, q, mu, var, bv, bi)

    def score(self, acq, params, xs, want_scores=True):
        self.calls.append(("score", acq, list(params), np.asarray(xs).shape))
        n = np.asarray(xs).shape[1] if np.asarray(xs).ndim == 2 else 1
        return np.arange(n, dtype=float), float(n - 1), n - 1

    def ascend(self, acq, params, lb, ub, starts, maxeval=2000, ftol_rel=1e-10, xtol_abs=1e-10):
        self.calls.append(("ascend", acq, list(params), starts.shape, maxeval, ftol_rel, xtol_abs))
        return np.zeros(starts.shape[1]), starts, 1.5, 0, starts[:, 0].copy(), 1


LB, UB = np.zeros(2), np.ones(2)


def test_max_value_entropy_search_argument_errors():
    from bohip.acquisition import MaxValueEntropySearch

    a = MaxValueEntropySearch()
    assert (a.samples, a.mode, a.acq_id, a.params()) == (16, "gumbel", "MES", []) and "extension" in MaxValueEntropySearch.__doc__
    assert (MaxValueEntropySearch(1024, "joint").samples, MaxValueEntropySearch(1024, "joint").mode) == (1024, "joint")
    for bad in (0, -3, 1025, 2.5, "16", True, None):
        with pytest.raises(ValueError, match="samples must be"):
            MaxValueEntropySearch(bad)
    for bad in ("exact", "", None, 0):
        with pytest.raises(ValueError, match="mode must be"):
            MaxValueEntropySearch(16, bad)


def test_max_value_entropy_search_plumbing():
    import bohip
    from bohip.acquisition import (ExpectedImprovement, KnowledgeGradient, MaxValueEntropySearch, acquire_max, acquisitionfunction,
                                   defaultoptions)
    from bohip.utils import latin_hypercube_sampling

    a = MaxValueEntropySearch(4)
    assert bohip.MaxValueEntropySearch is MaxValueEntropySearch and "MES" not in bohip._lib.ACQ   # not a functor id of the kernels
    assert "MaxValueEntropySearch" in bohip.__all__
    assert defaultoptions(StubModel, MaxValueEntropySearch) == dict(method="LD_LBFGS", restarts=1, maxeval=1024)
    assert defaultoptions(StubModel, KnowledgeGradient) == dict(method="LD_LBFGS", restarts=1, maxeval=1024)
    assert defaultoptions(StubModel, ExpectedImprovement) == dict(method="LD_LBFGS", restarts=10, maxeval=2000)
    m = StubModel()
    f = acquisitionfunction(a, m, rng=np.random.default_rng(3))
    xs = np.asfortranarray(np.random.default_rng(0).random((2, 9)))
    vals = f(xs)
    seed = int(np.random.default_rng(3).integers(0, 2**63))
    assert vals.shape == (9,) and m.calls == [("mes", (2, 9), 4, "gumbel", seed)]
    with pytest.raises(ValueError, match="candidate set"):
        f(xs[:, 0])
    for method in ("LD_LBFGS", "GN_DIRECT_L", "LN_COBYLA"):                                     # accepted, not used, no warning
        m = StubModel()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            fmax, xmax = acquire_max(a, m, LB, UB, {"method": method, "restarts": 2, "maxeval": 12}, np.random.default_rng(7))
        rng = np.random.default_rng(7)
        best, want_calls = (-math.inf, None), []
        for _ in range(2):                                                                      # the first maximum over the restarts;
            cand = latin_hypercube_sampling(LB, UB, 12, rng)                                    # the seed follows the candidates
            seed = int(rng.integers(0, 2**63))
            want_calls.append(("mes", (2, 12), 4, "gumbel", seed))
            r = StubModel().mes(cand, samples=4, seed=seed)
            if r.best_val > best[0]:
                best = (r.best_val, cand[:, r.best_idx])
        assert m.calls == want_calls
        assert fmax == best[0] and np.array_equal(xmax, best[1])
        assert np.all(xmax >= LB) and np.all(xmax <= UB)
    m = StubModel()
    acquire_max(MaxValueEntropySearch(2, "joint"), m, LB, UB, {"restarts": 1, "maxeval": 5}, np.random.default_rng(1))
    assert m.calls[0][:4] == ("mes", (2, 5), 2, "joint")
    lacking = type("Bare", (), {"nobs": 3, "y": np.zeros(3)})()
    with pytest.raises(NotImplementedError, match="has no mes"):
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
