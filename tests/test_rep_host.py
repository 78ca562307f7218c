"""Replicated sites without a GPU (include/bohip_rep.h): the NumPy twin of the collapsed model (tests/rep_reference.py)
against the model with every evaluation as its own row, collapse_evaluations, the ABI in every table that binds it, the refusals of
the host layer and the routing of the fit.

Bounds.  The device is held to the suite's existing bounds against the expanded reference (rep_reference.mu_bound, var_tol,
grad_bound, MLL_RTOL).  The twin claims to be that model EXACTLY, so here it has to sit at most 1e-3 of each of those bounds away
from the expanded reference, and the float64 twin as close to the np.longdouble one (the twin's own rounding is then no part of what
the device tests measure).  The other way round, the twin with every 1 / r_i forced to 1 -- the sites stored, the weights forgotten --
has to MISS mu, mll and the logNoise gradient by at least 100 times the device's bound on every input, or the device tests could not
tell the two apart."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rep_reference as rr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_append_sites", "bohip_gp_sites_info", "bohip_gp_get_reps"}
INPUTS = [(kern, n, h) for kern in rr.KERNS for n in (40, 130) for h in rr.HYPERS]
R = 200


def models(kern, n, h, orc, **kw):
    lnoise, lsig = h
    pos, reps, evals, Xs = rr.raw(n, lnoise, lsig)
    _, ybar, r, ss, _ = rr.sites_of(pos, evals)
    assert np.count_nonzero(r == 1) >= n / 4 and r.min() == 1 and r.max() == 5
    X, y = rr.expand(pos, evals)
    ex = rr.Expanded(kern, X, y, rr.LL[kern], lsig, lnoise, rr.BETA, orc)
    tw = rr.RepTwin(kern, pos, ybar, r, ss, rr.LL[kern], lsig, lnoise, rr.BETA, **kw)
    return ex, tw, Xs[:R]


def shares(ex, tw, Xs):
    """How far the twin lies from the expanded reference, in units of the device's bounds: (mu, var, mll, gradient[P])."""
    mu_o, var_o = ex.predict(Xs)
    mu, var = tw.predict(Xs)
    m_o, g_o = ex.mll_grad()
    m, dn, dm, dk = tw.mll_grad()
    g = np.concatenate([[dn, dm], dk]).astype(np.float64)
    return (float(np.max(np.abs(mu - mu_o) / rr.mu_bound(mu_o, ex.alpha, ex.s2f))),
            float(np.max(np.abs(var - var_o) / rr.var_tol(var_o, ex.N, ex.s2f))),
            float(abs(m - m_o) / (rr.MLL_RTOL * abs(m_o))), np.abs(g - g_o) / rr.grad_bound(g_o))


# ---- the twin ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,n,h", INPUTS)
def test_collapsed_twin_is_the_expanded_model(orc, kern, n, h):
    ex, tw, Xs = models(kern, n, h, orc)
    s_mu, s_var, s_mll, s_g = shares(ex, tw, Xs)
    print(f"{kern} n={n} N={ex.N} {h}: cond {np.linalg.cond(tw.cK):.1e}, shares of the device's bounds: mu {s_mu:.1e} var {s_var:.1e} "
          f"mll {s_mll:.1e} grad {s_g.max():.1e}")
    assert max(s_mu, s_var, s_mll, float(s_g.max())) <= 1e-3


@pytest.mark.parametrize("kern,n,h", INPUTS)
def test_float64_twin_against_longdouble(orc, kern, n, h):
    ex, tw, Xs = models(kern, n, h, orc)
    _, tq, _ = models(kern, n, h, orc, dtype=np.longdouble)
    assert tq.L.dtype == np.longdouble and tq.alpha.dtype == np.longdouble
    mu, var = tw.predict(Xs)
    muq, varq = tq.predict(Xs)
    m, dn, dm, dk = tw.mll_grad()
    mq, dnq, dmq, dkq = tq.mll_grad()
    gq = np.concatenate([[dnq, dmq], dkq]).astype(np.float64)
    g = np.concatenate([[dn, dm], dk])
    s2f = ex.s2f
    assert np.all(np.abs(mu - muq) <= 1e-3 * rr.mu_bound(muq.astype(float), ex.alpha, s2f))
    assert np.all(np.abs(var - varq) <= 1e-3 * rr.var_tol(varq.astype(float), ex.N, s2f))
    assert abs(m - mq) <= 1e-3 * rr.MLL_RTOL * abs(mq)
    assert np.all(np.abs(g - gq) <= 1e-3 * rr.grad_bound(gq))
    # L and alpha, of which the float64 twin is the device's only reference: at most a tenth of test_seeded_vs_oracle's bounds (rtol
    # 1e-9 / atol 1e-11 s_f and rtol 1e-6 / atol 1e-9 max|alpha|), so that the device keeps nine tenths of its bound.  The trailing rows
    # of ANY float64 factor carry the condition number -- cond x eps ~ 5e6 x 1e-16 of their size at (0, 5), measured 2.8e-2 of the
    # bound at 130 sites -- so a smaller share cannot be asked of a float64 reference there
    share_L = float(np.max(np.abs(tw.L - tq.L) / (1e-9 * np.abs(tq.L) + 1e-11 * math.sqrt(s2f))))
    share_a = float(np.max(np.abs(tw.alpha - tq.alpha) / (1e-6 * np.abs(tq.alpha) + 1e-9 * np.abs(tq.alpha).max())))
    print(f"{kern} n={n} {h}: float64 twin against longdouble, shares of the device's bounds: L {share_L:.1e} alpha {share_a:.1e}")
    assert share_L <= 1e-1 and share_a <= 1e-1


@pytest.mark.parametrize("kern,n,h", INPUTS)
def test_ignoring_the_weights_misses_by_a_hundred_bounds(orc, kern, n, h):
    ex, bad, Xs = models(kern, n, h, orc, ignore_weights=True)
    s_mu, _, s_mll, s_g = shares(ex, bad, Xs)
    print(f"{kern} n={n} {h}: weights ignored: mu {s_mu:.1e} mll {s_mll:.1e} logNoise gradient {s_g[0]:.1e} bounds away")
    assert min(s_mu, s_mll, float(s_g[0])) >= 100.0


def test_all_ones_is_the_plain_model(orc):
    """r_i = 1 everywhere: C = 0 and the twin is matern_reference's model."""
    from matern_reference import MaternGP

    pos, _, evals, Xs = rr.raw(40, -2.0, 0.0)
    y = np.array([v[0] for v in evals])
    tw = rr.RepTwin("Mat32Iso", pos, y, np.ones(40, dtype=np.int64), np.zeros(40), rr.LL["Mat32Iso"], 0.0, -2.0, rr.BETA)
    gp = MaternGP("Mat32Iso", pos, y, rr.LL["Mat32Iso"], 0.0, -2.0, rr.BETA)
    assert tw.site_constant() == (0.0, 0.0)
    assert float(tw.mll()) == pytest.approx(gp.mll(), rel=1e-13)
    np.testing.assert_allclose(tw.alpha, gp.alpha, rtol=1e-9, atol=1e-12 * np.abs(gp.alpha).max())


# ---- collapse_evaluations ----------------------------------------------------------------------------------------------------------------
def test_collapse_evaluations_groups_in_order_of_first_occurrence():
    from bohip import collapse_evaluations

    a, b, c = np.array([0.1, 0.2]), np.array([0.3, 0.4]), np.array([0.5, 0.6])
    x = np.stack([a, b, a, c, b, a], axis=1)                                 # a repeated non-adjacently, three times
    y = np.array([1.0, 10.0, 2.0, 7.0, 14.0, 6.0])
    xs, ybar, reps, ss, ymax = collapse_evaluations(x, y)
    np.testing.assert_array_equal(xs, np.stack([a, b, c], axis=1))
    assert xs.flags.f_contiguous and reps.dtype == np.int64
    np.testing.assert_array_equal(reps, [3, 2, 1])
    np.testing.assert_array_equal(ybar, [3.0, 12.0, 7.0])
    np.testing.assert_array_equal(ss, [14.0, 8.0, 0.0])
    np.testing.assert_array_equal(ymax, [6.0, 14.0, 7.0])
    # byte-identical means byte-identical: -0.0 and 0.0 are two positions, a nearby value another
    xs2, _, reps2, _, _ = collapse_evaluations(np.array([[0.0, -0.0, 1.0, np.nextafter(1.0, 2.0)]]), np.zeros(4))
    assert xs2.shape == (1, 4) and np.all(reps2 == 1)
    with pytest.raises(ValueError):
        collapse_evaluations(x, y[:-1])
    e = collapse_evaluations(np.zeros((2, 0)), np.zeros(0))
    assert e[0].shape == (2, 0) and all(v.size == 0 for v in e[1:])


def test_within_site_sum_of_squares_is_two_pass():
    """Five evaluations of 1e8 + small noise: the one-pass form sum y^2 - r ybar^2 loses every digit, the second pass none."""
    from bohip import collapse_evaluations

    rng = np.random.default_rng(3)
    dev = 1e-3 * rng.standard_normal(5)
    y = 1e8 + dev
    _, ybar, reps, ss, _ = collapse_evaluations(np.zeros((3, 5)), y)
    exact = np.sum((y.astype(np.longdouble) - np.mean(y.astype(np.longdouble))) ** 2)
    assert reps[0] == 5 and float(ss[0]) == pytest.approx(float(exact), rel=1e-6)
    one_pass = float(np.sum(y * y) - 5 * ybar[0] ** 2)
    assert abs(one_pass - float(exact)) > 1e3 * float(exact)                 # (what the test would not notice otherwise)
    xs, ybar1, _, ss1, ymax1 = collapse_evaluations(np.arange(6.0).reshape(3, 2), np.array([3.0, 4.0]))
    assert np.all(ss1 == 0.0) and np.array_equal(ybar1, [3.0, 4.0]) and np.array_equal(ymax1, [3.0, 4.0])   # r = 1: the value itself, s = 0 exactly


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_rep_header_exports_ctypes_and_julia_agree():
    """include/bohip_rep.h <-> exports <-> _lib.REP_SIGNATURES <-> julia/BOHipRep.jl: the same three symbols, the same types argument by
    argument, none of them in the model's header or table."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_rep.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double*": "ptr(double)", "int64_t*": "ptr(int64)", "int*": "ptr(int)", "bohip_gp*": "ptr(void)", "int64_t": "int64"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.REP_SIGNATURES)
    assert not WANT & set(_lib.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & declared and len(declared) == len(_lib.SIGNATURES) == 62
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)", C.POINTER(C.c_int64): "ptr(int64)",
          C.POINTER(C.c_int): "ptr(int)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)", "Ptr{Int64}": "ptr(int64)",
                "Ptr{Cint}": "ptr(int)"}
    src = open(os.path.join(ROOT, "julia", "BOHipRep.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.REP_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipRep.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert "BOHipRep.jl" in open(os.path.join(ROOT, "julia", "runtests.jl")).read()
    assert re.search(r"^function append_sites!\(", src, flags=re.M) and re.search(r"^function collapse_evaluations\(", src, flags=re.M)
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    code = re.sub(r"\[[^\[\]]*\bfor\b[^\[\]]*\]", "[]", code)
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_argument_errors_need_no_device():
    from bohip import _lib

    full = _lib.load()
    one = np.ones(1)
    r = np.ones(1, dtype=np.int64)
    p, ip = one.ctypes.data_as(C.POINTER(C.c_double)), r.ctypes.data_as(C.POINTER(C.c_int64))
    assert full.bohip_gp_append_sites(None, p, p, ip, p, 1) == _lib.E_ARG
    assert full.bohip_gp_sites_info(None, None, None, None, None, None) == _lib.E_ARG
    assert full.bohip_gp_get_reps(None, ip) == _lib.E_ARG


# ---- the host layer through a fake library -------------------------------------------------------------------------------------------------
class FakeLib:
    """Stores nothing and succeeds: enough of libbohip for ElasticGPE's bookkeeping.  It records the calls."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("bohip_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(name)
            return 0
        return call


@pytest.fixture
def fake(monkeypatch):
    from bohip import _lib

    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    return lib


def site_model(bohip, **kw):
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd([0.0, 0.0], 0.0), collapse=True, **kw)
    x = np.array([[0.1, 0.1, 0.7], [0.2, 0.2, 0.9]])
    bohip.update_(m, x, np.array([1.0, 3.0, 1.5]))
    return m


def test_update_collapses_and_the_fields_speak_of_sites(fake):
    import bohip

    m = site_model(bohip)
    assert fake.calls.count("bohip_gp_append_sites") == 1 and "bohip_gp_append" not in fake.calls
    assert (m.nobs, m.nevals, m.weighted) == (2, 3, True) and bohip.dims(m) == (2, 2)
    np.testing.assert_array_equal(m.x, [[0.1, 0.7], [0.2, 0.9]])
    np.testing.assert_array_equal(m.y, [2.0, 1.5])
    np.testing.assert_array_equal(m.reps, [2, 1])
    assert bohip.maxy(m) == 3.0                                             # the largest raw evaluation, not the largest mean (2.0)
    m.append_(np.array([[0.3], [0.3]]), [2.5])                              # a plain row on a weighted model: r = 1
    assert (m.nobs, m.nevals) == (3, 4) and m.reps[-1] == 1 and bohip.maxy(m) == 3.0
    plain = bohip.ElasticGPE(2, kernel=bohip.SEArd([0.0, 0.0], 0.0))
    bohip.update_(plain, np.array([[0.1, 0.1], [0.2, 0.2]]), np.array([1.0, 3.0]))
    assert fake.calls[-1] == "bohip_gp_append" and (plain.nobs, plain.nevals, plain.weighted) == (2, 2, False) and bohip.maxy(plain) == 3.0
    g = bohip.ElasticGPE.from_data(np.array([[0.1, 0.1, 0.5]]), np.array([1.0, 2.0, 0.0]), collapse=True)
    assert (g.nobs, g.nevals) == (2, 3) and fake.calls[-1] == "bohip_gp_append_sites"
    with pytest.raises(ValueError, match="number of sites"):
        m.append_sites_(np.zeros((2, 2)), [1.0, 2.0], [1], [0.0, 0.0])


def test_refusals_name_the_limitation(fake):
    import bohip
    from bohip.bopt import _map_fit, _marginal_fit

    m = site_model(bohip)
    with pytest.raises(ValueError, match="replicated sites"):
        m.draw_paths(1, 64, 0)
    with pytest.raises(ValueError, match="replicated sites"):
        bohip.acquire_max(bohip.ThompsonSamplingSimple(), m, [0.0, 0.0], [1.0, 1.0], {"pathwise": True, "restarts": 2, "maxeval": 10},
                          np.random.default_rng(0))
    Theta = np.zeros((2, 5))
    for call in (m.score_ensemble, m.score_ensemble_grad):
        with pytest.raises(ValueError, match="replicated sites"):
            call("EI", [0.0], np.zeros((2, 3)), Theta)
    with pytest.raises(ValueError, match=r'objective="loo".*replicated sites'):
        _map_fit(m, bohip.MAPGPOptimizer(objective="loo", noisebounds=[-4, 3], kernbounds=[[-3] * 3, [3] * 3]).options)
    with pytest.raises(ValueError, match="MarginalGPOptimizer.*replicated sites"):
        _marginal_fit(m, bohip.MarginalGPOptimizer(samples=2, noisebounds=[-4, 3], meanbounds=[[-1], [1]], kernbounds=[[-3] * 3, [3] * 3]).options)
    ok = bohip.ElasticGPE(2, kernel=bohip.SEArd([0.0, 0.0], 0.0))
    for make in (lambda: bohip.ConstrainedGPE(m, [ok], [0.0], [1]), lambda: bohip.ConstrainedGPE(ok, [m], [0.0], [1]),
                 lambda: bohip.MultiObjectiveGPE((ok, m)),
                 lambda: bohip.ConstrainedGPE(ok, [bohip.ElasticGPE(2, collapse=True)], [0.0], [1])):      # (collapse=True, nothing appended yet)
        with pytest.raises(ValueError, match="replicated sites"):
            make()
    bohip.ConstrainedGPE(ok, [ok], [0.0], [1])
    with pytest.raises(ValueError, match="MultiGPE does not support replicated sites"):
        bohip.MultiGPE(2, collapse=True)
    mg = bohip.MultiGPE(2)
    with pytest.raises(ValueError, match="MultiGPE does not support replicated sites"):
        mg.append_sites_(np.zeros((2, 1)), [0.0], [2], [0.0])
    # an unweighted model is refused nothing
    ok.append_(np.array([[0.1], [0.2]]), [1.0])
    ok.draw_paths(1, 64, 0)
    assert "bohip_gp_paths_draw" in fake.calls


class FakeFitModel:
    """Counts which objective call the fit makes; weighted says which model it is."""

    def __init__(self, weighted):
        from bohip.model import MeanConst, SEArd

        self.kernel, self.mean, self.logNoise, self.nobs, self.weighted = SEArd([0.1, 0.2], 0.3), MeanConst(0.5), -1.0, 9, weighted
        self.loop, self.batched = 0, 0

    def set_params_(self, **kw):
        pass

    def mll_batch_dims(self):
        return 5, 512

    def mll_grad(self):
        self.loop += 1
        return 1.0, 10.0, 20.0, np.array([30.0, 31.0, 40.0])

    def mll(self):
        self.loop += 1
        return 1.0

    def mll_grad_batch(self, Theta, want_grad=True):
        self.batched += 1
        return np.ones(len(Theta)), np.zeros(Theta.shape), np.zeros(len(Theta), dtype=np.int64)

    loo_grad_batch = mll_grad_batch


@pytest.mark.parametrize("want_grad", [True, False])
def test_fit_objective_takes_the_loop_for_a_weighted_model(want_grad):
    from bohip.bopt import _fit_objective

    opt = dict(domean=True, noise=True, kern=True)
    X = np.zeros((5, 8))                                                    # 9 observations, 8 columns: an unweighted model takes the batched call
    for weighted, want in ((False, (0, 1)), (True, (8, 0))):
        m = FakeFitModel(weighted)
        f, G = _fit_objective(m, opt, 3, lambda x: None, 5, 8, want_grad=want_grad)(X)
        assert (m.loop, m.batched) == want and f.shape == (8,) and (G is not None) == want_grad
