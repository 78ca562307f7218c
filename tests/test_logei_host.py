"""LogEI without a GPU: the NumPy twin of csrc/acq_log.h (tests/logei_reference.py) against the 80-digit table
(tests/golden/logei_table.npz), the shape of the function, the host mirror LogExpectedImprovement and its plumbing through
acquire_max / acquire_batch against stub models, and the ABI of include/bohip_acq.h in every table that binds it."""
import ctypes as C
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logei_reference as lr   # noqa: E402
from conftest import ROOT, load_golden   # noqa: E402

WANT = {"bohip_acq_eval"}
LB, UB = [0.0, 0.0], [1.0, 1.0]


@pytest.fixture(scope="module")
def table():
    return load_golden("logei_table")


@pytest.fixture(scope="module")
def twin(table):
    return dict(zip(("value", "dmu", "ds2"), lr.logei(table["mu"], table["s2"], table["tau"])))


# ---- the twin against the table --------------------------------------------------------------------------------------------------
def test_table_covers_the_grid_of_the_design(table):
    z, sigma = table["z"], table["sigma"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "logei_table.npz")) <= 200 * 1024
    for s in (1e-8, 1.0, 1e4):
        zs = z[sigma == s]
        assert np.sum((zs >= -6) & (zs <= 6)) >= 241
        for want in [np.nextafter(-4.0, -np.inf), -4.0, np.nextafter(-4.0, np.inf)] + [-(10.0 ** k) for k in range(1, 151)] \
                + [10.0 ** k for k in range(-3, 7)]:
            assert want in zs, (s, want)
    zero = table["s2"] == 0
    assert np.any(zero & (table["mu"] > table["tau"])) and np.any(zero & (table["mu"] < table["tau"])) \
        and np.any(zero & (table["mu"] == table["tau"]))
    assert np.array_equal(table["value"][zero & (table["mu"] <= table["tau"])], np.full(2, -np.inf))


def test_twin_matches_the_80_digit_table_within_twice_its_measured_worst_error(table, twin):
    """Measured on the full table (printed): value 2.376e-14, d/dmu 3.402e-14, d/ds2 3.212e-14, all at z in (-4, -3.5]; the
    continued-fraction branch 1.05e-15 / 2.4e-16 / 3.9e-16; z >= 7: 5.8e-16 / 1.3e-16 / 9.6e-15.  Bound: 2 x WORST."""
    for name in ("value", "dmu", "ds2"):
        worst = lr.assert_close(name, twin[name], table[name], 2.0, "twin")
        print(f"twin vs table, {name}: worst {worst:.3e} (WORST {lr.WORST[name]:.1e})")
        assert worst <= lr.WORST[name]                       # WORST is the measured figure rounded up, not a wish
    lo = table["z"] <= -4.0
    for name in ("value", "dmu", "ds2"):                     # the tail branch on its own: a few ulp
        fin = lo & np.isfinite(table[name])
        err = np.abs(twin[name][fin] - table[name][fin]) / np.maximum(np.abs(table[name][fin]), 1.0 if name == "value" else 1e-300)
        assert err.max() <= 2e-15, (name, err.max())


def test_finite_wherever_a_double_can_hold_the_result(table, twin):
    """Every finite z of the table gives a finite value and finite partials -- down to z = -1e150, where EI and its gradient have
    been exactly 0.0 since z ~ -38 -- except the four rows whose exact d/ds2 ~ z^2 / (2 s2) exceeds the largest double (the table
    holds +inf there, and so does the twin).  The partials are strictly positive for s2 > 0."""
    nz = table["s2"] > 0
    assert np.all(np.isfinite(table["z"][nz]))
    assert np.all(np.isfinite(twin["value"][nz])) and np.all(np.isfinite(twin["dmu"][nz]))
    over = ~np.isfinite(table["ds2"])
    assert over.sum() == 4 and np.all(table["z"][over] <= -1e147) and np.all(table["sigma"][over] == 1e-8)
    assert np.array_equal(np.isfinite(twin["ds2"]), ~over)
    assert np.all(twin["dmu"][nz] > 0) and np.all(twin["ds2"][nz & (table["z"] < 30)] > 0)
    far = nz & (table["z"] < -40)                            # where the linear-space EI is dead
    assert far.sum() >= 400 and np.all(twin["value"][far] < -700) and np.all(twin["dmu"][far] > 0)


def test_continuous_across_the_branch_switch(table, twin):
    for s in (1e-8, 1.0, 1e4):
        rows = [int(np.flatnonzero((table["sigma"] == s) & (table["z"] == z))[0])
                for z in (np.nextafter(-4.0, -np.inf), -4.0, np.nextafter(-4.0, np.inf))]
        assert table["z"][rows[1]] <= lr.LOGEI_SWITCH < table["z"][rows[2]]      # the two sides of `z > SWITCH`
        for name in ("value", "dmu", "ds2"):
            v = twin[name][rows]
            for a, b in ((0, 1), (1, 2)):
                assert abs(v[a] - v[b]) <= lr.tolerance(name, v[b], 2.0), (s, name, v)


def test_exp_of_the_twin_is_the_textbook_ei(table, twin):
    from scipy.special import erfc

    m = (table["s2"] > 0) & (table["z"] > -5)
    mu, s2, tau, z = table["mu"][m], table["s2"][m], table["tau"][m], table["z"][m]
    s = np.sqrt(s2)
    zz = (mu - tau) / s
    ei = (mu - tau) * (0.5 * erfc(-zz / math.sqrt(2))) + s * (np.exp(-0.5 * zz * zz) / math.sqrt(2 * math.pi))
    ok = np.isfinite(ei) & (np.abs(ei) >= np.finfo(np.float64).tiny)
    assert ok.sum() >= 690                                    # (702 rows have z > -5; a few underflow at sigma = 1e-8)
    got = np.exp(twin["value"][m][ok])
    assert np.all(np.abs(got - ei[ok]) <= 1e-12 * np.abs(ei[ok])), np.max(np.abs(got - ei[ok]) / np.abs(ei[ok]))


def test_value_rises_in_mu_and_in_s2_along_every_grid_line(table, twin):
    """The premise of the pruned arg-max's bound (k_prune_bound).  Exactly monotone mathematically; the computed values are so up
    to their evaluation error -- which only shows between the neighbouring doubles at the switch -- and the bound's slack
    2^-38 (1 + |f|) is ~100x that."""
    for s in (1e-8, 1.0, 1e4):                               # mu = z sigma rising at fixed sigma
        rows = np.flatnonzero(table["sigma"] == s)
        rows = rows[np.argsort(table["z"][rows], kind="stable")]
        v = twin["value"][rows]
        assert np.all(np.diff(v) >= -lr.tolerance("value", v[1:], 2.0))
        far = np.abs(np.diff(table["z"][rows])) > 1e-3       # apart by more than a rounding error: strictly
        assert np.all(np.diff(v)[far] > 0)
    sig = np.logspace(-8, 4, 241)
    for D in (-50.0, -5.0, -1.0, -1e-3, 0.0, 1e-3, 1.0, 5.0, 50.0):
        v, _, ds2 = lr.logei(D, sig * sig, 0.0)
        assert np.all(np.diff(v) >= -lr.tolerance("value", v[1:], 2.0)), D
        assert np.all(np.diff(v)[np.abs(D) / sig[1:] < 5] > 0), D      # (beyond |z| ~ 8 a step of the grid is below one ulp)
        v0 = lr.logei(D, 0.0, 0.0)[0]
        assert v0 <= v[0] + lr.tolerance("value", v[0], 2.0)            # s2 = 0 lies below every s2 > 0
    assert lr.SLACK_PRUNE > 50 * 2 * max(lr.WORST.values())


# ---- the host mirror --------------------------------------------------------------------------------------------------------------
def test_host_functor_is_the_twin(table, twin):
    import bohip

    assert bohip.LogExpectedImprovement().tau == -math.inf and bohip.LogExpectedImprovement.acq_id == "LogEI"
    assert "LogExpectedImprovement" in bohip.__all__
    assert (bohip.LogExpectedImprovement.SWITCH, bohip.LogExpectedImprovement.CF_DEPTH) == (lr.LOGEI_SWITCH, lr.LOGEI_CF_DEPTH)
    for tau in np.unique(table["tau"]):
        m = table["tau"] == tau
        a = bohip.LogExpectedImprovement(tau)
        assert a.params() == [tau]
        v = a(table["mu"][m], table["s2"][m])
        dmu, ds2 = a.partials(table["mu"][m], table["s2"][m])
        assert np.array_equal(v, twin["value"][m]) and np.array_equal(dmu, twin["dmu"][m]) and np.array_equal(ds2, twin["ds2"][m])
    a = bohip.LogExpectedImprovement(0.5)
    assert isinstance(a(1.5, 0.0), float) and a(1.5, 0.0) == 0.0 and a(0.5, 0.0) == -math.inf and a(0.0, 4.0) == lr.logei(0.0, 4.0, 0.5)[0]
    assert a.partials(1.0, 0.0) == (2.0, 0.0) and a.partials(0.0, 0.0) == (0.0, 0.0)
    # the ordering of the textbook EI, not of the reference's functor (D Phi + phi): at sigma > 1 they differ
    ei = bohip.ExpectedImprovement(0.5)
    assert ei(-2.0, 9.0) < 0 < math.exp(a(-2.0, 9.0))


class StubModel:
    """Records the calls; score / score_grad / ascend answer with whatever `fill` says."""

    def __init__(self, y=(1.0, 4.0, -2.0), fill=-math.inf, device=True):
        self.dim, self.y = 2, np.array(y, dtype=np.float64)
        self.x = np.asfortranarray(np.zeros((2, len(self.y))))
        self.nobs = len(self.y)
        self.fill, self.calls = fill, []
        if device:
            self.ascend = self._ascend

    def score(self, acq, params, xs, want_scores=True):
        xs = np.asarray(xs).reshape(self.dim, -1)
        self.calls.append(("score", acq, list(params), xs.shape))
        return np.full(xs.shape[1], self.fill), -math.inf, -1

    def score_grad(self, acq, params, xs):
        xs = np.asarray(xs).reshape(self.dim, -1)
        self.calls.append(("score_grad", acq, list(params), xs.shape))
        return np.full(xs.shape[1], self.fill), np.zeros(xs.shape, order="F")

    def _ascend(self, acq, p, lb, ub, starts, iters, ftol, xtol):
        self.calls.append(("ascend", acq, list(p), starts.shape))
        R = starts.shape[1]
        return np.full(R, self.fill), starts, -math.inf, -1, np.zeros(self.dim), 1      # the "nobody won" record: (-inf, -1)

    def select_batch(self, acq, params, xs, q, fantasy="believer", raise_tau=False):
        self.calls.append(("select_batch", acq, list(params), xs.shape, q, fantasy, raise_tau))
        return np.arange(q, dtype=np.int64), np.zeros(q), np.zeros(q), np.ones(q)


def test_setparams_follows_expected_improvement():
    """tau <- max(maxy, tau) (src/acquisitionfunctions.jl:44-46), the contract of test/warmstart.jl:64: tau == max y after a
    zero-iteration run on a pre-made model."""
    import bohip

    m = StubModel()
    a, e = bohip.LogExpectedImprovement(), bohip.ExpectedImprovement()
    assert bohip.setparams_(a, m) == bohip.setparams_(e, m) == 4.0 and a.tau == e.tau == 4.0
    m.y = np.array([1.0])
    bohip.setparams_(a, m)
    assert a.tau == 4.0                                       # never lowered
    a = bohip.LogExpectedImprovement()
    m = StubModel(fill=0.0)
    opt = bohip.BOpt(lambda x: 0.0, m, a, bohip.NoModelOptimizer(), LB, UB, maxiterations=0, initializer_iterations=0,
                     verbosity=bohip.Silent, rng=np.random.default_rng(0))
    bohip.boptimize_(opt)
    assert opt.acquisition is a and a.tau == 4.0 and len(m.y) == 3


def test_every_score_minus_inf_is_nobody_won():
    """A batch whose scores are all -inf gives the record (-inf, -1) on the device (tests/test_logei_gpu.py); the host then warns
    and returns (-inf, the lower bounds) -- what it does for an all-NaN batch -- on every route of acquire_max."""
    import bohip
    from bohip import acquisition as acq

    acq._WARNED_METHODS.add("LN_COBYLA")
    for opts, dev, called in (({"method": "LD_LBFGS", "restarts": 4}, True, "ascend"),
                              ({"method": "LD_LBFGS", "restarts": 4, "maxeval": 5}, False, "score_grad"),
                              ({"method": "LN_COBYLA", "restarts": 2, "maxeval": 8}, True, "score"),
                              ({"method": "GN_DIRECT_L", "restarts": 1, "maxeval": 9}, True, "score")):
        m = StubModel(device=dev)
        with pytest.warns(UserWarning, match="no finite value"):
            f, x = bohip.acquire_max(bohip.LogExpectedImprovement(), m, [0.25, 0.5], UB, opts, np.random.default_rng(0))
        assert f == -math.inf and np.array_equal(x, [0.25, 0.5])
        assert m.calls and all(c[0] == called and c[1] == "LogEI" and c[2] == [4.0] for c in m.calls), m.calls
    f = bohip.acquisitionfunction(bohip.LogExpectedImprovement(1.0), StubModel(fill=-3.0))
    assert f(np.zeros(2)) == -3.0 and np.array_equal(f(np.zeros((2, 5))), np.full(5, -3.0))


def test_batch_plumbing_takes_logei_and_qei_still_refuses_it():
    import bohip

    m = StubModel()
    a = bohip.LogExpectedImprovement()
    val, X = bohip.acquire_batch(a, m, LB, UB, 3, {"candidates": 16, "fantasy": "liar_max", "raise_tau": True}, np.random.default_rng(0))
    assert m.calls == [("select_batch", "LogEI", [4.0], (2, 16), 3, 4.0, True)] and X.shape == (2, 3)
    with pytest.raises(ValueError, match="ExpectedImprovement.*LogExpectedImprovement"):
        bohip.acquire_batch(a, m, LB, UB, 2, {"method": "qei"})
    with pytest.raises(ValueError, match="unknown batch option"):
        bohip.acquire_batch(a, m, LB, UB, 2, {"restarts": 3})
    with pytest.raises(ValueError, match="unknown acquisition option"):
        bohip.acquire_max(a, m, LB, UB, {"methd": "LD_LBFGS"})
    with pytest.raises(ValueError, match="pathwise"):
        bohip.acquire_max(a, m, LB, UB, {"pathwise": True})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.warns(UserWarning, match="NLopt setting"):
            bohip.acquire_max(a, m, LB, UB, {"population": 3})


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_acq_header_exports_ctypes_and_julia_agree():
    """include/bohip_acq.h <-> exports <-> _lib.ACQ_SIGNATURES <-> julia/BOHipAcq.jl: the same symbol, the same types argument by
    argument, in no other header's table; the id 6 in the header, in _lib.ACQ and in Julia; bohip.h keeps its 62 symbols."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_acq.h")).read()
    assert re.search(r"^#define BOHIP_ACQ_LOGEI 6$", raw, flags=re.M) and _lib.ACQ["LogEI"] == 6
    assert sorted(_lib.ACQ.values()) == list(range(7))
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "double*": "ptr(double)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.ACQ_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES):
        assert not WANT & set(other)
    main_raw = open(os.path.join(ROOT, "include", "bohip.h")).read()
    main = re.sub(r"/\*.*?\*/", "", main_raw, flags=re.S)
    main_syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & main_syms and len(main_syms) == 62 == len(_lib.SIGNATURES) and "LOGEI" not in main_raw
    assert "EXTENSION" in raw and "src/acquisitionfunctions.jl:4-9" in raw
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.POINTER(C.c_double): "ptr(double)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Ptr{Float64}": "ptr(double)"}
    src = open(os.path.join(ROOT, "julia", "BOHipAcq.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.ACQ_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert re.search(r"^const ACQ_LOGEI = Cint\(6\)", src, flags=re.M)
    assert f"const LOGEI_SWITCH = {lr.LOGEI_SWITCH}" in src and f"const LOGEI_CF_DEPTH = {lr.LOGEI_CF_DEPTH}" in src
    main_jl = open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert 'include("BOHipAcq.jl")' in main_jl and "LogExpectedImprovement" in main_jl
    assert "LogExpectedImprovement" in open(os.path.join(ROOT, "julia", "runtests.jl")).read()
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)
    csrc = open(os.path.join(ROOT, "bayesianoptimization.jl_amd", "csrc", "acq_log.h")).read()
    assert f"LOGEI_SWITCH = {lr.LOGEI_SWITCH}" in csrc and f"LOGEI_CF_DEPTH = {lr.LOGEI_CF_DEPTH}" in csrc
    assert "ACQ_LOGEI = 6" in open(os.path.join(ROOT, "bayesianoptimization.jl_amd", "csrc", "common.h")).read()


def test_acq_eval_rejects_bad_arguments_before_any_device_work():
    from bohip import _lib

    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    a = np.zeros(4)
    p = a.ctypes.data_as(dp)
    assert lib.bohip_acq_eval(7, p, 4, p, p, p, None, None) == _lib.E_ARG and b"unknown acq_id" in lib.bohip_last_error()
    assert lib.bohip_acq_eval(5, p, 4, p, p, p, None, None) == _lib.E_ARG            # a posterior draw is no functor of (mu, s2)
    assert lib.bohip_acq_eval(-1, p, 4, p, p, p, None, None) == _lib.E_ARG
    assert lib.bohip_acq_eval(6, None, 4, p, p, p, None, None) == _lib.E_ARG and b"acq_params" in lib.bohip_last_error()
    assert lib.bohip_acq_eval(6, p, -1, p, p, p, None, None) == _lib.E_ARG
    assert lib.bohip_acq_eval(6, p, 4, None, p, p, None, None) == _lib.E_ARG
    assert lib.bohip_acq_eval(6, p, 4, p, p, p, p, None) == _lib.E_ARG                 # dmu / dvar: together or not at all
    assert lib.bohip_acq_eval(4, None, 0, None, None, None, None, None) == _lib.OK     # n = 0: nothing to do
