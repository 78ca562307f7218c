"""Leave-one-out cross-validation without a GPU (include/bohip_loo.h): the NumPy twin (tests/loo_reference.py) against
N delete-one refits and against central differences, the ABI in every table that binds it, and the fit's objective switch.

Bounds.  Fast formula against brute force: both are float64 solves with the same cK, condition <= 3e3 at the BASELINE setting used
here, so they differ by ~ eps x condition ~ 1e-12 relative; 1e-10 of the largest magnitude is asked.  Gradient against central
differences with h = 1e-5: the differences' own error is h^2 f''' / 6 + eps |f| / h ~ 1e-9 relative, 1e-6 is asked (the project's
gradient tolerance, test_mll_gradient_vs_oracle)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_reference as lr   # noqa: E402
from conftest import ROOT, synth   # noqa: E402
from matern_reference import KERNELS   # noqa: E402
from oracle.oracle import NOISE_EPS   # noqa: E402

WANT = {"bohip_gp_loo", "bohip_gp_loo_grad"}
BASE = dict(loglen=math.log(0.5), logsig=0.0, lognoise=-2.0)


def hyper(kern, d, beta):
    nl = 1 if KERNELS[kern][1] else d
    return dict(loglen=np.full(nl, BASE["loglen"]), logsig=BASE["logsig"], lognoise=BASE["lognoise"], beta=beta)


# ---- the twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.3], ids=["MeanZero", "MeanConst"])
@pytest.mark.parametrize("kern", list(KERNELS))
@pytest.mark.parametrize("N", [1, 2, 5, 17])
def test_fast_formula_is_the_brute_force(kern, N, beta):
    X, y, _ = synth(N, 3, 1, seed=40 + N)
    h = hyper(kern, 3, beta)
    fast, brute = lr.loo_fast(kern, X, y, **h), lr.loo_brute(kern, X, y, **h)
    for a, b, what in zip(fast[:3], brute[:3], ("mu", "var", "logp")):
        scale = max(np.abs(b).max(), np.abs(y).max()) if what == "mu" else np.abs(b).max()   # (mu = y - alpha / kappa: rounds at the size of y)
        assert np.abs(a - b).max() <= 1e-10 * scale, what
    assert abs(fast[3] - brute[3]) <= 1e-10 * abs(brute[3])
    if N == 1:                                                    # one observation alone: the prior
        assert fast[0][0] == pytest.approx(beta, abs=1e-15)
        assert fast[1][0] == pytest.approx(math.exp(2 * h["logsig"]) + math.exp(2 * h["lognoise"]) + NOISE_EPS, rel=1e-14)


@pytest.mark.parametrize("kern", list(KERNELS))
@pytest.mark.parametrize("N,d", [(2, 2), (17, 3), (65, 5)])
def test_twin_gradient_is_the_derivative_of_the_twin_value(kern, N, d):
    X, y, _ = synth(N, d, 1, seed=7 + N)
    nl = 1 if KERNELS[kern][1] else d
    t = np.concatenate([[-1.6, 0.2], np.full(nl, -0.6) + 0.1 * np.arange(nl), [0.25]])
    tot, g = lr.grad_vec(kern, X, y, t)
    assert tot == pytest.approx(lr.total_at(kern, X, y, t), rel=1e-13)
    fd = lr.central_differences(kern, X, y, t)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-7 * np.abs(fd).max())


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_loo_header_exports_ctypes_and_julia_agree():
    """include/bohip_loo.h <-> exports <-> _lib.LOO_SIGNATURES <-> julia/BOHipLOO.jl: the same two symbols, the same types argument
    by argument, none of them in the model's header or table (tests/test_fit_host.py does this for the batched fit)."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_loo.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double*": "ptr(double)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.LOO_SIGNATURES)
    assert not WANT & set(_lib.SIGNATURES) and not WANT & set(_lib.FIT_SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & declared and len(declared) == len(_lib.SIGNATURES) == 62
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)"}
    jl_types = {"Cint": "int", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)"}
    src = open(os.path.join(ROOT, "julia", "BOHipLOO.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.LOO_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipLOO.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert re.search(r"^function loo\(", src, flags=re.M) and re.search(r"^function loo_grad\(", src, flags=re.M)
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_null_arguments_are_argument_errors():
    from bohip import _lib

    full = _lib.load()
    out = np.zeros(4)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    assert full.bohip_gp_loo(None, None, None, None, p) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()
    assert full.bohip_gp_loo_grad(None, p, p, p, p) == _lib.E_ARG


# ---- the fit's objective ------------------------------------------------------------------------------------------------------
def test_an_unknown_objective_raises():
    from bohip.bopt import MAPGPOptimizer

    with pytest.raises(ValueError, match="bogus"):
        MAPGPOptimizer(objective="bogus")
    assert MAPGPOptimizer().options["objective"] == "mll"
    assert MAPGPOptimizer(objective="loo", restarts=3).options["objective"] == "loo"


class FakeModel:
    """Answers loo_grad with slots that name themselves; any other objective call is a failure of the test."""

    def __init__(self, mean_const):
        from bohip.model import MeanConst, MeanZero, SEArd

        self.kernel, self.mean, self.logNoise, self.nobs = SEArd([0.1, 0.2], 0.3), MeanConst(0.5) if mean_const else MeanZero(), -1.0, 9
        self.seen = []

    def set_params_(self, ll=None, lsigma=None, logNoise=None, beta=None):
        self.now = dict(ll=None if ll is None else np.array(ll), lsigma=lsigma, logNoise=logNoise, beta=beta)

    def loo_grad(self):
        self.seen.append(self.now)
        return 100.0 + len(self.seen), 10.0, 20.0, np.array([30.0, 31.0, 40.0])

    def mll_batch_dims(self):
        return 5, 512

    def mll_grad(self):
        raise AssertionError("the marginal likelihood was asked for")

    mll = mll_grad_batch = mll_grad


@pytest.mark.parametrize("mean_const", [True, False])
def test_fit_objective_loo_takes_the_loop_and_maps_the_slots(mean_const):
    from bohip.bopt import _fit_objective

    m = FakeModel(mean_const)
    opt = dict(domean=True, noise=False, kern=True, objective="loo")
    p = 4 if mean_const else 3

    def apply(x):
        kw = {}
        if mean_const:
            kw["beta"] = x[0]
        kw["ll"], kw["lsigma"] = x[p - 3:p - 1], x[p - 1]
        m.set_params_(**kw)

    fg = _fit_objective(m, opt, 3, apply, p, 8)                   # (9 observations, 8 columns: the batched marginal likelihood would run)
    X = np.arange(p * 8, dtype=float).reshape(p, 8)
    f, G = fg(X)
    assert len(m.seen) == 8
    np.testing.assert_array_equal(f, 101.0 + np.arange(8))
    want = [20.0, 30.0, 31.0, 40.0] if mean_const else [30.0, 31.0, 40.0]   # idx = [1?, 2, 3, 4] of [noise, mean, ll0, ll1, lsigma]
    np.testing.assert_array_equal(G, np.tile(np.array(want)[:, None], (1, 8)))
    for r, s in enumerate(m.seen):
        np.testing.assert_array_equal(s["ll"], X[p - 3:p - 1, r])
        assert s["lsigma"] == X[p - 1, r] and s["logNoise"] is None and (s["beta"] == X[0, r] if mean_const else s["beta"] is None)
