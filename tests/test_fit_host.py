"""The batched marginal likelihood and the multi-start MAP fit without a GPU: the ABI of include/bohip_fit.h in every table that
binds it, and the search of bopt._multistart_map on the NumPy twin's objective (tests/fit_reference.py)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_reference as fr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_mll_batch_dims", "bohip_gp_mll_grad_batch"}


def test_fit_header_exports_ctypes_and_julia_agree():
    """include/bohip_fit.h <-> exports <-> _lib.FIT_SIGNATURES <-> julia/BOHipFit.jl: the same symbols, the same types argument by
    argument, none of them in the model's header or tables (tests/test_path_host.py does this for the paths)."""
    from bohip import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip_fit.h")).read(), flags=re.S)
    hdr = re.sub(r"#.*", "", hdr)
    c_types = {"int": "int", "int64_t": "int64", "double*": "ptr(double)", "int64_t*": "ptr(int64)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.FIT_SIGNATURES)
    assert not WANT & set(_lib.SIGNATURES) and not WANT & set(_lib.PATHS_SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    assert not WANT & set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert "src/models/gp.jl:54-77" in open(os.path.join(ROOT, "include", "bohip_fit.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int64): "ptr(int64)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)", "Ptr{Int64}": "ptr(int64)"}
    src = open(os.path.join(ROOT, "julia", "BOHipFit.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.FIT_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipFit.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert int(re.search(r"#define BOHIP_FIT_NMAX (\d+)", open(os.path.join(ROOT, "include", "bohip_fit.h")).read()).group(1)) == _lib.FIT_NMAX
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_null_handle_is_an_argument_error():
    from bohip import _lib

    full = _lib.load()
    P, nmax = C.c_int64(), C.c_int64()
    assert full.bohip_gp_mll_batch_dims(None, C.byref(P), C.byref(nmax)) == _lib.E_ARG
    th, out = np.zeros(4), np.zeros(1)
    dp = C.POINTER(C.c_double)
    assert full.bohip_gp_mll_grad_batch(None, 1, th.ctypes.data_as(dp), out.ctypes.data_as(dp), None, None) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()


# ---- the search, on the twin ---------------------------------------------------------------------------------------------------
def test_multistart_leaves_the_poor_basin():
    """From the current parameters alone the fit ends in the "all noise" basin (-14.1664); with 8 starts it finds the other one
    (-10.5456), and is no worse than SciPy's L-BFGS-B run from each of the same starts."""
    from bohip.bopt import _multistart_map

    best, x, per = _multistart_map(fr.twin_fg_batch, fr.X0, fr.LO, fr.HI, fr.RESTARTS, 500, np.random.default_rng(fr.SEED), 3.0)
    ref = fr.scipy_best()
    print("batched ascent per start:", np.array2string(per, precision=4), " SciPy per start:", np.array2string(ref, precision=4))
    assert per.shape == (fr.RESTARTS,)
    assert per[0] < -13
    assert best > -11
    assert best >= ref.max() - 1e-6 * abs(ref.max())
    assert best == per.max() and np.all(x >= fr.LO) and np.all(x <= fr.HI)
    assert fr.twin_mll_grad(x)[0] == pytest.approx(best, rel=1e-12)


def test_infinite_bounds_start_around_the_current_parameters():
    from bohip.bopt import _multistart_map

    seen = []

    def fg(X):
        seen.append(X.copy())
        return -np.sum((X - 0.5) ** 2, axis=0), -2.0 * (X - 0.5)

    x0 = np.array([1.0, -2.0, 0.25])
    lo, hi = np.array([-math.inf, -3.0, -math.inf]), np.array([math.inf, math.inf, 0.5])
    best, x, per = _multistart_map(fg, x0, lo, hi, 16, 60, np.random.default_rng(0), 2.0)
    S = seen[0]
    np.testing.assert_array_equal(S[:, 0], x0)
    assert np.all(S[0] >= 1.0 - 2.0) and np.all(S[0] <= 1.0 + 2.0)            # both sides open: x0 -/+ startwidth
    assert np.all(S[1] >= -3.0) and np.all(S[1] <= -2.0 + 2.0)                # upper side open
    assert np.all(S[2] >= 0.25 - 2.0) and np.all(S[2] <= 0.5)                 # lower side open
    assert S[0, 1:].min() < 0.0 and S[0, 1:].max() > 2.0                      # ... and the strata fill that range
    assert best == pytest.approx(0.0, abs=1e-12) and np.allclose(x, 0.5, atol=1e-6)
    assert all(np.isfinite(s).all() for s in seen)


class StubModel:
    """Records what the fit does to a model; its marginal likelihood is the twin's on the multimodal problem."""

    def __init__(self, mean_const=True):
        from bohip.model import MeanConst, MeanZero, SEIso

        self.kernel = SEIso(fr.X0[2], fr.X0[3])
        self.mean = MeanConst(fr.X0[1]) if mean_const else MeanZero()
        self.logNoise = float(fr.X0[0])
        self.nobs = 12
        self.calls, self.thetas = [], []

    def set_params_(self, ll=None, lsigma=None, logNoise=None, beta=None):
        from bohip.model import MeanConst

        if ll is not None:
            self.kernel.ll = np.atleast_1d(np.asarray(ll, float)).copy()
        if lsigma is not None:
            self.kernel.lsigma = float(lsigma)
        if logNoise is not None:
            self.logNoise = float(logNoise)
        if beta is not None:
            self.mean = MeanConst(beta)

    def theta(self):
        return np.concatenate([[self.logNoise, self.mean.beta], self.kernel.ll, [self.kernel.lsigma]])

    def mll_grad(self):
        m, g = fr.twin_mll_grad(self.theta())
        return m, g[0], g[1], g[2:]

    def mll_batch_dims(self):
        return 4, 512

    def mll_grad_batch(self, Theta, want_grad=True):
        self.thetas.append(np.array(Theta))
        out = [fr.twin_mll_grad(t) for t in Theta]
        mll = np.array([o[0] for o in out])
        return mll, np.stack([o[1] for o in out]), np.where(np.isfinite(mll), 0, 1)

    def fit_(self):
        self.calls.append(("fit_", self.theta()))


def test_single_start_calls_scipy_as_before(monkeypatch):
    import scipy.optimize

    from bohip.bopt import MAPGPOptimizer, optimizemodel_

    got = {}
    real = scipy.optimize.minimize

    def spy(fun, x0, **kw):
        got.update(x0=np.array(x0), kw=kw)
        return real(fun, x0, **kw)

    monkeypatch.setattr(scipy.optimize, "minimize", spy)
    o = MAPGPOptimizer(every=1, noisebounds=[-4, 2], meanbounds=[[-2], [2]], kernbounds=[[-4, -3], [3, 3]], maxeval=37)
    assert o.options["restarts"] == 1 and o.options["startwidth"] == 3.0 and o.options["seed"] is None
    m = StubModel()
    optimizemodel_(o, m)
    np.testing.assert_array_equal(got["x0"], fr.X0)
    assert got["kw"]["method"] == "L-BFGS-B" and got["kw"]["jac"] is True and got["kw"]["options"] == dict(maxfun=37)
    assert got["kw"]["bounds"] == list(zip(fr.LO.tolist(), fr.HI.tolist()))
    assert not m.thetas and len(m.calls) == 1                      # the batched call is never used, one refit at the end


def test_multistart_through_the_optimizer_and_fixed_parameters():
    from bohip.bopt import MAPGPOptimizer, optimizemodel_

    m = StubModel()
    optimizemodel_(MAPGPOptimizer(every=1, restarts=8, seed=fr.SEED, noisebounds=[-4, 2], meanbounds=[[-2], [2]],
                                  kernbounds=[[-4, -3], [3, 3]]), m)
    assert m.thetas and all(t.shape == (8, 4) for t in m.thetas)
    np.testing.assert_array_equal(m.thetas[0], fr.starts().T)
    assert len(m.calls) == 1 and fr.twin_mll_grad(m.calls[0][1])[0] > -11
    # kern = False: the kernel's entries of every row stay what the model holds, and only the free ones move
    m = StubModel()
    optimizemodel_(MAPGPOptimizer(every=1, restarts=4, seed=1, kern=False, noisebounds=[-4, 2], meanbounds=[[-2], [2]], maxeval=30), m)
    T = np.concatenate(m.thetas)
    assert np.all(T[:, 2] == fr.X0[2]) and np.all(T[:, 3] == fr.X0[3])
    assert np.ptp(T[:, 0]) > 0 and np.ptp(T[:, 1]) > 0
    np.testing.assert_array_equal(m.calls[0][1][2:], fr.X0[2:])
    # a MeanZero model: the mean entry is the constant 0 and is not optimised
    m = StubModel(mean_const=False)
    optimizemodel_(MAPGPOptimizer(every=1, restarts=3, seed=2, noisebounds=[-4, 2], kernbounds=[[-4, -3], [3, 3]], maxeval=20), m)
    assert np.all(np.concatenate(m.thetas)[:, 1] == 0.0)


def test_dispatch_rule_follows_the_table():
    from bohip import bopt

    assert not bopt._fit_batched(513, 64, 512)
    for size, hmin in bopt._FIT_BATCH_MIN_H:
        assert bopt._fit_batched(size, hmin, 512) and (hmin == 1 or not bopt._fit_batched(size, hmin - 1, 512))
    assert [s for s, _ in bopt._FIT_BATCH_MIN_H] == sorted(s for s, _ in bopt._FIT_BATCH_MIN_H) and bopt._FIT_BATCH_MIN_H[-1][0] == 512
