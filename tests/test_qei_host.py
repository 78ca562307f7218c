"""Greedy Monte-Carlo q-EI without a GPU: the ABI of include/bohip_qei.h in every table that binds it, the properties of the NumPy
twin of the selection (tests/qei_reference.py), and the option plumbing of acquire_batch's "qei" method against a recording fake
model."""
import ctypes as C
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qei_reference as qr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_qei_batch", "bohip_gp_qei_select"}


def test_qei_header_exports_ctypes_and_julia_agree():
    """include/bohip_qei.h <-> exports <-> _lib.QEI_SIGNATURES <-> julia/BOHipQEI.jl: the same symbols, the same types argument by
    argument, none of them in the other headers' tables (tests/test_fit_host.py does this for the batched likelihood)."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_qei.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "uint64_t": "uint64", "double": "double", "double*": "ptr(double)",
               "int64_t*": "ptr(int64)", "int*": "ptr(int)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.QEI_SIGNATURES)
    assert not WANT & set(_lib.SIGNATURES) and not WANT & set(_lib.PATHS_SIGNATURES) and not WANT & set(_lib.FIT_SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    main_syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & main_syms and len(main_syms) == 62 == len(_lib.SIGNATURES)
    assert "src/models/gp.jl:7" in raw and "EXTENSION" in raw
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_uint64: "uint64", C.c_double: "double", C.c_void_p: "ptr(void)",
          C.POINTER(C.c_double): "ptr(double)", C.POINTER(C.c_int64): "ptr(int64)", C.POINTER(C.c_int): "ptr(int)"}
    jl_types = {"Cint": "int", "Int64": "int64", "UInt64": "uint64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)",
                "Ptr{Float64}": "ptr(double)", "Ptr{Int64}": "ptr(int64)", "Ptr{Cint}": "ptr(int)"}
    src = open(os.path.join(ROOT, "julia", "BOHipQEI.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.QEI_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipQEI.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_null_handle_and_limits_are_reported_before_any_device_work():
    from bohip import _lib

    full = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    F, gain, idx = np.zeros(4), np.zeros(2), np.zeros(2, dtype=np.int64)
    assert full.bohip_gp_qei_select(None, F.ctypes.data_as(dp), 2, 2, 0.0, 1, idx.ctypes.data_as(ip), gain.ctypes.data_as(dp)) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()
    assert full.bohip_gp_qei_batch(None, F.ctypes.data_as(dp), 2, 2, 0, 1e-12, 40, 0.0, 1, idx.ctypes.data_as(ip),
                                   gain.ctypes.data_as(dp), None, None, None) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()


# ---- the twin ------------------------------------------------------------------------------------------------------------------
def test_twin_properties_on_random_matrices():
    rng = np.random.default_rng(11)
    for S, R, q in [(1, 1, 1), (7, 5, 5), (33, 12, 6), (100, 40, 8), (64, 9, 9)]:
        F = rng.standard_normal((S, R))
        tau = 0.3
        idx, gain = qr.qei_greedy(F, tau, q)
        live = idx >= 0
        assert np.all(np.diff(gain) <= 0) and np.all(gain[live] > 0) and np.all(gain[~live] == 0)        # gains never increase
        assert len(set(idx[live].tolist())) == int(live.sum())                                           # picks are distinct
        assert np.all(np.diff(live.astype(int)) <= 0)                                                    # -1 only as a tail
        for k in range(1, q + 1):                                                                        # prefix property in q
            ik, gk = qr.qei_greedy(F, tau, k)
            np.testing.assert_array_equal(ik, idx[:k])
            np.testing.assert_array_equal(gk, gain[:k])
        col = np.maximum(F - tau, 0.0).mean(axis=0)                                                      # q = 1: the column means
        i1, g1 = qr.qei_greedy(F, tau, 1)
        if col.max() > 0:
            assert i1[0] == int(np.argmax(col)) and g1[0] == pytest.approx(col.max(), rel=1e-13)
        else:
            assert i1[0] == -1
        assert gain.sum() == pytest.approx(qr.qei_value(F, tau, idx[live]), rel=1e-12, abs=1e-300)       # the gains telescope


@pytest.mark.parametrize("R,q", [(6, 2), (7, 3)])
def test_twin_greedy_is_within_the_submodular_bound_of_the_best_subset(R, q):
    rng = np.random.default_rng(100 + R)
    worst = 1.0
    for _ in range(20):
        F = rng.standard_normal((40, R)) * rng.uniform(0.2, 2.0, R) + rng.uniform(-1.0, 0.5, R)
        idx, gain = qr.qei_greedy(F, 0.0, q)
        best, _ = qr.best_subset(F, 0.0, q)
        assert gain.sum() >= (1.0 - 1.0 / math.e) * best
        assert gain.sum() <= best * (1 + 1e-12)
        worst = min(worst, gain.sum() / best) if best > 0 else worst
    print(f"R = {R}, q = {q}: worst greedy / best over 20 matrices {worst:.4f} (bound {1 - 1 / math.e:.4f})")


def test_twin_edges():
    F = np.array([[0.5, -1.0, 0.25], [0.0, 0.5, -3.0]])
    idx, gain = qr.qei_greedy(F, 0.5, 3)                                # every entry <= tau
    assert idx.tolist() == [-1, -1, -1] and gain.tolist() == [0.0, 0.0, 0.0]
    rng = np.random.default_rng(3)
    G = rng.standard_normal((50, 4))
    D = G[:, [0, 1, 1, 2, 0, 3]]                                        # columns 2 and 4 duplicate 1 and 0
    idx, gain = qr.qei_greedy(D, 0.0, 6)
    picked = set(idx[idx >= 0].tolist())
    assert not {1, 2} <= picked and not {0, 4} <= picked and 2 not in picked and 4 not in picked
    assert idx.tolist()[4:] == [-1, -1] and len(picked) == 4            # the four distinct columns, then nothing has a gain left
    T = np.array([[1.0, 2.0, 2.0], [1.0, 0.0, 0.0]])                    # gains 1, 1, 1 -> index 0; then 1 and 2 tie at 0.5 -> 1
    idx, gain = qr.qei_greedy(T, 0.0, 3)
    assert idx.tolist() == [0, 1, -1] and gain.tolist() == [1.0, 0.5, 0.0]
    N = np.array([[np.nan, 1.0, -np.inf], [np.nan, -np.inf, np.inf]])
    idx, gain = qr.qei_greedy(N, 0.0, 3)
    assert idx.tolist() == [2, 1, -1] and gain[0] == np.inf and gain[1] == 0.5 and not np.isnan(gain).any()
    mu, var = np.array([0.3, -0.2]), np.array([0.25, 1.0])
    ei = qr.textbook_ei(mu, var, 0.1)
    z = (mu - 0.1) / np.sqrt(var)
    Phi = np.array([0.5 * math.erfc(-t / math.sqrt(2)) for t in z])
    np.testing.assert_allclose(ei, (mu - 0.1) * Phi + np.sqrt(var) * np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi), rtol=1e-14)


# ---- the option plumbing of acquire_batch against a fake model -------------------------------------------------------------------
class FakeModel:
    """Records the calls.  qei_batch / qei_select answer with the twin on a fixed matrix whose last candidate never wins."""

    def __init__(self, d=2, n=3, dead=False):
        self.dim = d
        self.x = np.zeros((d, n), order="F")
        self.y = np.arange(n, dtype=float)
        self.calls = []
        self.dead = dead

    @property
    def nobs(self):
        return self.y.size

    def _F(self, S, R):
        F = np.random.default_rng(5).standard_normal((S, R)) + self.y.max()
        if self.dead:
            F[:, 1:] = -10.0                                            # only candidate 0 can ever win
        return F

    def select_batch(self, acq, params, xs, q, fantasy="believer", raise_tau=False):
        self.calls.append(("select_batch", acq, list(params), xs.shape, q, fantasy, raise_tau))
        return np.arange(q, dtype=np.int64), np.ones(q), np.zeros(q), np.ones(q)

    def qei_batch(self, xs, q, S=256, seed=0, tau=None, jitter=1e-12, max_tries=40, want_samples=False):
        from bohip.model import QEIBatch

        self.calls.append(("qei_batch", xs.shape, q, S, seed, tau))
        idx, gain = qr.qei_greedy(self._F(S, xs.shape[1]), tau, q)
        return QEIBatch(idx, gain, 0.0, 0, None)

    def draw_paths(self, S=1, M=2048, seed=0):
        model = self
        model.calls.append(("draw_paths", S, M, seed))

        class Paths:
            def __enter__(self):
                return self

            def __exit__(self, *exc):
                model.calls.append(("paths_closed",))
                return False

            def eval(self, xs, want_values=True):
                model.calls.append(("paths_eval", xs.shape))
                F = model._F(S, xs.shape[1])
                return F, F.max(axis=1), F.argmax(axis=1)

        return Paths()

    def qei_select(self, samples, tau, q):
        self.calls.append(("qei_select", np.asarray(samples).shape, tau, q))
        return qr.qei_greedy(samples, tau, q)


LB, UB = np.zeros(2), np.ones(2)


def test_acquire_batch_rejects_what_qei_cannot_mean():
    from bohip.acquisition import ExpectedImprovement, UpperConfidenceBound, acquire_batch

    m = FakeModel()
    with pytest.raises(ValueError, match="batch method must be one of"):
        acquire_batch(ExpectedImprovement(), m, LB, UB, 2, {"method": "joint"})
    with pytest.raises(ValueError, match="ExpectedImprovement.*UpperConfidenceBound"):
        acquire_batch(UpperConfidenceBound(), m, LB, UB, 2, {"method": "qei"})
    for extra in ({"fantasy": "believer"}, {"raise_tau": True}):
        with pytest.raises(ValueError, match="belong to method 'fantasy'"):
            acquire_batch(ExpectedImprovement(), m, LB, UB, 2, {"method": "qei", **extra})
    with pytest.raises(ValueError, match="needs 'pathwise'"):
        acquire_batch(ExpectedImprovement(), m, LB, UB, 2, {"method": "qei", "features": 64})
    with pytest.raises(ValueError, match="draws"):
        acquire_batch(ExpectedImprovement(), m, LB, UB, 2, {"method": "qei", "draws": 0})
    for k in ("draws", "pathwise", "features"):
        with pytest.raises(ValueError, match="needs 'method': 'qei'"):
            acquire_batch(ExpectedImprovement(), m, LB, UB, 2, {k: 1})
    assert not m.calls


def test_default_path_still_calls_select_batch_with_the_old_arguments():
    from bohip.acquisition import ExpectedImprovement, acquire_batch

    for opts in ({"candidates": 16}, {"candidates": 16, "method": "fantasy"}):
        m = FakeModel()
        val, X = acquire_batch(ExpectedImprovement(), m, LB, UB, 3, {**opts, "fantasy": "liar_max", "raise_tau": True},
                               np.random.default_rng(0))
        assert m.calls == [("select_batch", "EI", [2.0], (2, 16), 3, 2.0, True)]
        assert val.tolist() == [1.0, 1.0, 1.0] and X.shape == (2, 3)
    m = FakeModel()
    acquire_batch(ExpectedImprovement(), m, LB, UB, 2, {"candidates": 8}, np.random.default_rng(0))
    assert m.calls == [("select_batch", "EI", [2.0], (2, 8), 2, "believer", False)]


def test_qei_route_and_pathwise_route():
    from bohip.acquisition import ExpectedImprovement, acquire_batch

    xs = np.asfortranarray(np.random.default_rng(2).random((2, 12)))
    seed = int(np.random.default_rng(9).integers(0, 2 ** 63 - 1))
    m = FakeModel()
    val, X = acquire_batch(ExpectedImprovement(), m, LB, UB, 3, {"method": "qei", "xs": xs}, np.random.default_rng(9))
    assert m.calls == [("qei_batch", (2, 12), 3, 256, seed, 2.0)]                                        # tau = max y after setparams_
    idx, gain = qr.qei_greedy(m._F(256, 12), 2.0, 3)
    np.testing.assert_array_equal(X, xs[:, idx])
    np.testing.assert_array_equal(val, gain)
    m = FakeModel()
    a = ExpectedImprovement(0.5)
    val, X = acquire_batch(a, m, LB, UB, 2, {"method": "qei", "xs": xs, "draws": 32}, np.random.default_rng(9), setparams=False)
    assert m.calls == [("qei_batch", (2, 12), 2, 32, seed, 0.5)]                                         # setparams=False: tau as given
    m = FakeModel()
    val, X = acquire_batch(ExpectedImprovement(), m, LB, UB, 3, {"method": "qei", "xs": xs, "pathwise": True, "draws": 20},
                           np.random.default_rng(9))
    assert m.calls == [("draw_paths", 20, 2048, seed), ("paths_eval", (2, 12)), ("paths_closed",), ("qei_select", (20, 12), 2.0, 3)]
    idx, gain = qr.qei_greedy(m._F(20, 12), 2.0, 3)
    np.testing.assert_array_equal(X, xs[:, idx])
    np.testing.assert_array_equal(val, gain)
    m = FakeModel()
    acquire_batch(ExpectedImprovement(), m, LB, UB, 1, {"method": "qei", "candidates": 7, "pathwise": True, "features": 64},
                  np.random.default_rng(9))
    assert m.calls[0][:3] == ("draw_paths", 256, 64) and m.calls[1] == ("paths_eval", (2, 7))


def test_dropped_picks_warn():
    from bohip.acquisition import ExpectedImprovement, acquire_batch

    m = FakeModel(dead=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        val, X = acquire_batch(ExpectedImprovement(), m, LB, UB, 3, {"method": "qei", "candidates": 9, "draws": 16},
                               np.random.default_rng(1))
    assert any("only 1 of 3 picks" in str(x.message) for x in w)
    assert val.shape == (1,) and X.shape == (2, 1) and val[0] > 0
    lacking = type("Bare", (), {"nobs": 3, "y": np.zeros(3)})()
    with pytest.raises(NotImplementedError, match="has no qei_batch"):
        acquire_batch(ExpectedImprovement(), lacking, LB, UB, 2, {"method": "qei"})
