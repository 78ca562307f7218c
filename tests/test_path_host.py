"""Posterior sample paths without a GPU: the frequency law of the NumPy twin (tests/path_reference.py) against every kernel family,
the twin's generator against the library's host export, and the option plumbing of acquire_max / acquire_thompson_batch against a
stub model that records calls."""
import math
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_reference as mr   # noqa: E402
import path_reference as pr   # noqa: E402


@pytest.fixture(scope="module")
def bo():
    import bohip

    return bohip


def test_twin_generator_is_the_library_generator(bo):
    """Negative streams (the basis) included: the twin's vectorised splitmix64 + Box-Muller against bohip_thompson_normal."""
    from bohip import _lib

    lib = _lib.load()
    j = np.arange(64)
    for s in (-4097, -2, -1, 0, 1, 63):
        lib_z = np.array([lib.bohip_thompson_normal(9, s, int(k)) for k in j])
        assert np.all(np.abs(pr.normal(9, s, j) - lib_z) <= 4 * pr.EPS * np.maximum(np.abs(lib_z), 1.0))
    # the basis streams and the path streams do not meet
    assert not np.intersect1d(pr.normal(3, -1, j), pr.normal(3, 0, j)).size


# max |Phi Phi' - k| / s2f over 200 uniform points in d = 4, ARD length scales 0.3, 0.5, 1, 2, s2f = 1.7, frequencies from the
# LIBRARY'S generator (keys of include/bohip_paths.h), seeds 1..5, measured on the CPU:
#   family      F = 1024                              F = 4096
#   SE          0.0460 0.0367 0.0554 0.0495 0.0781    0.0266 0.0189 0.0252 0.0334 0.0332
#   Matérn 5/2  0.0577 0.0652 0.0590 0.0546 0.0679    0.0269 0.0223 0.0296 0.0301 0.0350
#   Matérn 3/2  0.0594 0.0646 0.0720 0.0715 0.0616    0.0360 0.0270 0.0357 0.0339 0.0406
#   Matérn 1/2  0.0680 0.0666 0.0752 0.0721 0.0718    0.0318 0.0307 0.0379 0.0421 0.0436
# (1 / sqrt(F) = 0.031 and 0.016: the maximum over 20 000 pairs sits two to three standard deviations out.)
# The limits are twice the worst value of each column.
LAW_LIMIT = {1024: 2 * 0.0781, 4096: 2 * 0.0436}


@pytest.mark.parametrize("kern", ["SEArd", "Mat52Ard", "Mat32Ard", "Mat12Ard"])
def test_frequency_law_reproduces_the_kernel(kern):
    rng = np.random.default_rng(11)
    d, s2f = 4, 1.7
    ll, ls = np.log(np.array([0.3, 0.5, 1.0, 2.0])), 0.5 * math.log(s2f)
    X = rng.uniform(0, 1, (200, d))
    K = mr.cov(kern, X, X, ll, ls)
    for F, seeds in ((1024, (1, 2, 3, 4, 5, 6, 7)), (4096, (1, 2, 3, 4, 5))):      # seeds 6, 7 were not among the measured ones
        for seed in seeds:
            Ph = pr.features(pr.frequencies(kern, ll, d, F, seed), X, s2f)
            # paired features: the prior variance is s2f exactly at every point
            np.testing.assert_allclose(np.sum(Ph * Ph, axis=1), s2f, rtol=1e-13)
            err = np.abs(Ph @ Ph.T - K).max() / s2f
            print(f"{kern} F={F} seed={seed}: max |PhiPhi' - k| / s2f = {err:.4f} (limit {LAW_LIMIT[F]:.4f})")
            assert err <= LAW_LIMIT[F]


def test_iso_kernel_differs_only_in_the_length_scales():
    a = pr.frequencies("SEIso", np.array([0.3]), 3, 16, 5)
    b = pr.frequencies("SEArd", np.full(3, 0.3), 3, 16, 5)
    np.testing.assert_array_equal(a, b)


def test_twin_interpolates_and_has_the_conditional_moments():
    """f_s(X_i) + eps_si + n u_si = y_i for the twin itself (N = 40), and the conditional covariance is positive semi-definite and
    close to the exact posterior covariance only up to the random-feature error."""
    rng = np.random.default_rng(2)
    N, d = 40, 3
    X = rng.uniform(0, 1, (N, d))
    y = np.sin(3 * X.sum(1))
    tw = pr.PathTwin("Mat52Ard", X, y, np.full(d, -0.5), 0.1, -2.0, 0.2, 256, 4)
    for s in range(3):
        u, w = tw.u(s), tw.w(s)
        f = tw.value(X, u, w)
        resid = np.abs(f + tw.eps(s) + tw.diag * u - y)
        bound = tw.value_bound(X, u, w) + 64 * N * pr.EPS * (np.abs(tw.K) @ np.abs(u) + np.abs(tw.rhs(s)))
        assert np.all(resid <= bound), (resid / bound).max()
    xs = rng.uniform(0, 1, (5, d))
    mu, cov = pr.conditional_moments(tw, xs)
    assert np.linalg.eigvalsh(cov).min() > -1e-12
    # gradient of the twin against central differences of the twin
    u, w = tw.u(0), tw.w(0)
    g = tw.grad(xs, u, w)
    h = 1e-6
    for k in range(d):
        e = np.zeros(d); e[k] = h
        fd = (tw.value(xs + e, u, w) - tw.value(xs - e, u, w)) / (2 * h)
        np.testing.assert_allclose(g[:, k], fd, rtol=1e-6, atol=1e-7)


# ---- the ABI of the paths: include/bohip_paths.h <-> exports <-> _lib.PATHS_SIGNATURES <-> julia/BOHipPaths.jl -------------------
def test_paths_header_exports_ctypes_and_julia_agree(bo):
    """What tests/test_abi.py and tests/test_julia_binding.py do for include/bohip.h, for the header of the paths object: the same
    symbols everywhere, the same types argument by argument, and none of them in the model's header or tables."""
    import ctypes as C
    import re

    from bohip import _lib
    from conftest import ROOT

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip_paths.h")).read(), flags=re.S)
    hdr = re.sub(r"#.*", "", hdr)
    c_types = {"int": "int", "void": "void", "int64_t": "int64", "uint64_t": "uint64", "double*": "ptr(double)", "int64_t*": "ptr(int64)",
               "bohip_gp*": "ptr(void)", "bohip_paths*": "ptr(void)", "bohip_paths**": "ptr(ptr)", "bohip_best*": "ptr(best)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    want = {"bohip_gp_paths_draw", "bohip_paths_destroy", "bohip_paths_dims", "bohip_paths_eval", "bohip_paths_eval_grad", "bohip_paths_coef"}
    assert set(protos) == want == set(_lib.PATHS_SIGNATURES)
    assert not want & set(_lib.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    assert not want & set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {None: "void", C.c_int: "int", C.c_int64: "int64", C.c_uint64: "uint64", C.c_void_p: "ptr(void)",
          C.POINTER(C.c_double): "ptr(double)", C.POINTER(C.c_int64): "ptr(int64)", C.POINTER(C.c_void_p): "ptr(ptr)",
          C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Cvoid": "void", "Int64": "int64", "UInt64": "uint64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)",
                "Ptr{Int64}": "ptr(int64)", "Ptr{Ptr{Cvoid}}": "ptr(ptr)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipPaths.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == want
    for name in sorted(want):
        assert hasattr(lib, name), name
        res, args = _lib.PATHS_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipPaths.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    # block structure of the Julia file, as tests/test_julia_binding.py checks BOHip.jl's
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)
    # null objects never crash (no device needed)
    full = _lib.load()
    out = C.c_void_p(1)
    assert full.bohip_gp_paths_draw(None, 1, 16, 0, C.byref(out)) == _lib.E_ARG and not out.value
    full.bohip_paths_destroy(None)
    assert full.bohip_paths_dims(None, None, None, None, None) == _lib.E_ARG
    assert b"null" in full.bohip_last_error()


# ---- option plumbing against a stub model ------------------------------------------------------------------------------------
class StubPaths:
    def __init__(self, model, S, M, seed):
        self.model, self.S, self.M, self.seed, self.closed = model, S, M, seed, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        self.closed = True
        self.model.calls.append(("paths.close",))

    def _f(self, xs):                       # path s peaks at x = (0.2 + 0.1 s, ...): smooth, inside the unit box
        xs = np.asarray(xs, float)
        c = 0.2 + 0.1 * np.arange(self.S)
        return -np.sum((xs[None, :, :] - c[:, None, None]) ** 2, axis=1)      # S x R

    def eval(self, xs, want_values=True):
        F = self._f(xs)
        self.model.calls.append(("paths.eval", np.asarray(xs).shape, want_values))
        idx = np.argmax(F, axis=1)
        return (F if want_values else None), F[np.arange(self.S), idx], idx.astype(np.int64)

    def eval_grad(self, xs, path_of=None):
        xs = np.asarray(xs, float)
        po = np.zeros(xs.shape[1], dtype=np.int64) if path_of is None else np.asarray(path_of, dtype=np.int64)
        self.model.calls.append(("paths.eval_grad", xs.shape, None if path_of is None else po.tolist()))
        c = 0.2 + 0.1 * po
        return -np.sum((xs - c[None, :]) ** 2, axis=0), -2.0 * (xs - c[None, :])


class StubModel:
    def __init__(self, d=2, n=3):
        self.dim, self.calls = d, []
        self.x = np.zeros((d, n), order="F")
        self.y = np.arange(n, dtype=float)

    @property
    def nobs(self):
        return self.y.size

    def predict_f(self, xs):
        xs = np.asarray(xs, float).reshape(self.dim, -1)
        self.calls.append(("predict_f", xs.shape))
        return np.zeros(xs.shape[1]), np.ones(xs.shape[1])

    def score(self, acq, params, xs, want_scores=True):
        self.calls.append(("score", acq, xs.shape))
        return np.zeros(xs.shape[1]), 0.0, 0

    def append_(self, x, y):
        y = np.atleast_1d(y)
        self.calls.append(("append_", y.size))
        self.x = np.asfortranarray(np.concatenate([self.x, np.asarray(x).reshape(self.dim, -1)], axis=1))
        self.y = np.concatenate([self.y, y])

    def thompson(self, xs, S, seed=0, j0=0):
        self.calls.append(("thompson", xs.shape, S))
        return np.zeros(S), np.zeros(S, dtype=np.int64)

    def sample_joint(self, xs, S=1, seed=0, jitter=1e-12, max_tries=40, want_samples=True, want_factor=False):
        from bohip.model import JointSample

        self.calls.append(("sample_joint", xs.shape, S))
        R = xs.shape[1]
        F = -np.abs(np.arange(R)[None, :] - np.arange(S)[:, None]).astype(float)
        return JointSample(F if want_samples else None, F.max(1), F.argmax(1).astype(np.int64), np.zeros(R), 0.0, 0, None)

    def draw_paths(self, S=1, M=2048, seed=0):
        self.calls.append(("draw_paths", S, M))
        return StubPaths(self, S, M, seed)


def _names(m):
    return [c[0] for c in m.calls]


def test_acquire_max_defaults_reach_no_path_method(bo):
    lb, ub = np.zeros(2), np.ones(2)
    rng = np.random.default_rng(0)
    for opts in ({"method": "GN_DIRECT_L", "restarts": 1, "maxeval": 30}, {"method": "LN_COBYLA", "restarts": 2, "maxeval": 16},
                 {"method": "LN_COBYLA", "restarts": 1, "maxeval": 16, "joint": True},
                 {"method": "GN_DIRECT_L", "restarts": 1, "maxeval": 30, "pathwise": False, "features": 64}):
        m = StubModel()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                        # (LN_*: "not a local search", said once per process)
            bo.acquire_max(bo.ThompsonSamplingSimple(), m, lb, ub, opts, rng)
        assert not any(n.startswith("paths.") or n == "draw_paths" for n in _names(m)), m.calls


def test_acquire_max_pathwise_routes(bo):
    lb, ub = np.zeros(2), np.ones(2)
    rng = np.random.default_rng(0)
    # DIRECT: one path per restart, every batch of the search evaluated on it, closed afterwards
    m = StubModel()
    f, x = bo.acquire_max(bo.ThompsonSamplingSimple(), m, lb, ub,
                          {"method": "GN_DIRECT_L", "restarts": 2, "maxeval": 200, "pathwise": True, "features": 64}, rng)
    assert _names(m).count("draw_paths") == 2 and _names(m).count("paths.close") == 2
    assert [c for c in m.calls if c[0] == "draw_paths"] == [("draw_paths", 1, 64)] * 2
    assert "predict_f" not in _names(m) and "thompson" not in _names(m) and "paths.eval_grad" not in _names(m)
    assert np.allclose(x, 0.2, atol=0.02) and f > -1e-3            # the stub path's maximiser
    # LD_*: maxeval candidates on the path, then the ascent from the best `restarts` of them
    m = StubModel()
    f, x = bo.acquire_max(bo.ThompsonSamplingSimple(), m, lb, ub,
                          {"method": "LD_LBFGS", "restarts": 3, "maxeval": 50, "pathwise": True}, rng)
    assert [c for c in m.calls if c[0] == "draw_paths"] == [("draw_paths", 1, 2048)] * 3
    ev = [c for c in m.calls if c[0] == "paths.eval"]
    assert ev == [("paths.eval", (2, 50), True)] * 3
    gr = [c for c in m.calls if c[0] == "paths.eval_grad"]
    assert gr and all(c[1] == (2, 3) and c[2] is None for c in gr)
    assert np.allclose(x, 0.2, atol=1e-6) and f > -1e-10
    # any other method: candidates only (with the warning that it is no local search, said once per process)
    m = StubModel()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bo.acquire_max(bo.ThompsonSamplingSimple(), m, lb, ub, {"method": "LN_BOBYQA", "restarts": 1, "maxeval": 40, "pathwise": True}, rng)
    assert _names(m) == ["draw_paths", "paths.eval", "paths.close"] and m.calls[1] == ("paths.eval", (2, 40), False)
    # pathwise belongs to ThompsonSamplingSimple; unknown options still raise
    with pytest.raises(ValueError):
        bo.acquire_max(bo.ExpectedImprovement(), StubModel(), lb, ub, {"pathwise": True}, rng)
    with pytest.raises(ValueError):
        bo.acquire_max(bo.ThompsonSamplingSimple(), StubModel(), lb, ub, {"pathwise": True, "featurez": 8}, rng)


def test_thompson_batch_plumbing(bo):
    lb, ub = np.zeros(2), np.ones(2)
    rng = np.random.default_rng(1)
    m = StubModel()
    bo.acquire_thompson_batch(m, lb, ub, 3, {"candidates": 32}, rng)                 # default: the joint draw, no path method
    assert _names(m) == ["sample_joint"]
    m = StubModel()
    vals, X = bo.acquire_thompson_batch(m, lb, ub, 3, {"candidates": 9000, "pathwise": True, "features": 128, "refine": False}, rng)
    assert _names(m) == ["draw_paths", "paths.eval", "paths.close"] and m.calls[0] == ("draw_paths", 3, 128)
    assert m.calls[1] == ("paths.eval", (2, 9000), True) and X.shape == (2, 3)       # more candidates than one joint-draw chunk
    m = StubModel()
    v0, X0 = bo.acquire_thompson_batch(m, lb, ub, 3, {"xs": rng.random((2, 40)), "pathwise": True, "refine": False}, np.random.default_rng(5))
    m2 = StubModel()
    xs = np.random.default_rng(1).random((2, 40))
    v0, X0 = bo.acquire_thompson_batch(m2, lb, ub, 3, {"xs": xs, "pathwise": True, "refine": False}, rng)
    m3 = StubModel()
    v1, X1 = bo.acquire_thompson_batch(m3, lb, ub, 3, {"xs": xs, "pathwise": True, "maxeval": 60}, rng)
    gr = [c for c in m3.calls if c[0] == "paths.eval_grad"]
    assert gr and all(c[1] == (2, 3) and c[2] == [0, 1, 2] for c in gr)              # every pick on its own path
    assert np.all(v1 >= v0) and np.all((X1 >= 0) & (X1 <= 1))
    for s in range(3):                                                               # the refined points reach their path's peak
        assert np.allclose(X1[:, s], 0.2 + 0.1 * s, atol=1e-5)
    assert len({tuple(c) for c in X1.T}) == 3
    for bad in ({"features": 64}, {"refine": True}, {"maxeval": 5}, {"pathwise": True, "nope": 1}):
        with pytest.raises(ValueError):
            bo.acquire_thompson_batch(StubModel(), lb, ub, 2, bad, rng)


def test_bopt_forwards_the_pathwise_batch_options(bo):
    m = StubModel()
    o = bo.BOpt(lambda x: float(np.sum(x)), m, bo.ThompsonSamplingSimple(), bo.NoModelOptimizer(), [0.0, 0.0], [1.0, 1.0],
                maxiterations=2, initializer_iterations=0, verbosity=bo.Silent, rng=np.random.default_rng(0), batchsize=2,
                batchoptions={"candidates": 16, "pathwise": True, "features": 32, "refine": False})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bo.boptimize_(o)
    assert [c for c in m.calls if c[0] == "draw_paths"] == [("draw_paths", 2, 32)] * 2 and "sample_joint" not in _names(m)
    assert [c[1] for c in m.calls if c[0] == "append_"] == [2, 2]
