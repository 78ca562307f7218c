"""Two-objective optimisation without a GPU: the ABI of include/bohip_mo.h in every table that binds it, bohip_mo_front (host code of
the library) against its NumPy twin and a brute-force area, the NumPy twin of k_ehvi (tests/mo_reference.py) against mpmath, a
Monte-Carlo improvement, the hypervolume identity at sigma^2 = (0, 0) and central differences of the 50-digit value, and the plumbing
of ExpectedHypervolumeImprovement / MultiObjectiveGPE through acquisitionfunction, acquire_max and BOpt on duck-typed members whose
score is the twin."""
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
import mo_reference as mr   # noqa: E402
from conftest import ROOT   # noqa: E402
from matern_reference import MaternGP   # noqa: E402

WANT = {"bohip_mo_front", "bohip_mo_ehvi_values", "bohip_gp_score_mo"}
EPS = np.finfo(np.float64).eps


def test_mo_header_exports_ctypes_and_julia_agree():
    """include/bohip_mo.h <-> exports <-> _lib.MO_SIGNATURES <-> julia/BOHipMO.jl: the same symbols, the same types argument by
    argument, none of them in the other headers' tables; bohip.h keeps its 62."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_mo.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "int64_t": "int64", "double": "double", "double*": "ptr(double)", "int64_t*": "ptr(int64)",
               "bohip_best*": "ptr(best)", "bohip_gp*": "ptr(void)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.MO_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.PATHS_SIGNATURES, _lib.FIT_SIGNATURES, _lib.QEI_SIGNATURES, _lib.ACQ_SIGNATURES,
                  _lib.KG_SIGNATURES, _lib.ENS_SIGNATURES, _lib.ENS_GRAD_SIGNATURES, _lib.MES_SIGNATURES, _lib.CON_SIGNATURES):
        assert not WANT & set(other)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    main_syms = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & main_syms and len(main_syms) == 62 == len(_lib.SIGNATURES)
    assert "EXTENSION" in raw and "Emmerich" in raw and "Yang" in raw and "Daulton" in raw
    assert int(re.search(r"#define\s+BOHIP_MO_FRONT_MAX\s+(\d+)", raw).group(1)) == 1024 == _lib.MO_FRONT_MAX == mr.FRONT_MAX
    assert int(re.search(r"#define\s+BOHIP_MO_GROUP\s+(\d+)", raw).group(1)) == 16 == _lib.MO_GROUP == mr.G
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_double: "double", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int64): "ptr(int64)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "Float64": "double", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)",
                "Ptr{Int64}": "ptr(int64)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipMO.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.MO_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipMO.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert int(re.search(r"const MO_FRONT_MAX = (\d+)", src).group(1)) == 1024
    for name in ("function mo_front(", "function ehvi_values(", "function score_mo("):
        assert name in src, name
    import bohip
    for name in ("ExpectedHypervolumeImprovement", "MultiObjectiveGPE", "MOScore", "mo_front", "ehvi_values"):
        assert name in bohip.__all__ and hasattr(bohip, name)


# ---- bohip_mo_front: host code of the library ----------------------------------------------------------------------------------------
REF = np.array([-0.5, 0.25])


def front_cases():
    rng = np.random.default_rng(42)
    out = {n: rng.normal(size=(2, n)) + REF[:, None] + 0.5 for n in (0, 1, 2, 50, 2000)}
    Y = rng.uniform(0.0, 1.0, (2, 30)) + REF[:, None]
    out["all dominated by one"] = np.concatenate([Y, REF[:, None] + 2.0], axis=1)
    out["none above ref"] = REF[:, None] - rng.uniform(0.0, 1.0, (2, 20))
    out["on ref's edges"] = np.array([[REF[0], REF[0] + 1.0, REF[0] + 1.0], [REF[1] + 1.0, REF[1], REF[1] + 0.5]])
    Y = rng.integers(0, 6, (2, 80)).astype(np.float64)                          # a coarse grid: duplicates and ties in either coordinate
    out["duplicates and ties"] = Y
    out["ties in f1"] = np.array([[1.0, 1.0, 1.0, 2.0], [3.0, 5.0, 4.0, 1.0]])
    out["ties in f2"] = np.array([[1.0, 3.0, 2.0, 0.0], [2.0, 2.0, 2.0, 7.0]])
    return out


@pytest.mark.parametrize("name", [str(k) for k in front_cases()])
def test_front_against_the_twin(name):
    import bohip

    Y = {str(k): v for k, v in front_cases().items()}[name]
    fr, hv = bohip.mo_front(Y, REF)
    tf, thv = mr.front(Y, REF)
    assert fr.shape == tf.shape and fr.tobytes() == tf.tobytes() and hv == thv
    n = fr.shape[1]
    assert np.all(fr[0] > REF[0]) and np.all(fr[1] > REF[1]) and np.all(np.diff(fr[0]) > 0) and np.all(np.diff(fr[1]) < 0)
    for a, b in Y.T:                                                            # every observation above ref is weakly dominated by a front point
        if a > REF[0] and b > REF[1]:
            assert np.any((fr[0] >= a) & (fr[1] >= b))
    for i in range(n):                                                          # every front point is an observation no other one dominates
        assert np.any((Y[0] == fr[0, i]) & (Y[1] == fr[1, i]))
        assert not np.any((Y[0] >= fr[0, i]) & (Y[1] >= fr[1, i]) & ((Y[0] > fr[0, i]) | (Y[1] > fr[1, i])))
    if name == "all dominated by one":
        assert n == 1 and hv == 4.0
    if name in ("none above ref", "0"):
        assert n == 0 and hv == 0.0
    if name == "on ref's edges":
        assert n == 1                                                           # strictly above ref in both coordinates only
    if name == "ties in f1":
        assert fr.tolist() == [[1.0, 2.0], [5.0, 1.0]]
    if name == "ties in f2":
        assert fr.tolist() == [[0.0, 3.0], [7.0, 2.0]]
    if name == "2000":
        assert 2 < n < 200


def test_front_size_query_and_refusals():
    from bohip import _lib

    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    Y = np.ascontiguousarray(front_cases()[50])
    n = Y.shape[1]
    want, whv = mr.front(Y, REF)
    nf, hv = C.c_int64(-7), C.c_double(-1.0)
    assert lib.bohip_mo_front(ptr(Y), n, ptr(REF), None, 0, C.byref(nf), C.byref(hv)) == _lib.OK     # cap = 0: a size query
    assert nf.value == want.shape[1] > 2 and hv.value == whv
    out = np.full((2, nf.value), np.nan)
    assert lib.bohip_mo_front(ptr(Y), n, ptr(REF), ptr(out), nf.value, None, None) == _lib.OK
    assert out.tobytes() == want.tobytes()
    small = np.full((2, 2), np.nan)
    assert lib.bohip_mo_front(ptr(Y), n, ptr(REF), ptr(small), 2, C.byref(nf), None) == _lib.E_ARG and nf.value == want.shape[1]
    assert np.all(np.isnan(small))
    for bad in (np.nan, np.inf, -np.inf):
        Z = Y.copy()
        Z[1, 7] = bad
        assert lib.bohip_mo_front(ptr(Z), n, ptr(REF), ptr(out), nf.value, None, None) == _lib.E_ARG, bad
        r = np.array([0.0, bad])
        assert lib.bohip_mo_front(ptr(Y), n, ptr(r), ptr(out), nf.value, None, None) == _lib.E_ARG, bad
    assert lib.bohip_mo_front(ptr(Y), -1, ptr(REF), ptr(out), nf.value, None, None) == _lib.E_ARG
    assert lib.bohip_mo_front(ptr(Y), n, None, ptr(out), nf.value, None, None) == _lib.E_ARG
    assert lib.bohip_mo_front(None, 0, ptr(REF), None, 0, C.byref(nf), C.byref(hv)) == _lib.OK and nf.value == 0 and hv.value == 0.0


@pytest.mark.parametrize("n", [1, 2, 7, 50])
def test_hypervolume_against_a_brute_force_area(n):
    """The union of the rectangles [ref, y] over ALL observations above ref, cell by cell on the grid of their coordinates."""
    import bohip

    rng = np.random.default_rng(100 + n)
    Y = rng.integers(-3, 9, (2, n)).astype(np.float64) / 4.0 if n == 50 else rng.normal(size=(2, n)) + 0.5
    ref = np.array([-0.25, 0.0])
    _, hv = bohip.mo_front(Y, ref)
    P = Y[:, (Y[0] > ref[0]) & (Y[1] > ref[1])]
    xs = np.unique(np.concatenate([[ref[0]], P[0]]))
    ys = np.unique(np.concatenate([[ref[1]], P[1]]))
    area = 0.0
    for i in range(xs.size - 1):
        for j in range(ys.size - 1):
            if np.any((P[0] >= xs[i + 1]) & (P[1] >= ys[j + 1])):
                area += (xs[i + 1] - xs[i]) * (ys[j + 1] - ys[j])
    assert abs(hv - area) <= 4 * (xs.size * ys.size) * EPS * max(area, 1.0)


# ---- the twin against 50 digits ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted_ref(n_front, R):
    """crafted's inputs and the 50-digit table of one case (tests/test_mo_gpu.py shares the recipe and the cache)."""
    seed = mr.grid_seed(n_front, R)
    fr, ref, mu, var = mr.crafted(n_front, R, seed)
    tab = mr.mp_table(fr, ref, mu, var, cache=(n_front, R, seed))
    for a in (fr, ref, mu, var) + tuple(tab.values()):
        a.setflags(write=False)
    return fr, ref, mu, var, tab


@pytest.mark.parametrize("n_front", [0, 1, 2, 15, 16, 17, 64, 1024])
def test_twin_against_mpmath(n_front):
    """R = 257 crafted candidates: the value and the four partials within 2 x WORST of the 50-digit evaluator, relative to the sum
    the strip differences cancel against; the columns with a NaN or a negative moment are NaN and never win."""
    fr, ref, mu, var, tab = crafted_ref(n_front, 257)
    f, pm, pv = mr.ehvi(fr, ref, mu, var)
    sh = mr.shares((f, pm, pv), tab, {k: 2 * mr.WORST[k] for k in mr.KEYS})
    print(f"n_front={n_front}: worst share of 2 x WORST {sh}")
    assert max(sh.values()) <= 1.0, sh
    assert np.all(np.isnan(f[9:12])) and np.all(np.isnan(pm[:, 9:12])) and np.all(np.isnan(pv[:, 9:12]))
    assert np.all(pv[0, [0, 1, 2, 6, 7, 8]] == 0.0) and np.all(pv[1, [3, 4, 5, 6, 7, 8]] == 0.0)     # sigma^2 = 0: no variance partial
    assert f[7] == 0.0 and np.all(pm[:, 7] == 0.0)                                                      # a point mass below ref
    bv, bi = mr.record(f)
    assert bi >= 0 and f[bi] == bv == np.nanmax(f)


def test_recorded_tables_are_the_evaluator_s():
    """Three columns of every recorded 50-digit table, evaluated afresh: the files under tests/golden/ hold what mp_ehvi returns."""
    seen = 0
    for n_front, R in ((64, 257), (1024, 257), (1024, 1000), (63, 1000)):
        seed = mr.grid_seed(n_front, R)
        if not os.path.exists(mr._case_file(n_front, R, seed)):
            continue
        fr, ref, mu, var = mr.crafted(n_front, R, seed)
        tab = mr.mp_table(fr, ref, mu, var, cache=(n_front, R, seed))
        for j in (0, 13, R - 1) if n_front < 1024 else (13,):
            vals, scales = mr.mp_ehvi(fr, ref, mu[:, j], var[:, j])
            assert [tab[k][j] for k in mr.KEYS] == vals and [tab["S_" + k][j] for k in mr.KEYS] == scales
            seen += 1
    assert seen >= 4


@pytest.mark.parametrize("n_front", [0, 1, 5, 40])
def test_point_masses_give_the_hypervolume_difference(n_front):
    """sigma^2 = (0, 0): EHVI = HV(F u {mu}) - HV(F), both sides sums of n + 1 products of magnitude below HV(F u {mu})."""
    import bohip

    rng = np.random.default_rng(11 + n_front)
    fr, ref, _, _ = mr.crafted(n_front, 1, seed=3)
    mu = np.concatenate([rng.uniform(-3.0, 3.0, (2, 60)), fr, ref[:, None]], axis=1)       # anywhere, on the front's points, on ref
    f, pm, pv = mr.ehvi(fr, ref, mu, np.zeros_like(mu))
    Y0 = fr
    hv0 = bohip.mo_front(Y0, ref)[1]
    for j in range(mu.shape[1]):
        hv1 = bohip.mo_front(np.concatenate([Y0, mu[:, j:j + 1]], axis=1), ref)[1]
        assert abs(f[j] - (hv1 - hv0)) <= 4 * (n_front + 2) * EPS * max(hv1, 1e-300), (j, f[j], hv1 - hv0)
        assert f[j] == pytest.approx(mr.hvi(fr, ref, mu[:, j:j + 1])[0], rel=1e-13, abs=1e-15)
    assert np.all(pv == 0.0) and np.all(f[-(n_front + 1):] == 0.0) and np.any(f > 0.1)


@pytest.mark.parametrize("n_front", [0, 1, 5])
def test_twin_against_a_monte_carlo_improvement(n_front):
    """2 10^4 draws of (f1, f2) per candidate, a fixed seed: the mean hypervolume improvement within 5 standard errors of the twin."""
    rng = np.random.default_rng(2024 + n_front)
    fr, ref, _, _ = mr.crafted(n_front, 1, seed=8)
    R, S = 12, 20000
    mu, sd = rng.uniform(-2.5, 2.5, (2, R)), 10.0 ** rng.uniform(-1.0, 0.3, (2, R))
    f, _, _ = mr.ehvi(fr, ref, mu, sd * sd)
    for j in range(R):
        y = mu[:, j, None] + sd[:, j, None] * rng.standard_normal((2, S))
        imp = mr.hvi(fr, ref, y)
        se = imp.std(ddof=1) / math.sqrt(S)
        assert abs(imp.mean() - f[j]) <= 5.0 * se, (j, imp.mean(), f[j], se)
    assert np.any(f > 0.05)


@pytest.mark.parametrize("n_front", [5, 17])
def test_partials_against_central_differences_of_the_mpmath_value(n_front):
    """Central differences of the 50-digit value with steps 1e-12 sigma (in mu) and 1e-12 sigma^2 (in sigma^2): the truncation is
    below 1e-20 of the scale, so the twin's partials meet them within 2 x WORST."""
    import mpmath as mp

    fr, ref, mu, var = mr.crafted(n_front, 40, seed=5)
    f, pm, pv = mr.ehvi(fr, ref, mu, var)
    worst = {k: 0.0 for k in mr.KEYS[1:]}
    with mp.workdps(50):
        for j in range(12, 40, 3):
            _, scales = mr.mp_ehvi(fr, ref, mu[:, j], var[:, j])
            for m in range(2):
                for what, got, key in (("mu", pm[m, j], f"dmu{m + 1}"), ("var", pv[m, j], f"dvar{m + 1}")):
                    h = mp.mpf("1e-12") * (mp.sqrt(mp.mpf(var[m, j])) if what == "mu" else mp.mpf(var[m, j]))
                    vals = []
                    for sgn in (1, -1):
                        a, b = [mp.mpf(x) for x in mu[:, j]], [mp.mpf(x) for x in var[:, j]]
                        (a if what == "mu" else b)[m] += sgn * h
                        vals.append(mr.mp_ehvi(fr, ref, a, b, as_float=False)[0][0])
                    cd = float((vals[0] - vals[1]) / (2 * h))
                    S = scales[mr.KEYS.index(key)]
                    worst[key] = max(worst[key], abs(got - cd) / (2 * mr.WORST[key] * max(S, 1e-300)))
    print(f"n_front={n_front}: worst share of 2 x WORST against central differences {worst}")
    assert max(worst.values()) <= 1.0, worst


# ---- plumbing on duck-typed members -------------------------------------------------------------------------------------------------
class Duck:
    """What MultiObjectiveGPE and BOpt read of a member: dim, x, y, nobs, append_ -- and the twin's model of its observations."""

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
        return MaternGP(self.kern, self._x.T, self._y, np.full(self.dim, -0.7), 0.0, -2.0, float(np.mean(self._y)))


def twin_model(d, ref=None, kerns=("SEArd", "Mat52Ard")):
    """A MultiObjectiveGPE over Duck members whose score is mo_reference.score_mo (what the device call computes)."""
    from bohip.model import MOScore, MultiObjectiveGPE

    class TwinMO(MultiObjectiveGPE):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.calls = []

        def score(self, xs, want_grad=False, want_moments=True):
            self.calls.append((np.shape(xs), want_grad))
            ref_ = self.reference_point(fix=True)
            fr, _ = mr.front(self.y, ref_)
            tw = mr.score_mo([m.gp() for m in self.objectives], fr, ref_, np.asarray(xs).T, want_grad)
            return MOScore(tw["scores"], tw["grad"].T if want_grad else None, tw["mu"], tw["var"], tw["best_val"], tw["best_idx"])

    return TwinMO((Duck(d, kerns[0]), Duck(d, kerns[1])), ref)


def test_refusals():
    import bohip
    from bohip.model import MultiObjectiveGPE

    with pytest.raises(ValueError, match="two objectives"):
        MultiObjectiveGPE((Duck(2), Duck(2), Duck(2)))
    with pytest.raises(ValueError, match="dimension"):
        MultiObjectiveGPE((Duck(2), Duck(3)))
    with pytest.raises(ValueError):
        MultiObjectiveGPE((Duck(2), Duck(2)), ref=[0.0, np.inf])
    with pytest.raises(ValueError):
        MultiObjectiveGPE((Duck(2), Duck(2)), ref=[0.0, 1.0, 2.0])

    class MultiGPE(Duck):
        pass

    with pytest.raises(ValueError, match="MultiGPE"):
        MultiObjectiveGPE((Duck(2), MultiGPE(2)))
    m = twin_model(2)
    a = bohip.ExpectedHypervolumeImprovement()
    lo, hi = [0.0, 0.0], [1.0, 1.0]
    kw = dict(verbosity=bohip.Silent, maxiterations=6, initializer_iterations=3)
    two = lambda x: (0.0, 0.0)   # noqa: E731
    with pytest.raises(ValueError, match="ExpectedHypervolumeImprovement"):
        bohip.BOpt(two, m, bohip.ExpectedImprovement(), bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="ExpectedHypervolumeImprovement"):
        bohip.BOpt(two, m, bohip.Constrained(bohip.ExpectedImprovement()), bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="MultiObjectiveGPE"):
        bohip.BOpt(lambda x: 0.0, Duck(2), a, bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="batchsize"):
        bohip.BOpt(two, m, a, bohip.NoModelOptimizer(), lo, hi, batchsize=2, **kw)
    with pytest.raises(ValueError, match="MarginalGPOptimizer"):
        bohip.BOpt(two, m, a, bohip.MarginalGPOptimizer(), lo, hi, **kw)
    one = Duck(2)
    one.append_(np.full((2, 1), 0.5), [0.0])
    with pytest.raises(ValueError, match="MultiObjectiveGPE"):
        bohip.acquire_max(a, one, lo, hi, dict(maxeval=8))
    with pytest.raises(ValueError, match="MultiObjectiveGPE"):
        bohip.acquisitionfunction(a, Duck(2))
    o = bohip.BOpt(lambda x: (0.0, 1.0, 2.0), m, a, bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="y_1, y_2"):
        bohip.boptimize_(o)                                                      # func must return two numbers
    with pytest.raises(ValueError, match="2 x n"):
        m.update_(np.zeros((2, 3)), np.zeros((3, 3)))
    assert bohip.defaultoptions(type(m), type(a)) == dict(method="LD_LBFGS", restarts=1, maxeval=1024)


def test_the_default_reference_point_is_fixed_once_at_the_first_score():
    import bohip

    m = twin_model(2)
    X = np.random.default_rng(0).random((2, 6))
    Y = np.array([[1.0, 3.0, 2.0, 5.0, 4.0, 2.5], [7.0, 7.0, 7.0, 7.0, 7.0, 7.0]])    # the second objective has range 0
    m.update_(X, Y)
    assert m.ref is None and m.nobs == 6 and m.y.tobytes() == Y.tobytes() and m.x.shape == (2, 6)
    want = np.array([1.0 - 0.1 * 4.0, 7.0 - 1.0])
    np.testing.assert_array_equal(m.default_ref(), want)
    fr, hv = m.front, m.hypervolume                                              # (not fixed by looking at the front)
    assert m.ref is None and fr.tolist() == [[5.0], [7.0]] and hv == (5.0 - want[0]) * 1.0
    f = bohip.acquisitionfunction(bohip.ExpectedHypervolumeImprovement(), m)
    xs = np.random.default_rng(1).random((2, 9))
    sc = f(xs)
    np.testing.assert_array_equal(m.ref, want)
    assert sc.shape == (9,) and np.all(sc >= 0.0)
    with pytest.raises(ValueError):
        f(xs[:, 0])
    m.update_(np.array([[0.5], [0.5]]), np.array([[-10.0], [20.0]]))            # new extremes do not move a fixed reference point
    m.score(xs)
    np.testing.assert_array_equal(m.ref, want)
    assert m.front.tolist() == [[5.0], [7.0]]                                   # (-10, 20) is not above ref in f1
    given = twin_model(2, ref=[0.0, 1.0])
    given.update_(X, Y)
    given.score(xs)
    np.testing.assert_array_equal(given.ref, [0.0, 1.0])
    with pytest.raises(ValueError, match="observations"):
        twin_model(2).default_ref()


def test_acquire_max_refine_never_below_the_candidates():
    import bohip

    m = twin_model(2, ref=[-2.0, -2.0])
    rng = np.random.default_rng(2)
    X = rng.random((2, 10))
    m.update_(X, np.stack([-((X - 0.2) ** 2).sum(0), -((X - 0.8) ** 2).sum(0)]))
    a = bohip.ExpectedHypervolumeImprovement()
    f0, x0 = bohip.acquire_max(a, m, [0.0, 0.0], [1.0, 1.0], dict(maxeval=64, restarts=1), np.random.default_rng(9))
    f1, x1 = bohip.acquire_max(a, m, [0.0, 0.0], [1.0, 1.0], dict(maxeval=64, restarts=1, refine=3), np.random.default_rng(9))
    assert f1 >= f0 > 0.0 and np.all(x1 >= 0.0) and np.all(x1 <= 1.0)
    assert [c[1] for c in m.calls].count(False) == 2 and m.calls[0][0] == (2, 64) and any(c[1] for c in m.calls)
    assert all(c[0] == (2, 3) for c in m.calls if c[1])                          # the ascent: one gradient call over the 3 starts per step


@pytest.mark.parametrize("sense", ["Max", "Min"])
def test_bopt_on_the_twin(sense):
    """A short loop on the twin: sense = Min flips both objectives, every proposal is in the box, the hypervolume never decreases, and
    the result carries the observed front in the caller's sense, the hypervolume, and no single optimum."""
    import bohip

    sgn = 1.0 if sense == "Max" else -1.0
    seen = []

    def func(x):
        y = (-sgn * ((x[0] - 0.2) ** 2 + (x[1] - 0.3) ** 2), -sgn * ((x[0] - 0.8) ** 2 + (x[1] - 0.7) ** 2))
        seen.append((np.array(x), y))
        return y

    m = twin_model(2)
    hvs = []
    m_score = m.score
    m.score = lambda *a, **k: (hvs.append(m.hypervolume) if m.ref is not None else None, m_score(*a, **k))[1]
    o = bohip.BOpt(func, m, bohip.ExpectedHypervolumeImprovement(), bohip.NoModelOptimizer(), [0.0, 0.0], [1.0, 1.0],
                   sense=getattr(bohip, sense), maxiterations=10, verbosity=bohip.Silent, initializer_iterations=5,
                   acquisitionoptions=dict(maxeval=96, refine=2), rng=np.random.default_rng(5))
    assert o.observed_optimum is None and o.model_optimum is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = bohip.boptimize_(o)
    X = np.array([s[0] for s in seen])
    Yc = np.array([s[1] for s in seen]).T                                         # the caller's values [2, 10]
    assert len(seen) == 10 and np.all(X >= 0.0) and np.all(X <= 1.0)
    np.testing.assert_array_equal(m.y, sgn * Yc)                                  # both objectives flipped under Min
    init = sgn * Yc[:, :5]
    lo, hi = init.min(axis=1), init.max(axis=1)
    np.testing.assert_array_equal(m.ref, lo - 0.1 * (hi - lo))                    # fixed after the initial design, by the default rule
    assert res["observed_optimum"] is None and res["model_optimum"] is None and res["observed_optimizer"] is None
    tf, thv = mr.front(sgn * Yc, m.ref)
    assert res["hypervolume"] == thv == m.hypervolume and thv > 0.0
    np.testing.assert_array_equal(res["observed_front"]["y"], sgn * tf)           # in the caller's sense
    np.testing.assert_array_equal(res["ref"], sgn * m.ref)
    fx = res["observed_front"]["x"]
    assert fx.shape == (2, tf.shape[1])
    for i in range(tf.shape[1]):
        assert np.allclose(func(fx[:, i]), res["observed_front"]["y"][:, i], rtol=0, atol=0)
    hvs.append(m.hypervolume)
    assert all(b >= a for a, b in zip(hvs, hvs[1:])) and hvs[-1] > hvs[0]
    assert m.calls[0] == ((2, 96), False) and any(c[1] for c in m.calls)
