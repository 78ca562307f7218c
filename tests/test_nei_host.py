"""Noisy expected improvement without a GPU (include/bohip_nei.h): the evidence that the header's definition is the right
quantity, and the source of the bounds the device tests use.

  * an independent Monte Carlo over the dense joint posterior of (f_X, f(x)) with NumPy's own generator agrees with the twin;
  * the fantasies have the posterior's mean y - D alpha and covariance D - D A^-1 D;
  * with nu = delta -> 0 the score tends to EI at tau = max y, monotonically;
  * a twin that ignores the sites' weights lies more than 100 device bounds away (the bound is not vacuous);
  * the float64 twin against the extended-precision twin on every input of tests/test_nei_gpu.py: the constants nei_reference.WORST;
  * at most 1 case in 10 of the device tests is a near tie;
  * the ABI in every table that binds it.
"""
import ctypes as C
import math
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nei_reference as nr   # noqa: E402
import pend_reference as pr   # noqa: E402
from conftest import ROOT   # noqa: E402

WANT = {"bohip_gp_nei_prepare", "bohip_gp_nei_fantasies", "bohip_gp_score_nei", "bohip_nei_values", "bohip_gp_nei_info",
        "bohip_gp_nei_release"}


def small_twin(N, d=1, lnoise=-0.7, ll=math.log(0.3), seed=0, jitter_rel=1e-8):
    """A 1-d model whose noise is comparable to the signal (nu = 0.25 against s_f^2 = 1)."""
    rng = np.random.default_rng(seed)
    X = np.sort(rng.random((N, d)), axis=0)
    y = np.sin(6 * X).sum(1) + math.exp(lnoise) * rng.standard_normal(N)
    nu = math.exp(2 * lnoise) + nr.EPS
    return nr.Twin("SEArd", X, y, np.full(d, ll), 0.0, nu, 0.0, jitter_rel), X, y, nu


# ---- 1. an independent Monte Carlo -------------------------------------------------------------------------------------------------------
def test_independent_monte_carlo():
    """E max(f(x) - max f_X, 0) under the joint posterior of the noise-free values, drawn from its DENSE covariance with NumPy's
    generator -- no Matheron's rule, no companion, none of the library's normals -- against the twin's NEI at S = 1024.  The expected
    improvement of the textbook is what LogEI is the logarithm of (the library's EI is the reference's own formula, D Phi(z) + phi(z),
    src/acquisitionfunctions.jl:47-50), so the twin's figure is exp(NEI with a = LogEI): the log-mean-exp undone."""
    N, S, draws = 6, 1024, 200_000
    t, X, y, nu = small_twin(N, ll=math.log(0.2))
    Xs = np.array([-0.15, 0.1, 0.45, 0.8, 1.15])[:, None]
    P = np.vstack([X, Xs])
    K = nr.cov("SEArd", P, P, t.ll, 0.0, np.float64)
    A = K[:N, :N] + nu * np.eye(N)
    mean = K[:, :N] @ np.linalg.solve(A, y)
    covm = K - K[:, :N] @ np.linalg.solve(A, K[:N, :])
    f = np.random.default_rng(123).multivariate_normal(mean, covm, size=draws, method="eigh")
    imp = np.maximum(f[:, N:] - f[:, :N].max(axis=1)[:, None], 0.0)
    mc, mc_se = imp.mean(axis=0), imp.std(axis=0, ddof=1) / math.sqrt(draws)
    Z, E = nr.normals(7, S, N)
    _, tau, alpha = t.fantasies(Z, E)
    m, s2 = t.moments(Xs, alpha)
    lognei, each = nr.score("LogEI", m, s2, tau)
    nei, each = np.exp(lognei), np.exp(each)
    np.testing.assert_allclose(nei, each.mean(axis=0), rtol=1e-12)
    se = np.sqrt(mc_se ** 2 + (each.std(axis=0, ddof=1) / math.sqrt(S)) ** 2)
    print("MC", mc, "twin", nei, "combined standard errors apart", np.abs(mc - nei) / se)
    assert np.sum(mc > 10 * mc_se) >= 4                           # (the candidates have an improvement to speak of)
    assert np.all(np.abs(mc - nei) <= 4 * se)


# ---- 2. the fantasies' moments -----------------------------------------------------------------------------------------------------------
def test_fantasy_moments():
    N, S = 12, 1024
    t, X, y, nu = small_twin(N, seed=1)
    Z, E = nr.normals(11, S, N)
    F, _, _ = t.fantasies(Z, E)
    D = nu * np.eye(N)
    A = t.K + D
    mean = y - D @ np.linalg.solve(A, y)                          # y - D alpha (beta = 0)
    covm = D - D @ np.linalg.solve(A, D)                          # D - D A^-1 D
    dm = np.abs(F.mean(axis=0) - mean) / np.sqrt(np.diag(covm) / S)
    Cs = np.cov(F.T, ddof=1)
    dc = np.abs(Cs - covm) / np.sqrt((np.outer(np.diag(covm), np.diag(covm)) + covm ** 2) / S)
    print(f"mean: worst {dm.max():.2f} standard errors; covariance: worst {dc.max():.2f}")
    assert dm.max() <= 4 and dc.max() <= 4
    F0, tau0, _ = t.fantasies(*nr.normals(11, 0, N))             # S = 0: the posterior mean at the sites itself
    assert np.max(np.abs(F0[0] - mean)) <= 1e-12 and tau0[0] == F0[0].max()


# ---- 3. the noise limit ------------------------------------------------------------------------------------------------------------------
def test_noise_limit():
    """nu = delta: the companion is the model.  As nu -> 0 every tau_s -> max y and NEI -> EI(tau = max y); the gap shrinks
    monotonically over nu = 1e-4, 1e-6, 1e-8 s_f^2.  Recorded: max |NEI - EI| = 4.7e-2, 2.4e-2, 1.7e-3 (the last step's gap) and
    max |tau_s - max y| = 2.9e-2, 3.5e-3, 3.4e-4: eight sites a third of a length-scale apart amplify what noise is left."""
    N, S = 8, 64
    rng = np.random.default_rng(5)
    X = np.linspace(0.0, 1.0, N)[:, None]
    y = np.sin(6 * X).sum(1)
    Xs = rng.random((50, 1))
    Z, E = nr.normals(3, S, N)
    gaps, dtau = [], []
    for rel in (1e-4, 1e-6, 1e-8):
        t = nr.Twin("SEArd", X, y, np.array([math.log(0.3)]), 0.0, rel, 0.0, rel)
        _, tau, alpha = t.fantasies(Z, E)
        m, s2 = t.moments(Xs, alpha)
        nei, _ = nr.score("EI", m, s2, tau)
        m0, _ = t.moments(Xs, nr.solve_lower_t(t.Ld, nr.solve_lower(t.Ld, y[:, None])))
        ei = pr.acq("EI", [float(y.max())], m0[:, 0], s2)
        gaps.append(float(np.max(np.abs(nei - ei))))
        dtau.append(float(np.max(np.abs(tau - y.max()))))
    print("gaps", gaps, "tau", dtau)
    assert gaps[0] > gaps[1] > gaps[2] and dtau[0] > dtau[1] > dtau[2]


# ---- 4. the weights matter ---------------------------------------------------------------------------------------------------------------
def test_ignoring_the_weights_is_visible():
    good, bad = nr.reference("weighted", 5), nr.reference("weighted-ignored", 5)
    b = nr.bounds(good, 40)
    far_F = np.max(np.abs(bad["F"] - good["F"])) / b["F"]
    far_m = np.max(np.abs(bad["m"] - good["m"]) / b["m"])
    far_s = {a: float(np.max(nr.score_distance(a, nr.score(a, bad["m"], bad["s2"], bad["tau"])[0],
                                               nr.score(a, good["m"], good["s2"], good["tau"])[0], good["s2f"]))) / b[a] for a in nr.ACQS}
    print(f"a twin without the weights: F {far_F:.3g}, m {far_m:.3g}, scores {far_s} device bounds away")
    assert far_F > 100 and far_m > 100 and all(v > 100 for v in far_s.values())
    gj, bj = nr.reference("jitter", 5), nr.reference("jitter-ignored", 5)     # and so does the last refit's jitter
    assert np.max(np.abs(bj["F"] - gj["F"])) / nr.bounds(gj, 300)["F"] > 100


# ---- 5. where the device's bounds come from --------------------------------------------------------------------------------------------
def test_tolerance_source():
    worst = {k: 0.0 for k in nr.WORST}
    for tag, S in nr.all_inputs():
        f = nr.figures(nr.reference(tag, S), nr.reference(tag, S, dt=np.longdouble))
        for k in worst:
            worst[k] = max(worst[k], f[k])
    print("float64 twin against the extended twin, worst figures:", {k: f"{v:.3g}" for k, v in worst.items()})
    print("nei_reference.WORST:", nr.WORST)
    for k in worst:
        assert worst[k] <= 2 * nr.WORST[k], (k, worst[k])
        assert nr.WORST[k] <= 2 * worst[k], (k, "the stored constant is not the measured one")


def test_condition_numbers():
    for model in nr.MODELS:
        for N in nr.NS + ((nr.BIG_N,) if model == "se3" else ()):
            c = nr.twin((model, N)).cond_kd()
            print(f"{model} N = {N}: cond(K_d) at jitter_rel = 1e-6 is {c:.3g}")
            assert c < 1e9


# ---- 6. near ties ------------------------------------------------------------------------------------------------------------------------
def grid_cases():
    out = [(("se3", 129), 40, S) for S in nr.S_EDGES if S not in nr.SS]
    out += [((model, N), R, S) for model in nr.MODELS for N in nr.NS for R in nr.RS for S in nr.SS]
    return out


def test_near_ties_are_rare():
    ties, total = [], 0
    for tag, R, S in grid_cases():
        ref = nr.reference(tag, S)
        for acq in nr.ACQS:
            total += 1
            if nr.near_tie(acq, nr.score(acq, ref["m"][:R], ref["s2"][:R], ref["tau"])[0], ref["s2f"]):
                ties.append((tag, R, S, acq))
    print(f"{len(ties)} near ties in {total} cases: {ties}")
    assert len(ties) * 10 <= total


# ---- 7. the ABI --------------------------------------------------------------------------------------------------------------------------
def test_nei_header_exports_ctypes_and_julia_agree():
    """include/bohip_nei.h <-> exports <-> _lib.NEI_SIGNATURES <-> julia/BOHipNEI.jl: the same six symbols, the same types argument by
    argument, none of them in the model's header or table; the constants agree."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_nei.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double": "double", "double*": "ptr(double)", "bohip_gp*": "ptr(void)", "int64_t": "int64", "uint64_t": "uint64",
               "bohip_best*": "ptr(best)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.NEI_SIGNATURES)
    assert not WANT & set(_lib.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & declared and len(declared) == len(_lib.SIGNATURES) == 62
    consts = dict(re.findall(r"#define\s+(BOHIP_NEI_\w+)\s+(\d+)", raw))
    assert consts == {"BOHIP_NEI_SMAX": "1024", "BOHIP_NEI_INFO_REFITS": "0", "BOHIP_NEI_INFO_APPENDS": "1", "BOHIP_NEI_INFO_REBUILDS": "2",
                      "BOHIP_NEI_INFO_JITTER_STEPS": "3", "BOHIP_NEI_INFO_BYTES": "4", "BOHIP_NEI_INFO_DELTA": "5"}
    assert _lib.NEI_SMAX == 1024 and (_lib.NEI_INFO_REFITS, _lib.NEI_INFO_APPENDS, _lib.NEI_INFO_REBUILDS, _lib.NEI_INFO_JITTER_STEPS,
                                      _lib.NEI_INFO_BYTES, _lib.NEI_INFO_DELTA) == (0, 1, 2, 3, 4, 5)
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_double: "double", C.c_int64: "int64", C.c_uint64: "uint64", C.c_void_p: "ptr(void)",
          C.POINTER(C.c_double): "ptr(double)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Float64": "double", "Int64": "int64", "UInt64": "uint64", "Ptr{Cvoid}": "ptr(void)",
                "Ptr{Float64}": "ptr(double)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipNEI.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.NEI_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipNEI.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    for fn in ("nei", "nei_fantasies", "nei_prepare!", "nei_values", "nei_info", "nei_release!"):
        assert re.search(r"^function " + re.escape(fn) + r"\(", src, flags=re.M), fn
    assert re.search(r"^struct NoisyExpectedImprovement\b", src, flags=re.M)
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


def test_acquisition_type_and_refusals():
    import bohip
    import pytest

    a = bohip.NoisyExpectedImprovement(S=8, seed=3, log=True)
    assert (a.S, a.seed, a.log, a.jitter_rel) == (8, 3, True, 1e-8) and bohip.setparams_(a, None) is None
    for bad in (-1, 1025, 2.5, True):
        with pytest.raises(ValueError):
            bohip.NoisyExpectedImprovement(S=bad)
    with pytest.raises(ValueError):
        bohip.NoisyExpectedImprovement(jitter_rel=0.0)
    assert bohip.defaultoptions(bohip.ElasticGPE, bohip.NoisyExpectedImprovement) == dict(method="LD_LBFGS", restarts=1, maxeval=1024)

    class NoNEI:
        nobs = 3

    with pytest.raises(NotImplementedError):
        bohip.acquisitionfunction(a, NoNEI())(np.zeros(2))
