"""Two to four objectives without a GPU: the ABI of include/bohip_mom.h in every table that binds it, bohip_mom_front and
bohip_mom_boxes (host code of the library) against their NumPy twins and brute-force cell counts, the NumPy twin of k_ehvi_boxes
(tests/mom_reference.py) against mpmath, against the two-objective strip form, a Monte-Carlo improvement and central differences of
the 50-digit value, and the plumbing of ExpectedHypervolumeImprovement / ManyObjectiveGPE through acquisitionfunction, acquire_max and
BOpt on duck-typed members whose score is the twin."""
import ctypes as C
import functools
import itertools
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mo_reference as mr   # noqa: E402
import mom_reference as qr   # noqa: E402
from conftest import ROOT   # noqa: E402
from test_mo_host import Duck   # noqa: E402

WANT = {"bohip_mom_front", "bohip_mom_boxes", "bohip_mom_ehvi_values", "bohip_gp_score_mom"}
EPS = np.finfo(np.float64).eps


def test_mom_header_exports_ctypes_and_julia_agree():
    """include/bohip_mom.h <-> exports <-> _lib.MOM_SIGNATURES <-> julia/BOHipMOM.jl: the same four symbols, the same types argument
    by argument, in no other header or table; bohip.h keeps its 62 and bohip_mo.h its 3."""
    from bohip import _lib

    def protos_of(name):
        raw = open(os.path.join(ROOT, "include", name)).read()
        hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
        return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr)}

    c_types = {"int": "int", "int64_t": "int64", "double*": "ptr(double)", "int64_t*": "ptr(int64)", "int32_t*": "ptr(int32)",
               "bohip_best*": "ptr(best)", "bohip_gp*": "ptr(void)", "bohip_gp**": "ptr(ptr(void))"}
    protos = {}
    for name, (res, arglist) in protos_of("bohip_mom.h").items():
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in arglist.split(",")]
        protos[name] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [res] + args]
    assert set(protos) == WANT == set(_lib.MOM_SIGNATURES)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "bohip_mom.h":
            assert not WANT & set(protos_of(other)), other
    for k in [k for k in vars(_lib) if k.endswith("SIGNATURES") and k != "MOM_SIGNATURES"]:
        assert not WANT & set(getattr(_lib, k)), k
    assert len(protos_of("bohip_mo.h")) == 3 == len(_lib.MO_SIGNATURES) and len(_lib.SIGNATURES) == 62
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))) == 62
    raw = open(os.path.join(ROOT, "include", "bohip_mom.h")).read()
    assert "EXTENSION" in raw and "Emmerich" in raw and "Yang" in raw and "Daulton" in raw
    for name, want, mine in (("OBJ_MAX", 4, qr.OBJ_MAX), ("FRONT_MAX", 256, qr.FRONT_MAX), ("BOX_MAX", 65536, qr.BOX_MAX),
                             ("LANES", 64, qr.LANES)):
        assert int(re.search(rf"#define\s+BOHIP_MOM_{name}\s+(\d+)", raw).group(1)) == want == getattr(_lib, "MOM_" + name) == mine
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int64): "ptr(int64)", C.POINTER(C.c_int32): "ptr(int32)", C.POINTER(_lib.Best): "ptr(best)",
          C.POINTER(C.c_void_p): "ptr(ptr(void))"}
    jl_types = {"Cint": "int", "Int64": "int64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)", "Ptr{Int64}": "ptr(int64)",
                "Ptr{Int32}": "ptr(int32)", "Ptr{Best}": "ptr(best)", "Ptr{Ptr{Cvoid}}": "ptr(ptr(void))"}
    src = open(os.path.join(ROOT, "julia", "BOHipMOM.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.MOM_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
        assert getattr(_lib.load(), name).argtypes == args                       # bound by the load loop
    for f in os.listdir(os.path.join(ROOT, "julia")):
        if f.endswith(".jl") and f != "BOHipMOM.jl":
            assert ":bohip_mom_" not in open(os.path.join(ROOT, "julia", f)).read() and ":bohip_gp_score_mom" not in open(
                os.path.join(ROOT, "julia", f)).read(), f
    assert 'include("BOHipMOM.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    for name in ("function mom_front(", "function mom_boxes(", "function ehvi_values_many(", "function score_mom("):
        assert name in src, name
    for c, v in (("MOM_OBJ_MAX", 4), ("MOM_FRONT_MAX", 256), ("MOM_BOX_MAX", 65536), ("MOM_LANES", 64)):
        assert int(re.search(rf"const {c} = (\d+)", src).group(1)) == v
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try|abstract type)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    import bohip
    for name in ("ManyObjectiveGPE", "mom_front", "mom_boxes", "ehvi_values_many", "score_mom"):
        assert name in bohip.__all__ and hasattr(bohip, name)


# ---- bohip_mom_front and bohip_mom_boxes: host code of the library ------------------------------------------------------------------
def observations(M, n, seed):
    """n observations around ref on a coarse grid (duplicates and ties in every coordinate) for even seeds, continuous for odd."""
    rng = np.random.default_rng(seed)
    ref = qr.REF4[:M] + 2.0
    Y = rng.integers(-2, 6, (M, n)).astype(np.float64) / 2.0 if seed % 2 == 0 else rng.normal(size=(M, n)) + ref[:, None] + 0.5
    return Y, ref


@pytest.mark.parametrize("n", [0, 1, 2, 8, 40])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_front_and_boxes_against_the_twin(M, n):
    import bohip

    for seed in (10 * n + M, 10 * n + M + 1):
        Y, ref = observations(M, n, seed)
        fr, hv = bohip.mom_front(Y, ref)
        tf, thv = qr.front(Y, ref)
        assert fr.shape == tf.shape and fr.tobytes() == tf.tobytes() and hv == thv
        nf = fr.shape[1]
        assert np.all(fr > ref[:, None]) and [tuple(c) for c in fr.T] == sorted({tuple(c) for c in fr.T})     # lexicographic, distinct
        for y in Y.T:                                                           # every observation above ref is weakly dominated by a front point
            if np.all(y > ref):
                assert np.any(np.all(fr >= y[:, None], axis=0))
        for i in range(nf):                                                     # every front point is an observation no other one dominates
            assert np.any(np.all(Y == fr[:, i:i + 1], axis=0))
            assert not np.any(np.all(Y >= fr[:, i:i + 1], axis=0) & np.any(Y > fr[:, i:i + 1], axis=0))
        L, B = bohip.mom_boxes(fr, ref)
        tL, tB = qr.boxes(tf, ref)
        assert B.dtype == np.int32 and B.shape == tB.shape and B.tobytes() == tB.tobytes()
        assert len(L) == M and all(a.tobytes() == b.tobytes() for a, b in zip(L, tL))
        for m in range(M):
            assert L[m][0] == ref[m] and L[m][-1] == np.inf and np.all(np.diff(L[m]) > 0) and L[m].size <= nf + 2
            assert np.all(B[m] >= 0) and np.all(B[m] < B[M + m]) and np.all(B[M + m] < L[m].size)
        if M == 3:
            assert B.shape[1] <= (nf + 1) * (nf + 2) // 2
        if M == 2:
            assert B.shape[1] == nf + 1
        perm = np.random.default_rng(seed).permutation(n)                       # the SET decides: permuted observations, a permuted front
        fr2, hv2 = bohip.mom_front(Y[:, perm], ref)
        assert fr2.tobytes() == fr.tobytes() and hv2 == hv
        L2, B2 = bohip.mom_boxes(np.ascontiguousarray(fr[:, ::-1]), ref)
        assert B2.tobytes() == B.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(L, L2))


@pytest.mark.parametrize("M", [2, 3, 4])
def test_boxes_against_a_brute_force_cell_count(M):
    """An integer-grid front above ref = 0: the dominated region's unit cells count hv, and for 20 seeded points y the box-sum
    improvement counts the cells below y that no front point dominates -- exactly, every quantity is a small integer."""
    import bohip

    rng = np.random.default_rng(500 + M)
    ref = np.zeros(M)
    while True:                                                                 # (the first seeded draw whose front has several points)
        Y = rng.integers(1, 6, (M, 12)).astype(np.float64)
        fr, hv = bohip.mom_front(Y, ref)
        if fr.shape[1] >= 3:
            break
    cells = np.array(list(itertools.product(range(6), repeat=M)), dtype=np.float64)       # the cell [c, c + 1)
    dominated = np.array([np.any(np.all(fr >= c[:, None] + 1.0, axis=0)) for c in cells])
    assert hv == dominated.sum() == qr.front(Y, ref)[1]
    L, B = bohip.mom_boxes(fr, ref)
    vol = np.prod([np.where(np.isinf(L[m][B[M + m]]), 6.0, L[m][B[M + m]]) - L[m][B[m]] for m in range(M)], axis=0)
    assert vol.sum() == 6 ** M - hv                                             # the boxes partition what is not dominated (cut at 6)
    for _ in range(20):
        y = rng.integers(0, 7, M).astype(np.float64)
        want = np.sum(~dominated & np.all(y[None, :] >= cells + 1.0, axis=1))
        assert qr.hvi(fr, ref, y[:, None])[0] == want, (y, want)


def test_caps_and_refusals():
    from bohip import _lib

    lib = _lib.load()
    dp, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    M = 3
    Y, ref = observations(M, 40, 7)
    Y = np.ascontiguousarray(Y)
    n = Y.shape[1]
    want, whv = qr.front(Y, ref)
    nf, hv = C.c_int64(-7), C.c_double(-1.0)
    assert lib.bohip_mom_front(ptr(Y), M, n, ptr(ref), None, 0, C.byref(nf), C.byref(hv)) == _lib.OK     # cap = 0: a size query
    assert nf.value == want.shape[1] > 2 and hv.value == whv
    out = np.full((M, nf.value), np.nan)
    assert lib.bohip_mom_front(ptr(Y), M, n, ptr(ref), ptr(out), nf.value, None, None) == _lib.OK and out.tobytes() == want.tobytes()
    small = np.full((M, 2), np.nan)
    assert lib.bohip_mom_front(ptr(Y), M, n, ptr(ref), ptr(small), 2, C.byref(nf), None) == _lib.E_ARG and nf.value == want.shape[1]
    assert np.all(np.isnan(small))
    for bad in (np.nan, np.inf, -np.inf):
        Z = Y.copy()
        Z[1, 7] = bad
        assert lib.bohip_mom_front(ptr(Z), M, n, ptr(ref), ptr(out), nf.value, None, None) == _lib.E_ARG, bad
        r = ref.copy()
        r[2] = bad
        assert lib.bohip_mom_front(ptr(Y), M, n, ptr(r), ptr(out), nf.value, None, None) == _lib.E_ARG, bad
    for badM in (1, 5, 0, -1):
        assert lib.bohip_mom_front(ptr(Y), badM, n, ptr(ref), ptr(out), nf.value, None, None) == _lib.E_ARG
        assert lib.bohip_mom_boxes(ptr(want), badM, want.shape[1], ptr(ref), None, None, None, 0, None) == _lib.E_ARG
    assert lib.bohip_mom_front(ptr(Y), M, -1, ptr(ref), ptr(out), nf.value, None, None) == _lib.E_ARG
    assert lib.bohip_mom_front(ptr(Y), M, n, None, ptr(out), nf.value, None, None) == _lib.E_ARG
    assert lib.bohip_mom_front(None, M, 0, ptr(ref), None, 0, C.byref(nf), C.byref(hv)) == _lib.OK and nf.value == 0 and hv.value == 0.0

    def bx(fr, r=ref, cap=0, boxes=None, nb=None, m=None):
        m = fr.shape[0] if m is None else m
        return lib.bohip_mom_boxes(ptr(fr), m, fr.shape[1], ptr(r), None, None, None if boxes is None else boxes.ctypes.data_as(i32p), cap,
                                   None if nb is None else C.byref(nb))

    nb = C.c_int64(0)
    tB = qr.boxes(want, ref)[1]
    assert bx(want, nb=nb) == _lib.OK and nb.value == tB.shape[1]
    got = np.full((2 * M, nb.value + 3), -1, dtype=np.int32)                    # cap above the count: the rows keep the stride cap
    assert bx(want, cap=nb.value + 3, boxes=got) == _lib.OK and np.array_equal(got[:, :nb.value], tB) and np.all(got[:, nb.value:] == -1)
    tiny = np.full((2 * M, 1), -1, dtype=np.int32)
    nb2 = C.c_int64(0)
    assert bx(want, cap=1, boxes=tiny, nb=nb2) == _lib.E_ARG and nb2.value == nb.value and np.all(tiny == -1)
    assert bx(want, cap=4) == _lib.E_ARG                                        # cap without a buffer
    dup = np.ascontiguousarray(np.concatenate([want, want[:, :1]], axis=1))
    assert bx(dup) == _lib.E_ARG and b"dominated" in lib.bohip_last_error()
    dom = np.ascontiguousarray(np.concatenate([want, want[:, :1] - np.array([[0.0], [0.125], [0.0]])], axis=1))
    assert bx(dom) == _lib.E_ARG and b"dominated" in lib.bohip_last_error()     # weakly dominated: equal in two coordinates
    on_ref = want.copy()
    on_ref[1, 0] = ref[1]
    assert bx(on_ref) == _lib.E_ARG and b"above ref" in lib.bohip_last_error()
    nan = want.copy()
    nan[0, 1] = np.nan
    assert bx(nan) == _lib.E_ARG
    rng = np.random.default_rng(3)
    for Mm in (2, 3, 4):
        big = qr.sphere_front(Mm, 257, rng)
        assert bx(big, r=qr.REF4[:Mm]) == _lib.E_UNSUPPORTED and b"257" in lib.bohip_last_error()
    full = qr.sphere_front(3, 256, rng)
    assert bx(full, r=qr.REF4[:3], nb=nb) == _lib.OK and 257 <= nb.value <= 257 * 258 // 2
    many = qr.sphere_front(4, 256, rng)                                         # 256 random points in four objectives: beyond the box limit
    assert bx(many, r=qr.REF4, nb=nb) == _lib.E_UNSUPPORTED and nb.value > 65536
    assert str(nb.value).encode() in lib.bohip_last_error() and b"65536" in lib.bohip_last_error()
    # the device entry points validate before they touch a device: a null handle is refused first, then the front
    mu = np.zeros((3, 2))
    for call in (lambda: lib.bohip_mom_ehvi_values(None, 3, ptr(want), want.shape[1], ptr(ref), ptr(mu), ptr(mu), 2, ptr(mu), None, None, None),
                 lambda: lib.bohip_gp_score_mom(None, 3, ptr(want), want.shape[1], ptr(ref), ptr(mu), 2, ptr(mu), None, None, None, None)):
        assert call() == _lib.E_ARG


# ---- the twin against 50 digits ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted_ref(M, n_front, R):
    """crafted's inputs and the 50-digit table of one case (tests/test_mom_gpu.py shares the recipe and the cache)."""
    seed = qr.grid_seed(M, n_front, R)
    fr, ref, mu, var = qr.crafted(M, n_front, R, seed)
    tab = qr.mp_table(fr, ref, mu, var, cache=(M, n_front, R, seed))
    for a in (fr, ref, mu, var) + tuple(tab.values()):
        a.setflags(write=False)
    return fr, ref, mu, var, tab


def test_crafted_fronts_hold_ties():
    """At least two front points share a value in the last objective and two share one in the first (M >= 3: with two objectives
    one of such a pair dominates the other), so a level array is shorter than the front."""
    for M in (3, 4):
        fr, ref, _, _ = qr.crafted(M, 17, 4, qr.grid_seed(M, 17, 257))
        assert fr[M - 1, 0] == fr[M - 1, 1] and fr[0, 2] == fr[0, 3]
        L, B = qr.boxes(fr, ref)
        assert L[0].size == 17 + 1 and L[M - 1].size == 17 + 1 and qr.front(fr, ref)[0].shape == fr.shape


@pytest.mark.parametrize("case", qr.GRID, ids=lambda c: "M{}-n{}-R{}".format(*c))
def test_twin_against_mpmath(case):
    """The value and the 2M partials within 2 x WORST of the 50-digit evaluator, relative to the box sum the differences cancel
    against; the columns with a NaN or a negative moment are NaN and never win."""
    M, n_front, R = case
    fr, ref, mu, var, tab = crafted_ref(M, n_front, R)
    f, pm, pv = qr.ehvi(fr, ref, mu, var)
    sh = qr.shares((f, pm, pv), tab, 2 * qr.WORST)
    print(f"M={M} n_front={n_front} boxes={qr.boxes(fr, ref)[1].shape[1]}: worst share of 2 x WORST {sh}")
    assert max(sh.values()) <= 1.0, sh
    assert np.all(np.isnan(f[9:12])) and np.all(np.isnan(pm[:, 9:12])) and np.all(np.isnan(pv[:, 9:12]))
    assert np.all(pv[0, [0, 1, 2, 6, 7, 8]] == 0.0) and np.all(pv[M - 1, 3:9] == 0.0) and np.all(pv[:, 6:9] == 0.0)     # sigma^2 = 0
    assert f[7] == 0.0 and np.all(pm[:, 7] == 0.0)                              # a point mass below ref
    bv, bi = qr.record(f)
    assert bi >= 0 and f[bi] == bv == np.nanmax(f)


def test_recorded_tables_are_the_evaluator_s():
    """Two columns of every recorded 50-digit table, evaluated afresh: the files under tests/golden/ hold what mp_ehvi returns."""
    seen = 0
    for M, n_front, R in qr.GRID:
        seed = qr.grid_seed(M, n_front, R)
        if not os.path.exists(qr._case_file(M, n_front, R, seed)):
            continue
        assert os.path.getsize(qr._case_file(M, n_front, R, seed)) < 200 * 1024
        fr, ref, mu, var = qr.crafted(M, n_front, R, seed)
        tab = qr.mp_table(fr, ref, mu, var, cache=(M, n_front, R, seed))
        for j in (13, R - 1) if n_front <= 17 else (13,):
            vals, scales = qr.mp_ehvi(fr, ref, mu[:, j], var[:, j])
            assert [tab[k][j] for k in qr.keys(M)] == vals and [tab["S_" + k][j] for k in qr.keys(M)] == scales
            seen += 1
    assert seen >= 4


@pytest.mark.parametrize("n_front", [0, 1, 2, 8, 17])
def test_two_objectives_against_the_strip_form(n_front):
    """M = 2: the box sum against mo_reference.ehvi (the strips of k_ehvi) on the same inputs, within the sum of both twins'
    2 x WORST shares, each relative to the sum its own differences cancel against."""
    fr, ref, mu, var, tab = crafted_ref(2, n_front, 257)
    fs = np.ascontiguousarray(fr[:, np.argsort(fr[0])])                         # (the strip form asks for ascending f1; the boxes for a set)
    strip_tab = mr.mp_table(fs, ref, mu, var)
    a, b = qr.ehvi(fr, ref, mu, var), mr.ehvi(fs, ref, mu, var)
    ok = np.isfinite(tab["value"])
    mine = dict(zip(qr.keys(2), (a[0],) + tuple(a[1]) + tuple(a[2])))
    theirs = dict(zip(qr.keys(2), (b[0],) + tuple(b[1]) + tuple(b[2])))
    for k, ks in zip(qr.keys(2), ("value", "dmu1", "dmu2", "dvar1", "dvar2")):
        bound = 2 * qr.WORST * np.maximum(tab["S_" + k][ok], 1e-300) + 2 * mr.WORST[ks] * np.maximum(strip_tab["S_" + ks][ok], 1e-300)
        assert np.all(np.abs(mine[k][ok] - theirs[k][ok]) <= bound), k
        assert np.all(np.isnan(mine[k][~ok])) and np.all(np.isnan(theirs[k][~ok]))


@pytest.mark.parametrize("M,n_front", [(3, 6), (4, 5)])
def test_twin_against_a_monte_carlo_improvement(M, n_front):
    """2 10^4 draws of f per candidate, a fixed seed: the mean hypervolume improvement within 5 standard errors of the twin."""
    rng = np.random.default_rng(2024 + M)
    fr, ref, _, _ = qr.crafted(M, n_front, 1, seed=8)
    R, S = 8, 20000
    mu, sd = rng.uniform(0.0, 2.5, (M, R)), 10.0 ** rng.uniform(-0.5, 0.3, (M, R))     # (where an improvement is not a rare event)
    f, _, _ = qr.ehvi(fr, ref, mu, sd * sd)
    worst = 0.0
    for j in range(R):
        y = mu[:, j, None] + sd[:, j, None] * rng.standard_normal((M, S))
        imp = qr.hvi(fr, ref, y)
        se = imp.std(ddof=1) / math.sqrt(S)
        worst = max(worst, abs(imp.mean() - f[j]) / se)
        assert abs(imp.mean() - f[j]) <= 5.0 * se, (j, imp.mean(), f[j], se)
    print(f"M={M}: worst {worst:.2f} standard errors")
    assert np.any(f > 0.05)


@pytest.mark.parametrize("M", [2, 3, 4])
def test_point_masses_give_the_hypervolume_difference(M):
    """sigma^2 = 0 in every objective: EHVI = HV(F u {mu}) - HV(F), both sides sums of products of magnitude below HV(F u {mu})."""
    import bohip

    rng = np.random.default_rng(11 + M)
    fr, ref, _, _ = qr.crafted(M, 6, 1, seed=3)
    mu = np.concatenate([rng.uniform(-3.0, 3.0, (M, 40)), fr, ref[:, None]], axis=1)       # anywhere, on the front's points, on ref
    f, pm, pv = qr.ehvi(fr, ref, mu, np.zeros_like(mu))
    hv0 = bohip.mom_front(fr, ref)[1]
    nb = qr.boxes(fr, ref)[1].shape[1]
    for j in range(mu.shape[1]):
        hv1 = bohip.mom_front(np.concatenate([fr, mu[:, j:j + 1]], axis=1), ref)[1]
        assert abs(f[j] - (hv1 - hv0)) <= 4 * (nb + 8) * M * EPS * max(hv1, 1e-300), (j, f[j], hv1 - hv0)
    assert np.all(pv == 0.0) and np.all(f[-7:] == 0.0) and np.any(f > 0.1)


@pytest.mark.parametrize("M", [3, 4])
def test_partials_against_central_differences_of_the_mpmath_value(M):
    """Central differences of the 50-digit value with steps 1e-12 sigma (in mu) and 1e-12 sigma^2 (in sigma^2): the truncation is
    below 1e-20 of the scale, so the twin's partials meet them within 2 x WORST."""
    import mpmath as mp

    fr, ref, mu, var = qr.crafted(M, 5, 40, seed=5)
    dec = qr.boxes(fr, ref)
    f, pm, pv = qr.ehvi(fr, ref, mu, var)
    K = qr.keys(M)
    worst = {k: 0.0 for k in K[1:]}
    with mp.workdps(50):
        for j in range(12, 40, 5):
            _, scales = qr.mp_ehvi(fr, ref, mu[:, j], var[:, j], decomposition=dec)
            for m in range(M):
                for what, got, key in (("mu", pm[m, j], f"dmu{m + 1}"), ("var", pv[m, j], f"dvar{m + 1}")):
                    h = mp.mpf("1e-12") * (mp.sqrt(mp.mpf(var[m, j])) if what == "mu" else mp.mpf(var[m, j]))
                    vals = []
                    for sgn in (1, -1):
                        a, b = [mp.mpf(x) for x in mu[:, j]], [mp.mpf(x) for x in var[:, j]]
                        (a if what == "mu" else b)[m] += sgn * h
                        vals.append(qr.mp_ehvi(fr, ref, a, b, as_float=False, decomposition=dec)[0][0])
                    cd = float((vals[0] - vals[1]) / (2 * h))
                    worst[key] = max(worst[key], abs(got - cd) / (2 * qr.WORST * max(scales[K.index(key)], 1e-300)))
    print(f"M={M}: worst share of 2 x WORST against central differences {worst}")
    assert max(worst.values()) <= 1.0, worst


# ---- plumbing on duck-typed members -------------------------------------------------------------------------------------------------
def twin_model(d, M=3, ref=None, kerns=("SEArd", "Mat52Ard", "Mat32Ard", "SEArd")):
    """A ManyObjectiveGPE over Duck members whose score is mom_reference.score_mom (what the device call computes)."""
    from bohip.model import ManyObjectiveGPE, MOScore

    class TwinMOM(ManyObjectiveGPE):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.calls = []

        def _front_hv(self):
            return qr.front(self.y, self.reference_point())

        def score(self, xs, want_grad=False, want_moments=True):
            self.calls.append((np.shape(xs), want_grad))
            ref_ = self.reference_point(fix=True)
            fr, _ = qr.front(self.y, ref_)
            tw = qr.score_mom([m.gp() for m in self.objectives], fr, ref_, np.asarray(xs).T, want_grad)
            return MOScore(tw["scores"], tw["grad"].T if want_grad else None, tw["mu"], tw["var"], tw["best_val"], tw["best_idx"])

    return TwinMOM(tuple(Duck(d, kerns[m]) for m in range(M)), ref)


def test_many_objective_model_and_its_refusals():
    import bohip
    from bohip.model import ManyObjectiveGPE, MultiObjectiveGPE

    for count in (1, 5):
        with pytest.raises(ValueError, match="2 to 4 objectives"):
            ManyObjectiveGPE(tuple(Duck(2) for _ in range(count)))
    with pytest.raises(ValueError, match="two objectives"):
        MultiObjectiveGPE((Duck(2), Duck(2), Duck(2)))                           # the two-objective model still refuses three
    with pytest.raises(ValueError, match="dimension"):
        ManyObjectiveGPE((Duck(2), Duck(2), Duck(3)))
    with pytest.raises(ValueError):
        ManyObjectiveGPE((Duck(2), Duck(2), Duck(2)), ref=[0.0, 0.0, np.inf])
    with pytest.raises(ValueError):
        ManyObjectiveGPE((Duck(2), Duck(2), Duck(2)), ref=[0.0, 1.0])

    class MultiGPE(Duck):
        pass

    with pytest.raises(ValueError, match="MultiGPE"):
        ManyObjectiveGPE((Duck(2), Duck(2), MultiGPE(2)))

    class Weighted(Duck):
        weighted = True

    with pytest.raises(ValueError):
        ManyObjectiveGPE((Duck(2), Weighted(2), Duck(2)))
    m = twin_model(2)
    assert isinstance(m, MultiObjectiveGPE) and m.n_objectives == 3 and len(m.members) == 3
    a = bohip.ExpectedHypervolumeImprovement()
    lo, hi = [0.0, 0.0], [1.0, 1.0]
    kw = dict(verbosity=bohip.Silent, maxiterations=6, initializer_iterations=3)
    three = lambda x: (0.0, 0.0, 0.0)   # noqa: E731
    with pytest.raises(ValueError, match="ExpectedHypervolumeImprovement"):
        bohip.BOpt(three, m, bohip.ExpectedImprovement(), bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="batchsize"):
        bohip.BOpt(three, m, a, bohip.NoModelOptimizer(), lo, hi, batchsize=2, **kw)
    with pytest.raises(ValueError, match="MarginalGPOptimizer"):
        bohip.BOpt(three, m, a, bohip.MarginalGPOptimizer(), lo, hi, **kw)
    o = bohip.BOpt(lambda x: (0.0, 1.0), m, a, bohip.NoModelOptimizer(), lo, hi, **kw)
    with pytest.raises(ValueError, match="3 objectives"):
        bohip.boptimize_(o)                                                      # func must return three numbers
    with pytest.raises(ValueError, match="3 x n"):
        m.update_(np.zeros((2, 3)), np.zeros((2, 3)))
    assert bohip.defaultoptions(type(m), type(a)) == dict(method="LD_LBFGS", restarts=1, maxeval=1024)
    X = np.random.default_rng(0).random((2, 6))
    Y = np.array([[1.0, 3.0, 2.0, 5.0, 4.0, 2.5], [7.0] * 6, [6.0, 5.0, 4.0, 3.0, 2.0, 1.0]])
    m.update_(X, Y)
    assert m.ref is None and m.nobs == 6 and m.y.tobytes() == Y.tobytes()
    want = np.array([1.0 - 0.4, 7.0 - 1.0, 1.0 - 0.5])                          # the two-objective rule, per objective
    np.testing.assert_array_equal(m.default_ref(), want)
    f = bohip.acquisitionfunction(a, m)
    sc = f(np.random.default_rng(1).random((2, 9)))
    np.testing.assert_array_equal(m.ref, want)                                  # fixed once, at the first score
    assert sc.shape == (9,) and np.all(sc >= 0.0)
    with pytest.raises(ValueError):
        f(np.zeros(2))
    fr, hv = m.front, m.hypervolume
    assert fr.shape[0] == 3 and hv == qr.front(Y, want)[1] > 0.0
    assert [tuple(Y[:, i]) for i in m.front_indices()] == [tuple(c) for c in fr.T]


def test_acquire_max_refine_never_below_the_candidates():
    import bohip

    m = twin_model(2, ref=[-2.0, -2.0, -2.0])
    rng = np.random.default_rng(2)
    X = rng.random((2, 10))
    m.update_(X, np.stack([-((X - 0.2) ** 2).sum(0), -((X - 0.8) ** 2).sum(0), -((X - np.array([[0.2], [0.8]])) ** 2).sum(0)]))
    a = bohip.ExpectedHypervolumeImprovement()
    f0, x0 = bohip.acquire_max(a, m, [0.0, 0.0], [1.0, 1.0], dict(maxeval=64, restarts=1), np.random.default_rng(9))
    f1, x1 = bohip.acquire_max(a, m, [0.0, 0.0], [1.0, 1.0], dict(maxeval=64, restarts=1, refine=3), np.random.default_rng(9))
    assert f1 >= f0 > 0.0 and np.all(x1 >= 0.0) and np.all(x1 <= 1.0)
    assert [c[1] for c in m.calls].count(False) == 2 and m.calls[0][0] == (2, 64) and any(c[1] for c in m.calls)
    assert all(c[0] == (2, 3) for c in m.calls if c[1])                          # the ascent: one gradient call over the 3 starts per step


@pytest.mark.parametrize("sense", ["Max", "Min"])
def test_bopt_on_the_twin_with_three_objectives(sense):
    """A short loop on the twin: sense = Min flips all three objectives, every proposal is in the box, the hypervolume never
    decreases, and the result carries the observed front [3, n_front] in the caller's sense, the hypervolume and ref."""
    import bohip

    sgn = 1.0 if sense == "Max" else -1.0
    seen = []
    centres = np.array([[0.2, 0.3], [0.8, 0.7], [0.2, 0.8]])

    def func(x):
        y = tuple(-sgn * float(np.sum((np.asarray(x) - c) ** 2)) for c in centres)
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
    Yc = np.array([s[1] for s in seen]).T                                         # the caller's values [3, 10]
    assert len(seen) == 10 and np.all(X >= 0.0) and np.all(X <= 1.0)
    np.testing.assert_array_equal(m.y, sgn * Yc)                                  # every objective flipped under Min
    init = sgn * Yc[:, :5]
    lo, hi = init.min(axis=1), init.max(axis=1)
    np.testing.assert_array_equal(m.ref, lo - 0.1 * (hi - lo))                    # fixed after the initial design, by the default rule
    assert res["observed_optimum"] is None and res["model_optimum"] is None and res["observed_optimizer"] is None
    tf, thv = qr.front(sgn * Yc, m.ref)
    assert res["hypervolume"] == thv == m.hypervolume and thv > 0.0
    np.testing.assert_array_equal(res["observed_front"]["y"], sgn * tf)           # in the caller's sense
    np.testing.assert_array_equal(res["ref"], sgn * m.ref)
    fx = res["observed_front"]["x"]
    assert fx.shape == (2, tf.shape[1]) and res["observed_front"]["y"].shape[0] == 3
    for i in range(tf.shape[1]):
        assert np.allclose(func(fx[:, i]), res["observed_front"]["y"][:, i], rtol=0, atol=0)
    hvs.append(m.hypervolume)
    assert all(b >= a for a, b in zip(hvs, hvs[1:])) and hvs[-1] > hvs[0]
    assert m.calls[0] == ((2, 96), False) and any(c[1] for c in m.calls)
