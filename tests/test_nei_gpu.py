"""GPU tests of noisy expected improvement (include/bohip_nei.h): bohip_gp_nei_prepare / _nei_fantasies / _score_nei /
_nei_info / _nei_release, bohip_nei_values, ElasticGPE.nei, NoisyExpectedImprovement through acquire_max and BOpt, MultiGPE.nei.

The reference is the header's definition in NumPy (tests/nei_reference.py, float64 twin).  Bounds: 16 x nei_reference.WORST of the
matching quantity -- the float64 twin's own distance from its extended-precision twin on these very inputs (tests/test_nei_host.py
test_tolerance_source), times what tests/test_limits_gpu.py grants over a CPU-measured twin error; for the mean-like and
variance-like quantities tests/test_pend_gpu.py's bound where that is larger.  Every comparison prints the share of its bound that
the device uses.  The arg-max record is the first arg-max of the device's own scores, and the twin's winner except in near ties
(the two best twin scores closer than twice the score bound; at most 1 case in 10: test_nei_host.test_near_ties_are_rare)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nei_reference as nr   # noqa: E402

pytestmark = pytest.mark.gpu
NAME = {"EI": "ei", "PI": "pi", "LogEI": "logei"}


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def model_of(bohip, a, capacity=None, lnoise=None, n=None):
    """An ElasticGPE on the arguments of a twin (nei_reference.spec's dict)."""
    X, y = a["X"][:n], a["y"][:n]
    K = getattr(bohip, a["kern"])
    m = bohip.ElasticGPE(X.shape[1], mean=bohip.MeanConst(a["beta"]), kernel=K(a["ll"] if a["kern"].endswith("Ard") else float(a["ll"][0]), a["lsig"]),
                         logNoise=lnoise if lnoise is not None else 0.5 * math.log(a["nu"] - nr.EPS), capacity=capacity or len(y))
    m.append_(X.T, y)
    return m


def grid_model(bohip, model, N, capacity=None):
    return model_of(bohip, nr.spec((model, N)), capacity, lnoise=nr.MODELS[model]["lnoise"])


def adhoc_reference(a, Xs, S, jitter_rel=nr.JREL, n=None, ll=None):
    """The twin's dict for a model that is not one of nei_reference's inputs (a grown or re-parameterised one)."""
    t = nr.Twin(a["kern"], a["X"][:n], a["y"][:n], a["ll"] if ll is None else ll, a["lsig"], a["nu"], a["beta"], jitter_rel)
    F, tau, alpha = t.fantasies(*nr.normals(nr.SEED, S, len(t.y)))
    m, s2 = t.moments(Xs, alpha)
    return dict(F=F, tau=tau, m=m, s2=s2, s2f=float(t.s2f), asum=float(np.abs(alpha).sum(axis=0).max()))


def labels(m):
    return [n for n, _ in m.timing()]


def check_fantasies(tag, F, tau, ref, N, assert_=True):
    b = nr.bounds(ref, N)
    sF, sT = float(np.max(np.abs(F - ref["F"]))) / b["F"], float(np.max(np.abs(tau - ref["tau"]))) / b["F"]
    print(f"{tag}: shares of the bound  F {sF:.3g}  tau {sT:.3g}")
    if assert_:
        assert sF <= 1 and sT <= 1, (tag, sF, sT)


def check_scores(tag, got, ref, R, acq, N, assert_=True):
    """got: the device's NEIScore; ref: the twin's dict (all its candidates; the first R are compared)."""
    m, s2 = ref["m"][:R], ref["s2"][:R]
    sc = nr.score(acq, m, s2, ref["tau"])[0]
    b = nr.bounds(dict(ref, m=m.mean(axis=1), s2=s2), N)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(sc)
        same_inf = np.array_equal(got.score[~fin], sc[~fin], equal_nan=True)
    s_sc = float(np.max(nr.score_distance(acq, got.score, sc, ref["s2f"]), initial=0.0)) / b[acq]
    s_mu = float(np.max(np.abs(got.mu - m.mean(axis=1)) / b["m"]))
    s_var = float(np.max(np.abs(got.var - s2) / b["s2"]))
    s_tau = float(np.max(np.abs(got.tau - ref["tau"]))) / b["F"]
    i0 = nr.top_two(sc)[0]
    tie = nr.near_tie(acq, sc, ref["s2f"])
    print(f"{tag} {acq}: shares of the bound  score {s_sc:.3g}  mean {s_mu:.3g}  s^2 {s_var:.3g}  tau {s_tau:.3g} | twin idx {i0}"
          f"{' (near tie)' if tie else ''} dev idx {got.best[1]}")
    i_dev = nr.top_two(got.score)[0]
    assert got.best[1] == i_dev and (i_dev < 0 or got.best[0] == got.score[i_dev]), (tag, got.best, i_dev)   # the device's own first arg-max
    if assert_:
        assert same_inf, tag
        assert s_sc <= 1 and s_mu <= 1 and s_var <= 1 and s_tau <= 1, (tag, acq, s_sc, s_mu, s_var, s_tau)
        assert tie or got.best[1] == i0, (tag, acq, got.best, i0)
    return s_sc


def expected_route(N, R):
    if N + 1 > 7 * 128:                                           # split-K applies from eight row tiles on
        return "small_V" if R <= min(256, max(16, (20 + 260000 // N) // 16 * 16)) else "split_V"
    return "small_V" if R <= min(256, 90 + 300000 // N) else "trigemm_sq"


# ---- 0. the ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_is_present(bohip):
    from bohip import _lib

    lib = C.CDLL(_lib.LIB_PATH)
    for name in _lib.NEI_SIGNATURES:
        assert hasattr(lib, name), name
    assert len(_lib.NEI_SIGNATURES) == 6 and hasattr(bohip.ElasticGPE, "nei") and hasattr(bohip, "NoisyExpectedImprovement")


# ---- 1. fantasies ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(nr.MODELS))
@pytest.mark.parametrize("N", nr.NS)
def test_fantasies(bohip, model, N):
    m = grid_model(bohip, model, N)
    got = {}
    for S in nr.SS:
        F, tau = m.nei_fantasies(S=S, seed=nr.SEED, jitter_rel=nr.JREL)
        assert F.shape == (max(S, 1), N) and tau.shape == (max(S, 1),)
        check_fantasies(f"{model} N={N} S={S}", F, tau, nr.reference((model, N), S), N)
        assert np.array_equal(tau, F.max(axis=1))
        got[S] = (F, tau)
    assert got[64][0][:5].tobytes() == got[5][0].tobytes() and got[64][1][:5].tobytes() == got[5][1].tobytes()   # s-prefixes are identical
    assert got[5][0][:1].tobytes() == got[1][0].tobytes()
    steps = None
    for S in (0, 64):                                             # the default jitter_rel once per shape: printed, not bounded
        F, tau = m.nei_fantasies(S=S, seed=nr.SEED)
        steps = m.nei_info(bohip._lib.NEI_INFO_JITTER_STEPS)
        ref = nr.reference((model, N), S, jitter_rel=nr.JREL_DEFAULT * 10 ** steps)
        check_fantasies(f"{model} N={N} S={S} jitter_rel=1e-8 (delta steps {steps})", F, tau, ref, N, assert_=False)
        assert np.all(np.isfinite(F))
    m.close()


# ---- 2. scores -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(nr.MODELS))
@pytest.mark.parametrize("N", nr.NS)
@pytest.mark.parametrize("R", nr.RS)
def test_scores(bohip, model, N, R):
    m = grid_model(bohip, model, N)
    Xs = nr.data(model, N, R)[2]
    m.enable_timing(True)
    for S in nr.SS:
        ref = nr.reference((model, N), S)
        for acq in nr.ACQS:
            got = m.nei(Xs.T, S=S, seed=nr.SEED, acq=NAME[acq], jitter_rel=nr.JREL)
            lab = labels(m)
            assert expected_route(N, R) in lab and "nei_means" in lab and "nei_reduce" in lab, (lab, expected_route(N, R))
            check_scores(f"{model} N={N} R={R} S={S}", got, ref, R, acq, N)
    m.enable_timing(False)
    for S in (0, 64):                                             # the default jitter_rel once per shape: printed, not bounded
        got = m.nei(Xs.T, S=S, seed=nr.SEED, acq="ei")
        steps = m.nei_info(bohip._lib.NEI_INFO_JITTER_STEPS)
        ref = nr.reference((model, N), S, jitter_rel=nr.JREL_DEFAULT * 10 ** steps)
        check_scores(f"{model} N={N} R={R} S={S} jitter_rel=1e-8 (delta steps {steps})", got, ref, R, "EI", N, assert_=False)
    m.close()


def test_chunk_boundary(bohip):
    """One candidate past the chunk cap at N = 17 (65536): several K*' chunks; the candidates on both sides of every boundary and the last one."""
    N, R, S = nr.CHUNK_N, nr.CHUNK_R, nr.CHUNK_S
    tag = ("se3", N, R)
    m = model_of(bohip, nr.spec(tag), lnoise=nr.MODELS["se3"]["lnoise"])
    ref = nr.reference(tag, S)
    m.enable_timing(True)
    got = m.nei(nr.spec(tag)["Xs"].T, S=S, seed=nr.SEED, acq="ei", jitter_rel=nr.JREL)
    lab = labels(m)
    chunks = lab.count("trigemm_sq")
    assert chunks >= 2 and lab.count("nei_means") == chunks and lab.count("nei_reduce") == chunks, lab
    check_scores("chunk boundary", got, ref, R, "EI", N)
    R512 = (R + 511) // 512 * 512
    chunk = ((R512 + chunks - 1) // chunks + 511) // 512 * 512    # equal-sized multiples of 512 candidates
    sc = nr.score("EI", ref["m"], ref["s2"], ref["tau"])[0]
    b = nr.bounds(ref, N)
    for j in [c * chunk + o for c in range(1, chunks) for o in (-1, 0)] + [R - 1]:
        assert abs(got.score[j] - sc[j]) <= b["EI"] and abs(got.var[j] - ref["s2"][j]) <= b["s2"][j], j
    print(f"chunk boundary: {chunks} chunks of {chunk} candidates")
    m.close()


def test_nine_row_tiles_small_and_split(bohip):
    """N = 1100.  R = 200 lies below the small-batch limit of that size (256), so the companion's variance pass is the small route;
    R = 300 takes split-K."""
    N, S = nr.BIG_N, nr.BIG_S
    tag = ("se3", N, max(nr.BIG_RS))
    m = model_of(bohip, nr.spec(tag), lnoise=nr.MODELS["se3"]["lnoise"])
    ref = nr.reference(tag, S)
    m.enable_timing(True)
    for R in nr.BIG_RS:
        for acq in nr.ACQS:
            got = m.nei(nr.spec(tag)["Xs"][:R].T, S=S, seed=nr.SEED, acq=NAME[acq], jitter_rel=nr.JREL)
            lab = labels(m)
            assert expected_route(N, R) in lab, lab
            check_scores(f"se3 N={N} R={R} S={S} [{expected_route(N, R)}]", got, ref, R, acq, N)
    assert expected_route(N, 300) == "split_V" and expected_route(N, 200) == "small_V"
    m.close()


def test_s_tile_edges(bohip):
    N, R = 129, 40
    m = grid_model(bohip, "se3", N)
    Xs = nr.data("se3", N, R)[2]
    for S in nr.S_EDGES:
        for acq in nr.ACQS:
            check_scores(f"se3 N={N} R={R} S={S}", m.nei(Xs.T, S=S, seed=nr.SEED, acq=NAME[acq], jitter_rel=nr.JREL),
                         nr.reference(("se3", N), S), R, acq, N)
    m.close()


# ---- 3. determinism and slicing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,R", [(129, 40), (300, 700)])
def test_determinism_and_slicing(bohip, N, R):
    m = grid_model(bohip, "se3", N)
    Xs = nr.data("se3", N, R)[2]
    a = m.nei(Xs.T, S=5, seed=nr.SEED, acq="logei", jitter_rel=nr.JREL)
    b = m.nei(Xs.T, S=5, seed=nr.SEED, acq="logei", jitter_rel=nr.JREL)
    for u, v in zip((a.score, a.mu, a.var, a.tau), (b.score, b.mu, b.var, b.tau)):
        assert u.tobytes() == v.tobytes()
    assert a.best == b.best
    m.set_batch_hint(R)
    h = R // 2
    lo = m.nei(Xs[:h].T, S=5, seed=nr.SEED, acq="logei", jitter_rel=nr.JREL)
    hi = m.nei(Xs[h:].T, S=5, seed=nr.SEED, acq="logei", jitter_rel=nr.JREL)
    m.set_batch_hint(0)
    for name in ("score", "mu", "var"):
        assert np.concatenate([getattr(lo, name), getattr(hi, name)]).tobytes() == getattr(a, name).tobytes(), name
    m.close()


# ---- 4. the life cycle -------------------------------------------------------------------------------------------------------------------
def _counts(m):
    from bohip import _lib

    return (m.nei_info(_lib.NEI_INFO_REFITS), m.nei_info(_lib.NEI_INFO_APPENDS), m.nei_info(_lib.NEI_INFO_REBUILDS), m.info(_lib.INFO_REFITS))


def test_life_cycle(bohip):
    from bohip import _lib

    a = nr.spec(("se3", 300))
    Xs, S, R = a["Xs"][:40], 5, 40
    lnoise = nr.MODELS["se3"]["lnoise"]
    m = model_of(bohip, a, capacity=256, lnoise=lnoise, n=100)
    assert _counts(m)[:3] == (0, 0, 0) and m.nei_info(_lib.NEI_INFO_BYTES) == 0      # nothing before the first call
    r0 = m.info(_lib.INFO_REFITS)
    g1 = m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)
    assert _counts(m) == (1, 0, 1, r0) and m.nei_info(_lib.NEI_INFO_BYTES) > 0          # first call: one companion refit
    g2 = m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)
    assert _counts(m) == (1, 0, 1, r0) and g2.score.tobytes() == g1.score.tobytes()      # second call: nothing
    check_scores("life cycle n=100", g1, adhoc_reference(a, Xs, S, n=100), R, "EI", 100)
    m.append_(a["X"][100:101].T, a["y"][100:101])                                        # one row: one incremental companion append
    g3 = m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)
    assert _counts(m) == (1, 1, 2, r0)
    ref101 = adhoc_reference(a, Xs, S, n=101)
    check_scores("life cycle n=101 (appended)", g3, ref101, R, "EI", 101)
    fresh = model_of(bohip, a, capacity=256, lnoise=lnoise, n=101)
    check_scores("life cycle n=101 (fresh handle)", fresh.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL), ref101, R, "EI", 101)
    fresh.close()
    m.append_(a["X"][101:134].T, a["y"][101:134])                                        # 33 rows: a companion refit
    g4 = m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)
    c = _counts(m)
    assert c[:3] == (2, 1, 3), c
    check_scores("life cycle n=134 (33 appended)", g4, adhoc_reference(a, Xs, S, n=134), R, "EI", 134)
    r1 = m.info(_lib.INFO_REFITS)
    ll2 = a["ll"] + 0.1
    m.set_params_(ll=ll2)                                                                # no fit_(): both stale, the call refits both
    g5 = m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)
    assert _counts(m) == (3, 1, 4, r1 + 1)
    check_scores("life cycle after set_params_", g5, adhoc_reference(a, Xs, S, n=134, ll=ll2), R, "EI", 134)
    m.nei_release()
    assert _counts(m)[:3] == (0, 0, 0) and m.nei_info(_lib.NEI_INFO_BYTES) == 0
    g6 = m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)                              # after the release: the same bytes
    for name in ("score", "mu", "var", "tau"):
        assert getattr(g6, name).tobytes() == getattr(g5, name).tobytes(), name
    assert g6.best == g5.best and _counts(m)[:3] == (1, 0, 1)
    m.close()


def test_capacity_growth(bohip):
    """Capacity 100 -> 200 across a call sequence: rows arrive 25 at a time with a call after each."""
    from bohip import _lib

    a = nr.spec(("se3", 300))
    Xs, S, R = a["Xs"][:40], 5, 40
    m = model_of(bohip, a, capacity=100, lnoise=nr.MODELS["se3"]["lnoise"], n=100)
    m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)
    for n0 in range(100, 200, 25):
        m.append_(a["X"][n0:n0 + 25].T, a["y"][n0:n0 + 25])
        got = m.nei(Xs.T, S=S, seed=nr.SEED, jitter_rel=nr.JREL)
    assert m.info(_lib.INFO_CAPACITY) >= 200 and m.nei_info(_lib.NEI_INFO_APPENDS) >= 1
    check_scores("capacity growth n=200", got, adhoc_reference(a, Xs, S, n=200), R, "EI", 200)
    m.close()


# ---- 5. weighted and jittered handles ---------------------------------------------------------------------------------------------------
def test_weighted_handle(bohip):
    x_raw, y_raw, X, ybar, reps, Xs = nr.weighted_data()
    p = nr.MODELS["se3"]
    m = bohip.ElasticGPE.from_data(x_raw, y_raw, mean=bohip.MeanConst(p["beta"]), kernel=bohip.SEArd(nr.model_ll("se3"), p["lsig"]),
                                   logNoise=p["lnoise"], collapse=True)
    assert m.weighted and np.array_equal(m.reps, reps) and np.array_equal(m.x, X.T)
    ref = nr.reference("weighted", 5)
    F, tau = m.nei_fantasies(S=5, seed=nr.SEED, jitter_rel=nr.JREL)
    check_fantasies("weighted", F, tau, ref, 40)
    for acq in nr.ACQS:
        check_scores("weighted", m.nei(Xs.T, S=5, seed=nr.SEED, acq=NAME[acq], jitter_rel=nr.JREL), ref, len(Xs), acq, 40)
    m.close()


def test_jittered_handle(bohip):
    """tests/test_hardening_gpu.py's singular model under set_jitter(1e-3, 3): D carries the last refit's jitter."""
    from bohip import _lib

    X, y, Xs, J = nr.jitter_data()
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(nr.JIT_LL, nr.JIT_LSIG), logNoise=nr.JIT_LNOISE, capacity=len(y) + 8)
    m.set_jitter(nr.JIT_REL, 3)
    m.append_(X.T, y)
    assert m.info(_lib.INFO_JITTER_STEPS) == 1
    ref, wrong = nr.reference("jitter", 5), nr.reference("jitter-ignored", 5)
    F, tau = m.nei_fantasies(S=5, seed=nr.SEED, jitter_rel=nr.JREL)
    assert m.nei_info(_lib.NEI_INFO_JITTER_STEPS) == 0
    check_fantasies("jittered", F, tau, ref, len(y))
    far = float(np.max(np.abs(F - wrong["F"]))) / nr.bounds(ref, len(y))["F"]
    print(f"jittered: a twin whose D lacks the jitter is {far:.3g} bounds from the device")
    assert far > 100
    for acq in nr.ACQS:
        check_scores("jittered", m.nei(Xs.T, S=5, seed=nr.SEED, acq=NAME[acq], jitter_rel=nr.JREL), ref, len(Xs), acq, len(y))
    m.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable(bohip):
    from bohip import _lib

    lib = _lib.load()
    N, R = 17, 40
    m = grid_model(bohip, "se3", N)
    Xs = np.ascontiguousarray(nr.data("se3", N, R)[2])
    ref = nr.reference(("se3", N), 5)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    sc, prm = np.empty(R), np.zeros(2)

    def call(acq_id, S=5, jrel=nr.JREL, h=None):
        return lib.bohip_gp_score_nei(h or m._h, acq_id, ptr(prm), ptr(Xs), R, S, nr.SEED, jrel, ptr(sc), None, None, None)

    def still_fine():
        check_scores("after an error", m.nei(Xs.T, S=5, seed=nr.SEED, jitter_rel=nr.JREL), ref, R, "EI", N)

    for acq in ("UCB", "MI", "MaxMean", "ThompsonDraw"):
        assert call(_lib.ACQ[acq]) == _lib.E_ARG, acq
        still_fine()
    assert call(_lib.ACQ["EI"], S=1025) == _lib.E_ARG
    still_fine()
    assert call(_lib.ACQ["EI"], S=-1) == _lib.E_ARG
    for bad in (0.0, -1e-6, math.inf, math.nan):
        assert call(_lib.ACQ["EI"], jrel=bad) == _lib.E_ARG, bad
    still_fine()
    assert lib.bohip_gp_nei_fantasies(m._h, 0.0, 5, 0, None, None) == _lib.E_ARG
    assert lib.bohip_gp_nei_prepare(m._h, nr.JREL, 1025, 0) == _lib.E_ARG
    empty = bohip.ElasticGPE(3, kernel=bohip.SEArd(np.zeros(3), 0.0))
    assert call(_lib.ACQ["EI"], h=empty._h) == _lib.E_STATE
    assert lib.bohip_gp_nei_prepare(empty._h, nr.JREL, 5, 0) == _lib.E_STATE
    empty.close()
    still_fine()
    m.close()


# ---- 7. no side effects -----------------------------------------------------------------------------------------------------------------
def test_no_side_effects_on_the_other_entry_points(bohip):
    N, R = 129, 40
    Xs = nr.data("se3", N, R)[2]
    Xp = np.random.default_rng(3).random((3, 4))                  # four pending points, d x p
    used, clean = grid_model(bohip, "se3", N), grid_model(bohip, "se3", N)
    used.nei(Xs.T, S=5, seed=nr.SEED, jitter_rel=nr.JREL)
    tau = [float(nr.data("se3", N)[1].max())]
    for m in (used, clean):
        m.set_pending(Xp)

    def everything(m):
        sc, bv, bi = m.score("EI", tau, Xs.T)
        sg, g = m.score_grad("EI", tau, Xs.T)
        mu, var = m.predict_f(Xs.T)
        ps = m.score_pending("EI", tau, Xs.T, fantasies=4, seed=9, raise_tau=True)
        return [sc, np.array([bv, bi]), sg, g, mu, var, ps.scores, ps.mu, ps.var, np.array([ps.best_val, ps.best_idx]), m.factor(), m.alpha()]

    for u, v in zip(everything(used), everything(clean)):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    used.nei(Xs.T, S=64, seed=1, acq="logei", jitter_rel=nr.JREL)  # and again with a call in between
    for u, v in zip(everything(used), everything(clean)):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    used.close()
    clean.close()


# ---- 8. the averaging stage and the host layers --------------------------------------------------------------------------------------
def test_nei_values_is_the_score_calls_last_stage(bohip):
    N, R, S = 129, 300, 5
    m = grid_model(bohip, "se3", N)
    ref = nr.reference(("se3", N), S)
    for acq in nr.ACQS:
        sc, mm, bv, bi = m.nei_values(NAME[acq], ref["m"][:R], ref["s2"][:R], ref["tau"])
        twin = nr.score(acq, ref["m"][:R], ref["s2"][:R], ref["tau"])[0]
        fin = np.isfinite(twin)
        assert np.array_equal(sc[~fin], twin[~fin]) and np.all(np.abs(sc - twin)[fin] <= 1e-12 * np.maximum(1.0, np.abs(twin[fin])))
        assert np.max(np.abs(mm - ref["m"][:R].mean(axis=1))) <= 1e-13 and bi == nr.top_two(sc)[0] and bv == sc[bi]
    m.close()


def test_host_layers(bohip):
    N, d = 129, 3
    m = grid_model(bohip, "se3", N)
    a = bohip.NoisyExpectedImprovement(S=8, seed=4, jitter_rel=nr.JREL)
    lb, ub = np.zeros(d), np.ones(d)
    opts = dict(restarts=1, maxeval=512)
    f, x = bohip.acquire_max(a, m, lb, ub, opts, rng=np.random.default_rng(5))
    xs = bohip.latin_hypercube_sampling(lb, ub, 512, np.random.default_rng(5))
    direct = m.nei(xs, S=8, seed=4, acq="ei", jitter_rel=nr.JREL)
    assert direct.best[1] >= 0 and np.array_equal(x, xs[:, direct.best[1]]) and f == direct.best[0]
    fn = bohip.acquisitionfunction(a, m)
    assert fn(xs).tobytes() == direct.score.tobytes() and fn(xs[:, 7]) == direct.score[7]
    m.close()


def test_multigpe_runs_it_on_the_first_replica(bohip):
    N, d = 129, 3
    m = grid_model(bohip, "se3", N)
    xs = nr.data("se3", N, 40)[2].T
    direct = m.nei(xs, S=8, seed=4, acq="ei", jitter_rel=nr.JREL)
    mg = bohip.MultiGPE(d, devices=(0,), mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(nr.model_ll("se3"), 0.0),
                        logNoise=nr.MODELS["se3"]["lnoise"], capacity=N)
    X, y, _ = nr.data("se3", N)
    mg.append_(X.T, y)
    other = mg.nei(xs, S=8, seed=4, acq="ei", jitter_rel=nr.JREL)
    for name in ("score", "mu", "var", "tau"):
        assert getattr(other, name).tobytes() == getattr(direct, name).tobytes(), name
    assert other.best == direct.best
    Fm, _ = mg.nei_fantasies(S=8, seed=4, jitter_rel=nr.JREL)
    assert Fm.tobytes() == m.nei_fantasies(S=8, seed=4, jitter_rel=nr.JREL)[0].tobytes()
    mg.close()
    m.close()


def test_bopt_runs_under_noisy_expected_improvement(bohip):
    rng = np.random.default_rng(2)
    f = lambda x: -float((x[0] - 0.3) ** 2) + 0.1 * float(rng.standard_normal())   # noqa: E731
    model = bohip.ElasticGPE(1, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.array([-1.0]), 0.0), logNoise=-2.0, capacity=16)
    o = bohip.BOpt(f, model, bohip.NoisyExpectedImprovement(S=8, seed=1), bohip.NoModelOptimizer(), [-1.0], [1.0], maxiterations=6,
                   initializer_iterations=3, verbosity=bohip.Silent, acquisitionoptions=dict(restarts=1, maxeval=128),
                   rng=np.random.default_rng(0))
    res = bohip.boptimize_(o)
    assert model.nobs == 6 and res["observed_optimum"] == model.y.max()
    mu, _ = model.predict_f(model.x)
    j = int(np.argmax(mu))
    assert res["model_optimum"] == mu[j] and np.array_equal(res["model_optimizer"], model.x[:, j])
    model.close()
