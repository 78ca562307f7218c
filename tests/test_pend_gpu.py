"""GPU tests of pending evaluations (include/bohip_pend.h): bohip_gp_pending_set / _pending_info / _score_pending,
bohip_pend_values, ElasticGPE.score_pending, acquire_max_pending and BOpt.ask / tell.

An extension of the reference, whose loop evaluates one point at a time (src/BayesianOptimization.jl:185-196).  The reference here
is the definition itself, on the CPU: append the fantasised outcomes at the pending points, refit the whole model, score, average
over the fantasies (pend_reference.refit_per_fantasy).

Bounds are test_batch_gpu.compare's: values and mu 1e-6 relative + 64 eps s_f^2 sum|alpha| + 1e-12, s^2 conftest.var_tol.  EI, PI and
LogEI use tau = max y - 1, so the compared values stay off the 1 + erf tail, as there.  The arg-max must equal the twin's in EVERY
case: the inputs are chosen so that the twin's top-two relative gap is >= 1e-5 (asserted; the smallest on the CPU is printed by
the test), and no case is skipped on a tie."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pend_reference as pr   # noqa: E402
from batch_reference import gp_factory   # noqa: E402
from conftest import synth, var_tol   # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LL, LSIG, LNOISE, BETA = math.log(0.5), 0.0, -2.0, 0.0           # BASELINE recipe
S2F = math.exp(2 * LSIG)
ACQS = ("EI", "PI", "UCB", "MI", "MaxMean", "LogEI")
MIN_GAP = 1e-5
# (kernel, N, d, p, stress, S, R, seed): N = 17; 129 (the alpha row alone in the second row tile); 300 (three row tiles);
# p = 1, 2 with both columns equal, 17 with one column on an observation, 32; S = 0, 1, 3, 64, 257 (past one tile of fantasies at
# p = 32); R = 1 and 257.  The candidates lie in [0, XS_BOX]^d, where the recipe's mean is low: at tau = max y - 1 PI is then no
# 1.0 shared by many candidates, and every case has ONE winner.
XS_BOX = 0.3
CONFIGS = {
    "n17-p1-S1": ("SEArd", 17, 3, 1, None, 1, 257, 0),
    "n17-p1-S0-R1": ("SEArd", 17, 3, 1, None, 0, 1, 0),
    "n129-p2dup-S3": ("Mat52Ard", 129, 3, 2, "dup", 3, 257, 1),
    "n129-p17obs-S64": ("Mat32Iso", 129, 3, 17, "obs", 64, 257, 2),
    "n17-p32-S257": ("Mat12Iso", 17, 3, 32, None, 257, 257, 3),
    "n300-p32-S3": ("Mat12Iso", 300, 4, 32, None, 3, 257, 3),
    "n300-p17-S0": ("SEArd", 300, 4, 17, None, 0, 257, 4),
}


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def make_model(bohip, kern, X, y, capacity=None, lnoise=LNOISE, ll=LL, lsig=LSIG):
    d = X.shape[1]
    K = getattr(bohip, kern)
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(BETA), kernel=K(ll if kern.endswith("Iso") else np.full(d, ll), lsig), logNoise=lnoise,
                         capacity=capacity or len(y))
    m.append_(X.T, y)
    return m


def factory(kern, d, lnoise=LNOISE, ll=LL, lsig=LSIG):
    return gp_factory(kern, np.array([ll]) if kern.endswith("Iso") else np.full(d, ll), lsig, lnoise, BETA)


def params_of(acq, y):
    return {"EI": [float(y.max()) - 1.0], "PI": [float(y.max()) - 1.0], "LogEI": [float(y.max()) - 1.0], "UCB": [2.0], "MI": [1.0, 0.3],
            "MaxMean": []}[acq]


def normals(seed, S, p):
    """Z [max(S, 1)][p] as the library draws it: bohip_thompson_normal(seed, s, i); S = 0: zeros (the Kriging believer)."""
    from bohip import _lib

    lib = _lib.load()
    if S == 0:
        return np.zeros((1, p))
    return np.array([[lib.bohip_thompson_normal(seed, s, i) for i in range(p)] for s in range(S)])


def inputs(cfg):
    kern, N, d, p, stress, S, R, seed = CONFIGS[cfg]
    X, y, Xs = synth(N, d, R, seed)
    Xs = XS_BOX * Xs
    Xp = XS_BOX * np.random.default_rng(1000 + seed).random((p, d))
    if stress == "dup":
        Xp[1] = Xp[0]
    if stress == "obs":
        Xp[p // 2] = X[N // 2]
    return kern, X, y, Xs, Xp, S, 77 + seed


_MOMENTS = {}


def moments(cfg):
    """The refits of the definition, computed once per configuration and shared by its cases."""
    if cfg not in _MOMENTS:
        kern, X, y, Xs, Xp, S, seed = inputs(cfg)
        _MOMENTS[cfg] = pr.refit_moments(factory(kern, X.shape[1]), X, y, Xp, Xs, normals(seed, S, len(Xp)))
    return _MOMENTS[cfg]


def compare(tag, got, ref, N, s2f=S2F):
    """got: PendingScore of the device; ref: the twin's dict.  Every value, mu, s^2 and the arg-max."""
    sc, i0 = ref["score"], pr.top_two_gap(ref["score"])[0]
    gap = pr.top_two_gap(sc)[1]
    fin = np.isfinite(sc)
    with np.errstate(invalid="ignore"):
        dv = np.abs(got.scores - sc)
    bound = pr.value_bound(sc, s2f, ref["asum"])
    print(f"{tag}: ref idx {i0} gap {gap:.3g} | dev idx {got.best_idx} worst value share {np.max((dv / bound)[fin], initial=0.0):.3g} "
          f"mu {np.max(np.abs(got.mu - ref['mu']) / pr.value_bound(ref['mu'], s2f, ref['asum'])):.3g} "
          f"var {np.max(np.abs(got.var - ref['var']) / var_tol(ref['var'], N, s2f)):.3g}")
    assert gap >= MIN_GAP, (tag, gap)
    assert np.array_equal(got.scores[~fin], sc[~fin], equal_nan=True), tag
    assert np.all(dv[fin] <= bound[fin]), (tag, float(np.max((dv / bound)[fin])))
    assert np.all(np.abs(got.mu - ref["mu"]) <= pr.value_bound(ref["mu"], s2f, ref["asum"])), tag
    assert np.all(np.abs(got.var - ref["var"]) <= var_tol(ref["var"], N, s2f)), tag
    assert got.best_idx == i0, (tag, got.best_idx, i0)
    if i0 >= 0:
        assert got.best_val == got.scores[i0]


# ---- 1. values, moments and the arg-max against the definition -----------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_against_refit_per_fantasy(bohip, cfg):
    kern, X, y, Xs, Xp, S, seed = inputs(cfg)
    N, p = len(y), len(Xp)
    m = make_model(bohip, kern, X, y)
    m.set_pending(Xp.T)
    assert np.array_equal(m.pending, Xp.T)
    mom = moments(cfg)
    xq, mu_p, cov_p = m.pending_info()
    assert np.array_equal(xq, Xp.T)
    assert np.all(np.abs(mu_p - mom["mu_p"]) <= pr.value_bound(mom["mu_p"], S2F, mom["asum"]))
    assert np.all(np.abs(cov_p - mom["Sigma_p"]) <= var_tol(mom["Sigma_p"], N, S2F)) and np.array_equal(cov_p, cov_p.T)
    for acq in ACQS:
        for raise_tau in (False, True):
            ref = pr.score_refits(mom, acq, params_of(acq, y), raise_tau)
            got = m.score_pending(acq, params_of(acq, y), Xs.T, fantasies=S, seed=seed, raise_tau=raise_tau)
            compare(f"{cfg} {kern} {acq} raise={raise_tau}", got, ref, N + p)
    m.close()


def test_multi_chunk(bohip):
    """More candidates than one K*' chunk (N = 200, R = 70001: three chunks, as tests/test_limits_gpu.py reaches them)."""
    from bohip import _lib

    N, d, R, p, S, seed = 200, 3, 70001, 2, 1, 6
    X, y, Xs = synth(N, d, R, seed)
    Xp = np.random.default_rng(9).random((p, d))
    m = make_model(bohip, "SEArd", X, y)
    m.set_pending(Xp.T)
    got = m.score_pending("UCB", [2.0], Xs.T, fantasies=S, seed=seed)
    assert m.info(_lib.INFO_SCORE_LAUNCHES) > 1
    ref = pr.refit_per_fantasy(factory("SEArd", d), X, y, Xp, Xs, "UCB", [2.0], normals(seed, S, p))
    compare("multi-chunk", got, ref, N + p)
    m.close()


# ---- 2. identities on the device -------------------------------------------------------------------------------------------------
def test_empty_set_is_score_and_the_model_is_untouched(bohip):
    from bohip import _lib

    kern, X, y, Xs, Xp, S, seed = inputs("n129-p17obs-S64")
    m = make_model(bohip, kern, X, y)
    for acq in ("EI", "UCB", "LogEI"):
        sc, bv, bi = m.score(acq, params_of(acq, y), Xs.T)
        got = m.score_pending(acq, params_of(acq, y), Xs.T, fantasies=S, seed=seed, raise_tau=True)
        assert got.scores.tobytes() == sc.tobytes() and (got.best_val, got.best_idx) == (bv, bi)
        mu, var = m.predict_f(Xs.T)
        assert got.mu.tobytes() == mu.tobytes() and got.var.tobytes() == var.tobytes()
    L0, a0, n0, refits, appends = m.factor(), m.alpha(), m.nobs, m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS)
    m.set_pending(Xp.T)
    a = m.score_pending("EI", params_of("EI", y), Xs.T, fantasies=S, seed=seed, raise_tau=True)
    b = m.score_pending("EI", params_of("EI", y), Xs.T, fantasies=S, seed=seed, raise_tau=True)
    for u, v in zip(a, b):                                        # two identical calls: identical bytes
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert m.nobs == n0 and m.info(_lib.INFO_REFITS) == refits and m.info(_lib.INFO_APPENDS) == appends
    assert m.factor().tobytes() == L0.tobytes() and m.alpha().tobytes() == a0.tobytes()
    sc1 = m.score("EI", params_of("EI", y), Xs.T)                 # every other entry point ignores the set
    assert sc1[0].tobytes() == m.clear_pending().score("EI", params_of("EI", y), Xs.T)[0].tobytes()
    assert m.pending.shape == (X.shape[1], 0)
    m.close()


@pytest.mark.parametrize("cfg", ["n129-p2dup-S3", "n300-p32-S3"])
def test_one_fantasy_is_one_append_on_the_device(bohip, cfg):
    """S = 1: the score equals bohip_gp_score on a second handle after appending (Xp, y_f) in ONE call, y_f rebuilt on the host from
    pending_info and bohip_thompson_normal; the appended handle took the incremental route (its stage labels show append_W21)."""
    kern, X, y, Xs, Xp, _, seed = inputs(cfg)
    N, p = len(y), len(Xp)
    m = make_model(bohip, kern, X, y)
    m.set_pending(Xp.T)
    _, mu_p, cov_p = m.pending_info()
    yf = mu_p + np.linalg.cholesky(cov_p) @ normals(seed, 1, p)[0]
    m2 = make_model(bohip, kern, X, y, capacity=N + p)
    m2.enable_timing(True)
    m2.append_(Xp.T, yf)
    assert "append_W21" in [n for n, _ in m2.timing()]
    m2.enable_timing(False)
    for acq in ("EI", "UCB", "LogEI"):
        prm = params_of(acq, y)
        for raise_tau in (False, True):
            prm2 = [max(prm[0], float(yf.max()))] + prm[1:] if raise_tau and acq in pr.TAU_ACQS else prm
            got = m.score_pending(acq, prm, Xs.T, fantasies=1, seed=seed, raise_tau=raise_tau)
            sc, bv, bi = m2.score(acq, prm2, Xs.T)
            mu2, var2 = m2.predict_f(Xs.T)
            asum = float(np.abs(m2.alpha()).sum())
            fin = np.isfinite(sc)
            assert np.array_equal(got.scores[~fin], sc[~fin], equal_nan=True)
            assert np.all(np.abs(got.scores - sc)[fin] <= pr.value_bound(sc, S2F, asum)[fin]), (cfg, acq, raise_tau)
            assert np.all(np.abs(got.var - var2) <= var_tol(var2, N + p, S2F))
            assert pr.top_two_gap(sc)[1] >= MIN_GAP and got.best_idx == bi
    m.close(); m2.close()


def test_state_is_rebuilt_after_an_append_and_after_set_params(bohip):
    from bohip import _lib

    kern, X, y, Xs, Xp, S, seed = inputs("n129-p17obs-S64")
    N, d = X.shape
    m = make_model(bohip, kern, X[:-1], y[:-1], capacity=N)
    m.set_pending(Xp.T)
    m.score_pending("UCB", [2.0], Xs.T, fantasies=S, seed=seed)   # the state of N - 1 observations
    refits = m.info(_lib.INFO_REFITS)
    m.append_(X[-1], y[-1:])                                      # a real observation arrives: incremental, the handle stays fresh
    got = m.score_pending("UCB", [2.0], Xs.T, fantasies=S, seed=seed)
    assert m.info(_lib.INFO_REFITS) == refits
    compare("after append_", got, pr.score_refits(moments("n129-p17obs-S64"), "UCB", [2.0]), N + len(Xp))
    m.set_params_(logNoise=-1.5)                                   # stale, no fit_(): the call refits once, then rebuilds the state
    got = m.score_pending("UCB", [2.0], Xs.T, fantasies=S, seed=seed)
    assert m.info(_lib.INFO_REFITS) == refits + 1
    ref = pr.refit_per_fantasy(factory(kern, d, lnoise=-1.5), X, y, Xp, Xs, "UCB", [2.0], normals(seed, S, len(Xp)))
    compare("after set_params_", got, ref, N + len(Xp))
    fresh = make_model(bohip, kern, X, y, lnoise=-1.5)
    fresh.set_pending(Xp.T)
    ff = fresh.score_pending("UCB", [2.0], Xs.T, fantasies=S, seed=seed)
    assert np.all(np.abs(ff.scores - got.scores) <= pr.value_bound(ff.scores, S2F, ref["asum"])) and ff.best_idx == got.best_idx
    m.close(); fresh.close()


def test_jittered_model_carries_the_jitter_on_sigma_p(bohip):
    """test_hardening_gpu's singular model (every position five times, s_f^2 = e^10, noise e^-50) under set_jitter(1e-3, 3): the
    result agrees with the twin at logNoise' = 1/2 log(e^(2 logNoise) + J), J what the refit added."""
    from bohip import _lib

    rng = np.random.default_rng(11)
    pos = rng.random((60, 2)) * 10 - 5
    X = np.repeat(pos, 5, axis=0)
    y = -(((X - 1) ** 2).sum(1) + rng.standard_normal(len(X)))
    lsig, lnoise, p, S, seed = 5.0, -25.0, 3, 3, 21
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(BETA), kernel=bohip.SEArd(np.zeros(2), lsig), logNoise=lnoise, capacity=len(y))
    m.set_jitter(1e-3, 3)
    m.append_(X.T, y)
    assert m.info(_lib.INFO_JITTER_STEPS) >= 1
    s2f = math.exp(2 * lsig)
    J = 1e-3 * (s2f + math.exp(2 * lnoise)) * 10.0 ** (m.info(_lib.INFO_JITTER_STEPS) - 1)
    Xs, Xp = rng.random((257, 2)) * 10 - 5, rng.random((p, 2)) * 10 - 5
    m.set_pending(Xp.T)
    got = m.score_pending("UCB", [2.0], Xs.T, fantasies=S, seed=seed)
    tw = gp_factory("SEArd", np.zeros(2), lsig, 0.5 * math.log(math.exp(2 * lnoise) + J), BETA)
    ref = pr.refit_per_fantasy(tw, X, y, Xp, Xs, "UCB", [2.0], normals(seed, S, p))
    _, _, cov_p = m.pending_info()
    assert np.all(np.abs(cov_p - ref["Sigma_p"]) <= var_tol(ref["Sigma_p"], len(y), s2f))
    assert np.min(np.diag(cov_p)) >= 0.99 * J                      # (nu WITH the jitter is there)
    compare("jittered", got, ref, len(y) + p, s2f)
    m.close()


# ---- 3. the averaging stage on crafted inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,S", [(1, 1), (32, 1024), (32, 1), (1, 1024)])
def test_pend_values_on_crafted_inputs(bohip, p, S):
    """bohip_pend_values against bohip_acq_eval per fantasy, averaged in the stated order on the host.

    Tolerance, derived: mu_s = mu + sum_i b_i z_si is a (p + 1)-term sum, forward error <= (p + 1) eps (|mu| + sum_i |b_i z_si|)
    whatever the order or the use of fused multiply-adds; that error moves a(mu_s, s^2) by at most |da/dmu| (bohip_acq_eval's
    partial, at the twin's mu_s) times it, to first order -- doubled here for the second-order term and the partial's own change
    across the interval; adding S values and dividing costs <= S eps mean|a_s|; and 8 eps |a_s| for the functor's own rounding on
    two evaluations of the same arguments' neighbours.  LogEI: the same bound on each log-value v_s carries over to the
    log-mean-exp, whose partials with respect to the v_s are weights that sum to one, plus S eps for the sum of exponentials."""
    from bohip import _lib

    rng = np.random.default_rng(100 * p + S)
    R = 300
    mu, var = rng.standard_normal(R), rng.random(R) * 0.5 + 1e-3
    B = rng.standard_normal((R, p)) * 0.1
    var[:7] = 0.0                                                 # sigma^2 = 0 rows
    mu[7:11] = np.nan                                             # NaN rows
    B[11, 0] = np.nan
    Z = np.linspace(-10.0, 10.0, S * p).reshape(S, p) if S * p > 1 else np.array([[10.0]])
    rng.shuffle(Z.ravel())
    tau_s = 0.3 + 0.1 * rng.standard_normal(S)
    dev = make_model(bohip, "SEArd", *synth(20, 2, 1)[:2])
    MU = np.array([mu + B @ z for z in Z])                        # (S, R)
    mag = np.abs(mu)[None, :] + np.abs(Z) @ np.abs(B).T            # (S, R): |mu| + sum_i |b_i z_si|
    for acq, prm in (("EI", [0.3]), ("PI", [0.3]), ("UCB", [2.0]), ("MI", [1.0, 0.3]), ("MaxMean", []), ("LogEI", [0.3])):
        for taus in (None, tau_s):
            if taus is not None and acq not in pr.TAU_ACQS:
                continue
            each, dmu = np.empty((S, R)), np.empty((S, R))
            for s in range(S):
                ps = [float(taus[s])] + prm[1:] if taus is not None else prm
                each[s], dmu[s], _ = _lib.acq_eval(acq, ps, MU[s], var)
            ref = pr.average(acq, each)
            with np.errstate(invalid="ignore"):
                err_s = 2.0 * np.abs(dmu) * (p + 1) * EPS * mag + 8 * EPS * np.abs(each)
                if acq == "LogEI":
                    w = np.exp(each - each.max(axis=0))
                    tol = (w * np.where(np.isfinite(err_s), err_s, 0.0)).sum(axis=0) / w.sum(axis=0) + (S + 8) * EPS * (1.0 + np.abs(ref))
                else:
                    tol = err_s.mean(axis=0) + S * EPS * np.abs(each).mean(axis=0)
            sc, bv, bi = dev.pend_values(acq, prm, mu, var, B, Z, taus)
            ok = np.isfinite(ref)
            assert np.array_equal(np.isnan(sc), np.isnan(ref)) and np.all(np.isnan(sc[7:12]))
            assert np.array_equal(sc[~ok], ref[~ok], equal_nan=True), (acq, p, S)
            diff = np.abs(sc - ref)[ok]
            worst = float(np.max(np.where(diff > 0.0, diff / np.maximum(tol[ok], 1e-300), 0.0)))   # (0 <= 0 holds: sigma^2 = 0 rows)
            print(f"pend_values p={p} S={S} {acq} tau_s={'yes' if taus is not None else 'no'}: worst share of the tolerance {worst:.3g}")
            assert worst <= 1.0, (acq, p, S, worst)
            i0 = pr.top_two_gap(ref)[0]
            assert bi == int(np.argmax(np.where(np.isnan(sc), -np.inf, sc))) and bv == sc[bi]
            if pr.top_two_gap(ref)[1] >= MIN_GAP:
                assert bi == i0
    dev.close()


# ---- 4. errors: a status code and a message that names the limit --------------------------------------------------------------------
def test_errors(bohip):
    from bohip import _lib

    X, y, Xs = synth(40, 2, 16, 1)
    m = make_model(bohip, "SEArd", X, y)
    lib, dp = _lib.load(), C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    with pytest.raises(_lib.BohipError, match="BOHIP_PEND_PMAX") as e:
        m.set_pending(np.zeros((2, 33)))
    assert e.value.code == _lib.E_ARG
    assert lib.bohip_gp_pending_set(m._h, None, -1) == _lib.E_ARG and b"0..32" in lib.bohip_last_error()
    bad = np.zeros((2, 3), order="F"); bad[1, 2] = np.inf
    with pytest.raises(_lib.BohipError, match="not finite") as e:
        m.set_pending(bad)
    assert e.value.code == _lib.E_ARG and m.pending.shape[1] == 0
    m.set_pending(Xs[:3].T)
    with pytest.raises(_lib.BohipError, match="BOHIP_PEND_SMAX") as e:
        m.score_pending("UCB", [2.0], Xs.T, fantasies=1025)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.BohipError, match="0..1024") as e:
        m.score_pending("UCB", [2.0], Xs.T, fantasies=-1)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.BohipError, match="posterior draw") as e:
        m.score_pending("ThompsonDraw", [0.0], Xs.T)
    assert e.value.code == _lib.E_ARG
    xs, prm, sc = np.asfortranarray(Xs.T), np.array([2.0, 0.0]), np.empty(16)
    assert lib.bohip_gp_score_pending(m._h, _lib.ACQ["UCB"], ptr(prm), ptr(xs), 16, 4, 0, 6, ptr(sc), None, None, None) == _lib.E_ARG
    assert b"unknown flags" in lib.bohip_last_error()
    assert lib.bohip_gp_score_pending(m._h, _lib.ACQ["UCB"], ptr(prm), ptr(xs), 16, 4, 0, 1, ptr(sc), None, None, None) == _lib.OK
    empty = bohip.ElasticGPE(2, kernel=bohip.SEArd(np.full(2, LL), LSIG))
    empty.set_pending(Xs[:2].T)                                    # (the set itself needs no observations)
    with pytest.raises(_lib.BohipError, match="no observations") as e:
        empty.score_pending("UCB", [2.0], Xs.T)
    assert e.value.code == _lib.E_STATE
    # A pending covariance that is not positive definite, and no jitter is added here: two equal pending points so far from three
    # well-separated observations that K(X, Xp) underflows to 0, with nu = eps + e^-80 below half an ulp of s_f^2 = e^2.2 = 9.025...:
    # Sigma_p is [[a, a], [a, a]] in float64 and its second pivot a - fl(a / fl(sqrt a))^2 is 0 or -1 ulp for this a and its eight
    # float64 neighbours (checked on the host below), never positive.
    a = np.float64(math.exp(2 * 1.1))
    assert a + (EPS + math.exp(-80.0)) == a and not a - (a / np.sqrt(a)) ** 2 > 0
    sing = make_model(bohip, "SEArd", np.array([[0.0, 0.0], [5.0, 0.0], [0.0, 5.0]]), np.array([0.3, -0.2, 0.1]), lnoise=-40.0, lsig=1.1)
    sing.set_pending(np.full((2, 2), 100.0))
    with pytest.raises(_lib.NotPositiveDefinite, match="pending points is not positive definite") as e:
        sing.score_pending("UCB", [2.0], Xs.T)
    assert e.value.code == _lib.E_NOTPD
    sing.set_pending(Xs[:2].T)                                     # the handle works on
    assert np.all(np.isfinite(sing.score_pending("UCB", [2.0], Xs.T).scores))
    with pytest.raises(_lib.BohipError, match="BOHIP_PEND_PMAX"):
        m.pend_values("UCB", [2.0], np.zeros(4), np.ones(4), np.zeros((4, 33)), np.zeros((2, 33)))
    with pytest.raises(_lib.BohipError, match="BOHIP_PEND_SMAX"):
        m.pend_values("UCB", [2.0], np.zeros(4), np.ones(4), np.zeros((4, 2)), np.zeros((1025, 2)))
    w = bohip.ElasticGPE(2, kernel=bohip.SEArd(np.full(2, LL), LSIG), collapse=True)
    with pytest.raises(ValueError, match="collapse=True"):
        w.set_pending(Xs[:2].T)
    w2 = make_model(bohip, "SEArd", X, y, capacity=64)
    w2.append_sites_(Xs[:1].T, [0.5], [3], [0.1])
    assert lib.bohip_gp_pending_set(w2._h, ptr(xs), 2) == _lib.E_UNSUPPORTED and b"replicated sites" in lib.bohip_last_error()
    good = m.score_pending("UCB", [2.0], Xs.T, fantasies=4)        # the handle works on
    assert np.all(np.isfinite(good.scores)) and 0 <= good.best_idx < 16
    for h in (m, empty, sing, w, w2):
        h.close()


# ---- 5. the loop: ask(4) / tell in shuffled order on Branin -------------------------------------------------------------------------
def test_branin_ask_tell_regret(bohip):
    """test/branin.jl:17-38 with four evaluations in flight: regret under test_batch_gpu.test_branin_batch_regret's bar (0.05) at its
    budget (10 initial points + 47 x 4 = 198 evaluations); the outcomes come back in shuffled order, two at a time."""
    from test_bo_loop_gpu import BRANIN_MIN, branin, make_opt

    bo = bohip
    model = bo.ElasticGPE(2, mean=bo.MeanConst(-10.0), kernel=bo.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=3000)
    opt = make_opt(bo, model, bo.ExpectedImprovement(), maxiterations=10 + 4 * 47, initializer_iterations=10,
                   acquisitionoptions=dict(restarts=2, maxeval=1024, fantasies=16))
    shuffle = np.random.default_rng(8)
    X0 = opt.ask(10)
    opt.tell(X0, [branin(X0[:, j]) for j in range(10)])
    out = opt.ask(4)
    flight = [out[:, j] for j in range(4)]
    while flight:
        shuffle.shuffle(flight)
        back, flight = flight[:2], flight[2:]
        opt.tell(np.stack(back, axis=1), [branin(x) for x in back])
        if not bo.isdone(opt):
            new = opt.ask(min(2, opt.iterations.N - opt.iterations.i))
            flight += [new[:, j] for j in range(new.shape[1])]
    res = opt.result()
    regret = abs(res["observed_optimum"] - BRANIN_MIN)
    print(f"branin ask(4)/tell EI: regret {regret:.4g} after {len(model.y)} evaluations, {model.info(3)} incremental appends, "
          f"{model.info(2)} refits")
    assert len(model.y) == 198 and model.pending.shape[1] == 0
    assert regret < 0.05
