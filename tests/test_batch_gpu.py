"""GPU tests of greedy batch selection (bohip_gp_select_batch, ElasticGPE.select_batch, acquire_batch, BOpt(batchsize=...)).

An extension of the reference, whose iteration proposes ONE point (src/BayesianOptimization.jl:185-196).  The reference here is
the definition itself, on the CPU: append the fantasised observation, refit the whole model, score again (batch_reference.py).

Tolerances are those of test_parity_gpu.py for the same quantities: value and mu 1e-6 relative + mu_floor (+ 1e-12), sigma^2
conftest.var_tol.  Indices are exact under a guard computed from the reference: a round whose top-two relative gap is below 1e-7
ends that case's comparison (later rounds would be conditioned on a legitimately different pick); none of the cases below may end
early (their smallest gap on the CPU is 1.7e-5)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_reference import gp_factory, masked_argmax, refit_per_pick   # noqa: E402
from conftest import synth, var_tol   # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LL, LSIG, LNOISE, BETA = math.log(0.5), 0.0, -2.0, 0.0           # BASELINE recipe
CONFIGS = {"n500": (500, 4, 2048, 8, 3), "n1000": (1000, 8, 4096, 8, 0)}   # (N, d, R, q, seed)
GAP_GUARD = 1e-7


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def make_model(bohip, kern, X, y, capacity=None):
    d = X.shape[1]
    K = getattr(bohip, kern)
    ll = LL if kern.endswith("Iso") else np.full(d, LL)
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(BETA), kernel=K(ll, LSIG), logNoise=LNOISE, capacity=capacity or len(y))
    m.append_(X.T, y)
    return m


def factory(kern, d):
    return gp_factory(kern, np.array([LL]) if kern.endswith("Iso") else np.full(d, LL), LSIG, LNOISE, BETA)


def acq_params(acq, y, tau_shift=0.0):
    return {"EI": [float(y.max()) - tau_shift], "PI": [float(y.max()) - tau_shift], "UCB": [2.0], "MI": [1.0, 0.3]}[acq]


def fantasy_of(name, y):
    return {"believer": "believer", "max": float(y.max()), "min": float(y.min())}[name]


def compare(tag, got, ref, N, rounds=None, may_end_early=False):
    """got = (idx, val, mu, var) of the device, ref = rows of refit_per_pick.  Returns the number of rounds compared."""
    idx, val, mu, var = got
    s2f = math.exp(2 * LSIG)
    n = 0
    for t, (i0, v0, mu0, var0, gap0, asum) in enumerate(ref[:rounds]):
        print(f"{tag} round {t}: ref idx {i0} val {v0:.12g} gap {gap0:.3g} | dev idx {idx[t]} dval {abs(val[t] - v0):.3g} "
              f"dmu {abs(mu[t] - mu0):.3g} dvar {abs(var[t] - var0):.3g}")
        if gap0 < GAP_GUARD:
            assert may_end_early, f"{tag}: the reference's top two of round {t} are {gap0:.3g} apart"
            break
        fl = 64 * EPS * s2f * asum
        assert idx[t] == i0, (tag, t, idx[t], i0)
        assert abs(val[t] - v0) <= 1e-6 * abs(v0) + fl + 1e-12, (tag, t, val[t], v0)
        assert abs(mu[t] - mu0) <= 1e-6 * abs(mu0) + fl + 1e-12, (tag, t, mu[t], mu0)
        assert abs(var[t] - var0) <= var_tol(np.array(var0), N, s2f), (tag, t, var[t], var0)
        n += 1
    return n


# ---- 1. picks and values against the refit-per-pick reference -------------------------------------------------------------
_CASES = [(acq, f, 0.0, False) for acq in ("UCB", "MI") for f in ("believer", "max", "min")] + \
         [("EI", "believer", 0.0, False), ("EI", "max", 0.0, False),   # (EI with liar = min falls into the 1 + erf tail: left out)
          ("EI", "believer", 1.0, True), ("EI", "max", 1.0, True)]   # (the EI values compared are >= 0.089: far from that tail)


@pytest.mark.parametrize("kern", ["SEArd", "Mat52Ard"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_against_refit_per_pick(bohip, cfg, kern):
    N, d, R, q, seed = CONFIGS[cfg]
    X, y, Xs = synth(N, d, R, seed)
    m = make_model(bohip, kern, X, y)
    for acq, fname, shift, raise_tau in _CASES:
        p, fv = acq_params(acq, y, shift), fantasy_of(fname, y)
        ref = refit_per_pick(factory(kern, d), X, y, Xs, acq, p, q, fv, raise_tau)
        got = m.select_batch(acq, p, Xs.T, q, fantasy=fv, raise_tau=raise_tau)
        tag = f"{cfg} {kern} {acq} {fname} tau-{shift} raise={raise_tau}"
        assert compare(tag, got, ref, N) == q
    m.close()


@pytest.mark.parametrize("kern,acq,fname", [("Mat32Ard", "UCB", "believer"), ("Mat32Ard", "MI", "max"), ("Mat52Iso", "UCB", "min"),
                                            ("Mat12Iso", "MI", "believer")])
def test_other_kernels_against_refit_per_pick(bohip, kern, acq, fname):
    """Matérn 3/2, 1/2 and iso kernels through matern_reference.MaternGP."""
    N, d, R, q, seed = CONFIGS["n500"]
    X, y, Xs = synth(N, d, R, seed)
    m = make_model(bohip, kern, X, y)
    p, fv = acq_params(acq, y), fantasy_of(fname, y)
    ref = refit_per_pick(factory(kern, d), X, y, Xs, acq, p, q, fv)
    got = m.select_batch(acq, p, Xs.T, q, fantasy=fv)
    assert compare(f"{kern} {acq} {fname}", got, ref, N, may_end_early=True) >= 1
    m.close()


def test_pi_first_round(bohip):
    """PI saturates at 1.0 and ties once tau lies well below max y, so only its first round at tau = max y is compared."""
    N, d, R, q, seed = CONFIGS["n500"]
    X, y, Xs = synth(N, d, R, seed)
    m = make_model(bohip, "SEArd", X, y)
    p = acq_params("PI", y)
    ref = refit_per_pick(factory("SEArd", d), X, y, Xs, "PI", p, 1)
    got = m.select_batch("PI", p, Xs.T, 4)
    assert compare("PI", got, ref, N, rounds=1, may_end_early=True) <= 1
    assert len(set(got[0].tolist())) == 4
    m.close()


# ---- 2. q = 1, reproducibility, distinct picks, a permutation ---------------------------------------------------------------
def test_q1_reproducible_distinct_permutation(bohip):
    N, d, R, q, seed = CONFIGS["n1000"]
    X, y, Xs = synth(N, d, R, seed)
    m = make_model(bohip, "SEArd", X, y)
    for acq in ("EI", "UCB", "MI", "PI", "MaxMean"):
        p = acq_params(acq, y) if acq != "MaxMean" else []
        _, bv, bi = m.score(acq, p, Xs.T, want_scores=False)
        idx, val, mu, var = m.select_batch(acq, p, Xs.T, 1)
        assert idx[0] == bi and val[0].tobytes() == np.float64(bv).tobytes(), (acq, idx, bi, val, bv)
        mu_p, var_p = m.predict_f(Xs[bi])
        assert mu[0] == mu_p[0] and var[0] == var_p[0]
    for acq, fv in (("EI", "believer"), ("UCB", float(y.max()))):
        a = m.select_batch(acq, acq_params(acq, y), Xs.T, q, fantasy=fv)
        b = m.select_batch(acq, acq_params(acq, y), Xs.T, q, fantasy=fv)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
        assert len(set(a[0].tolist())) == q and a[0].min() >= 0 and a[0].max() < R
        assert np.all(np.isfinite(a[1])) and np.all(a[3] >= 0.0)
    idx, val, _, _ = m.select_batch("UCB", [2.0], Xs[:10].T, 10)
    assert sorted(idx.tolist()) == list(range(10)) and np.all(np.isfinite(val))
    m.close()


def test_fewer_winners_than_q(bohip):
    """Candidates whose score is NaN can never win: the rest of the batch is idx = -1, val = -Inf."""
    N, d, R, q, seed = 60, 2, 6, 6, 1
    X, y, Xs = synth(N, d, R, seed)
    Xs[2:] = np.nan
    m = make_model(bohip, "SEArd", X, y)
    idx, val, mu, var = m.select_batch("UCB", [2.0], Xs.T, q)
    assert sorted(idx[:2].tolist()) == [0, 1] and np.all(idx[2:] == -1)
    assert np.all(np.isfinite(val[:2])) and np.all(val[2:] == -np.inf)
    m.close()


# ---- 3. the model is untouched ---------------------------------------------------------------------------------------------
def test_model_untouched(bohip):
    N, d, R, q, seed = CONFIGS["n500"]
    X, y, Xs = synth(N, d, R, seed)
    m = make_model(bohip, "Mat52Ard", X, y)
    L0, a0, n0 = m.factor(), m.alpha(), m.nobs
    sc0 = m.score("EI", [float(y.max())], Xs.T)
    refits, appends = m.info(2), m.info(3)
    m.select_batch("EI", [float(y.max())], Xs.T, q, fantasy=float(y.max()), raise_tau=True)
    assert m.nobs == n0 and m.info(2) == refits and m.info(3) == appends
    assert m.factor().tobytes() == L0.tobytes() and m.alpha().tobytes() == a0.tobytes()
    sc1 = m.score("EI", [float(y.max())], Xs.T)
    assert sc1[0].tobytes() == sc0[0].tobytes() and sc1[1:] == sc0[1:]
    m.close()


# ---- 4. more candidates than one K*' chunk -----------------------------------------------------------------------------------
def test_multi_chunk(bohip):
    """N = 3000, d = 8, R = 16384, q = 4, EI, believer.  CPU reference (seed 0, tau = max y): picks 7817, 1335, 5122, 15016 --
    both halves of the candidate set -- smallest gap 1.6e-2."""
    from bohip import _lib

    N, d, R, q, seed = 3000, 8, 16384, 4, 0
    X, y, Xs = synth(N, d, R, seed)
    m = make_model(bohip, "SEArd", X, y)
    p = [float(y.max())]
    got = m.select_batch("EI", p, Xs.T, q)
    assert m.info(_lib.INFO_SCORE_LAUNCHES) > 1
    ref = refit_per_pick(factory("SEArd", d), X, y, Xs, "EI", p, q)
    assert compare("multi-chunk", got, ref, N) == q
    assert [r[0] for r in ref] == [7817, 1335, 5122, 15016]
    m.close()


# ---- 5. the equivalence the feature claims, on the device alone --------------------------------------------------------------
@pytest.mark.parametrize("acq,fname", [("UCB", "believer"), ("EI", "max"), ("MI", "min")])
def test_equals_score_append_loop_on_device(bohip, acq, fname):
    N, d, R, q, seed = CONFIGS["n500"]
    X, y, Xs = synth(N, d, R, seed)
    p, fv = acq_params(acq, y), fantasy_of(fname, y)
    m = make_model(bohip, "SEArd", X, y)
    idx, val, mu, var = m.select_batch(acq, p, Xs.T, q, fantasy=fv)
    m2 = make_model(bohip, "SEArd", X, y, capacity=N + q)
    picked = np.zeros(R, bool)
    for t in range(q):
        sc, _, _ = m2.score(acq, p, Xs.T)
        i, v, gap = masked_argmax(sc, picked)
        print(f"{acq} {fname} round {t}: loop idx {i} val {v:.12g} gap {gap:.3g} | batch idx {idx[t]} val {val[t]:.12g}")
        if gap < GAP_GUARD:
            break
        assert i == idx[t]
        assert abs(v - val[t]) <= 1e-6 * abs(v) + 64 * EPS * np.abs(m2.alpha()).sum() + 1e-12
        picked[i] = True
        yf = float(m2.predict_f(Xs[i])[0][0]) if fv == "believer" else fv
        m2.append_(Xs[i], [yf])
    assert m2.nobs == N + t + 1 and m.nobs == N
    m.close(); m2.close()


# ---- 6. errors: a status code and a message, never an abort --------------------------------------------------------------------
def test_errors(bohip):
    from bohip import _lib

    N, d, R, q, seed = CONFIGS["n500"]
    X, y, Xs = synth(N, d, R, seed)
    m = make_model(bohip, "SEArd", X, y)
    with pytest.raises(_lib.BohipError, match="q must lie in 1..R") as e:
        m.select_batch("UCB", [2.0], Xs[:5].T, 6)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.BohipError, match="q must lie") as e:
        m.select_batch("UCB", [2.0], Xs.T, 0)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.BohipError) as e:
        m.select_batch("ThompsonDraw", [0.0], Xs.T, 2)
    assert e.value.code == _lib.E_ARG
    # unknown fantasy / flags: through the raw symbol
    lib = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    xs = np.asfortranarray(Xs.T)
    prm = np.array([2.0, 0.0])
    idx, val = np.zeros(4, np.int64), np.zeros(4)
    call = lambda fantasy, flags: lib.bohip_gp_select_batch(m._h, _lib.ACQ["UCB"], prm.ctypes.data_as(dp), xs.ctypes.data_as(dp), R, 4,
                                                            fantasy, 0.0, flags, idx.ctypes.data_as(ip), val.ctypes.data_as(dp), None, None)
    assert call(7, 0) == _lib.E_ARG and b"unknown fantasy" in lib.bohip_last_error()
    assert call(0, 6) == _lib.E_ARG and b"flags" in lib.bohip_last_error()
    assert call(0, 0) == _lib.OK and len(set(idx.tolist())) == 4          # (mu, var are nullable)
    empty = bohip.ElasticGPE(d, kernel=bohip.SEArd(np.full(d, LL), LSIG))
    with pytest.raises(_lib.BohipError, match="no observations") as e:
        empty.select_batch("UCB", [2.0], Xs.T, 2)
    assert e.value.code == _lib.E_STATE
    # the size cap: V' of 2.1 M candidates at this model size is 8.9 GB > 8 GiB
    big = np.zeros((d, 2_100_000), order="F")
    with pytest.raises(_lib.BohipError, match="above the cap of 8589934592") as e:
        m.select_batch("UCB", [2.0], big, 2)
    assert e.value.code == _lib.E_UNSUPPORTED
    good = m.select_batch("UCB", [2.0], Xs.T, 4)                           # the handle works on
    assert np.array_equal(good[0], idx)
    with pytest.raises(NotImplementedError):
        bohip.MultiGPE.select_batch(None, "UCB", [2.0], Xs.T, 2)
    m.close(); empty.close()


# ---- 7. the loop: BOpt(batchsize = 4) on Branin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("acname", ["EI", "UCB"])
def test_branin_batch_regret(bohip, acname):
    """test/branin.jl:17-38 with 4 points per iteration: regret < 0.05 within the reference's budget of 200 evaluations
    (test/branin.jl:31,36): 10 initial points + 47 batches of 4 = 198 evaluations, every batch ONE incremental append."""
    from test_bo_loop_gpu import BRANIN_MIN, make_opt

    bo = bohip
    ac = {"EI": bo.ExpectedImprovement, "UCB": bo.UpperConfidenceBound}[acname]()
    model = bo.ElasticGPE(2, mean=bo.MeanConst(-10.0), kernel=bo.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=3000)
    batches = 47
    opt = make_opt(bo, model, ac, maxiterations=10 + batches, batchsize=4)
    res = bo.boptimize_(opt)
    regret = abs(res["observed_optimum"] - BRANIN_MIN)
    print(f"branin batchsize=4 {acname}: regret {regret:.4g} after {len(model.y)} evaluations, {batches} batches, "
          f"{model.info(3)} incremental appends, {model.info(2)} refits")
    assert len(model.y) == 10 + 4 * batches
    assert batches - 2 <= model.info(3) <= batches + 1      # one append per batch (the MAP fits at iterations 0 and 50 refit)
    assert regret < 0.05
