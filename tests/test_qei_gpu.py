"""Greedy Monte-Carlo q-EI batch selection on the device (bohip_gp_qei_batch / bohip_gp_qei_select, ElasticGPE.qei_batch /
qei_select, acquire_batch's "qei" method, BOpt(batchsize, batchoptions={"method": "qei"})).

Reference: tests/qei_reference.py, the NumPy twin of the contract of include/bohip_qei.h.  The summation order is part of the ABI,
so indices AND gains are compared bit for bit (assert_array_equal), on caller matrices and on the call's own draws; the draws are
compared bit for bit with bohip_gp_sample_joint's.  The statistical anchor ties the whole chain to the textbook EI of the oracle's
posterior at 5 standard errors (the bar tests/test_parity_gpu.py uses for empirical moments)."""
import math
import warnings

import numpy as np
import pytest

import qei_reference as qr
from conftest import synth
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LSIG, LNOISE, BETA = 0.2, -1.0, 0.1                                     # as tests/test_joint_gpu.py
LL = np.full(4, -0.4)
_models = {}


def model_of(bohip, kern):
    """One N = 300, d = 4 model per kernel and its 1500 candidates."""
    if kern not in _models:
        X, y, Xs = synth(300, 4, 1500, seed=31)
        m = bohip.ElasticGPE(4, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(LL, LSIG), logNoise=LNOISE, capacity=len(y))
        m.append_(X.T, y)
        _models[kern] = (m, np.asfortranarray(Xs.T), y)
    return _models[kern]


def empty_model(bohip):
    return bohip.ElasticGPE(4, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(LL, 0.0), logNoise=-1.0, capacity=8)


# ---- 1. the edges of the mapping, through qei_select ----------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 255, 256, 257, 1500])
def test_select_matches_the_twin_over_the_tile_edges(bohip, R):
    m = empty_model(bohip)                                              # the handle supplies the device and the stream only
    for S in [1, 31, 32, 33, 1000]:
        F = np.random.default_rng(1000 * R + S).standard_normal((S, R))
        q, tau = min(R, 8), 0.4
        idx, gain = m.qei_select(F, tau, q)
        ri, rg = qr.qei_greedy(F, tau, q)
        np.testing.assert_array_equal(idx, ri, err_msg=f"R = {R}, S = {S}")
        np.testing.assert_array_equal(gain, rg, err_msg=f"R = {R}, S = {S}")
    m.close()


# ---- 2. crafted matrices --------------------------------------------------------------------------------------------------------
def test_crafted_matrices(bohip):
    m = empty_model(bohip)
    nan, inf = math.nan, math.inf
    T = np.array([[1.0, 2.0, 2.0], [1.0, 0.0, 0.0]])                    # gains 1, 1, 1 -> index 0; then 1 and 2 tie at 0.5 -> 1
    idx, gain = m.qei_select(T, 0.0, 3)
    assert idx.tolist() == [0, 1, -1] and gain.tolist() == [1.0, 0.5, 0.0]
    N = np.array([[nan, 1.0, -inf, 0.5], [nan, -inf, 0.25, nan], [-inf, nan, nan, 0.5]])     # NaN and -Inf contribute 0
    idx, gain = m.qei_select(N, 0.0, 4)
    ri, rg = qr.qei_greedy(N, 0.0, 4)
    assert idx.tolist() == ri.tolist() == [1, 3, 2, -1] and not np.isnan(gain).any()
    np.testing.assert_array_equal(gain, rg)
    A = np.array([[0.5, -1.0, 0.25], [0.0, 0.5, -3.0], [0.5, 0.5, 0.5], [-inf, nan, 0.1]])   # every entry <= tau (or NaN)
    idx, gain = m.qei_select(A, 0.5, 3)
    assert idx.tolist() == [-1, -1, -1] and gain.tolist() == [0.0, 0.0, 0.0]
    E = np.array([[3.0, 1.0, 0.0, -1.0], [0.0, 2.0, 0.0, -1.0]])         # q = R: two live columns, then the set is exhausted
    idx, gain = m.qei_select(E, 0.0, 4)
    assert idx.tolist() == [0, 1, -1, -1] and gain.tolist() == [1.5, 1.0, 0.0, 0.0]
    P = np.array([[1.0, inf, 3.0], [1.0, 0.0, 0.0], [2.0, inf, 9.0]])    # +Inf wins once (gain +Inf), then its draws are dead
    idx, gain = m.qei_select(P, 0.0, 3)
    ri, rg = qr.qei_greedy(P, 0.0, 3)
    assert idx.tolist() == ri.tolist() == [1, 0, -1]
    assert gain[0] == inf and gain[1] == 1.0 / 3.0 and gain[2] == 0.0 and not np.isnan(gain).any()
    np.testing.assert_array_equal(gain, rg)
    m.close()


# ---- 3. qei_batch against the draw ----------------------------------------------------------------------------------------------
def score_record(m, xs, y):
    sc, bv, bi = m.score("EI", [y.max()], xs[:, :64])
    return sc.tobytes(), bv, bi, m.info(2), m.info(3)


@pytest.mark.parametrize("kern", ["SEArd", "Mat12Ard"])
@pytest.mark.parametrize("R", [5, 257, 1500])
def test_batch_equals_sample_joint_then_twin(bohip, kern, R):
    m, Xs, y = model_of(bohip, kern)
    xs = np.asfortranarray(Xs[:, :R])
    tau = float(y.max()) - 1.0                                          # (below max y: several rounds have something to gain)
    before = score_record(m, Xs, y)
    for S in [3, 64, 1000]:                                             # both sides of the MFMA switch at 200 draws
        seed, q = 1000 * R + S, min(R, 8)
        js = m.sample_joint(xs, S, seed)
        res = m.qei_batch(xs, q, S, seed, tau=tau, want_samples=True)
        np.testing.assert_array_equal(res.samples, js.samples)          # the draw, bit for bit
        assert (res.jitter, res.tries) == (js.jitter, js.tries)
        ri, rg = qr.qei_greedy(js.samples, tau, q)
        np.testing.assert_array_equal(res.idx, ri, err_msg=f"{kern} R = {R} S = {S}")
        np.testing.assert_array_equal(res.gain, rg, err_msg=f"{kern} R = {R} S = {S}")
        bare = m.qei_batch(xs, q, S, seed, tau=tau)                     # nothing but idx / gain crosses
        assert bare.samples is None and (bare.jitter, bare.tries) == (js.jitter, js.tries)
        np.testing.assert_array_equal(bare.idx, ri)
        np.testing.assert_array_equal(bare.gain, rg)
        again = m.qei_batch(xs, q, S, seed, tau=tau, want_samples=True)  # a second identical call: identical bytes
        assert again.idx.tobytes() == res.idx.tobytes() and again.gain.tobytes() == res.gain.tobytes()
        assert again.samples.tobytes() == res.samples.tobytes()
        si, sg = m.qei_select(js.samples, tau, q)                       # the same matrix from the caller: the same result
        np.testing.assert_array_equal(si, ri)
        np.testing.assert_array_equal(sg, rg)
        if q == 8:                                                      # prefix property in q
            short = m.qei_batch(xs, 3, S, seed, tau=tau)
            np.testing.assert_array_equal(short.idx, res.idx[:3])
            np.testing.assert_array_equal(short.gain, res.gain[:3])
    dflt = m.qei_batch(xs, 1, 64, 9)                                    # tau defaults to max y
    expl = m.qei_batch(xs, 1, 64, 9, tau=float(y.max()))
    assert dflt.idx.tolist() == expl.idx.tolist() and dflt.gain.tolist() == expl.gain.tolist()
    assert score_record(m, Xs, y) == before                             # the model is untouched


# ---- 4. statistical anchor ------------------------------------------------------------------------------------------------------
def test_q1_estimates_the_textbook_ei(bohip, orc):
    """S = 4096, q = 1, R = 200, tau = max y, SEArd, N = 300, d = 4 from synth(seed = 44).  For every candidate with more than 2 % of
    its terms positive, the column mean of max(F - tau, 0) lies within 5 standard errors (from the samples themselves) of the
    textbook EI, Delta Phi(z) + sigma phi(z), of the oracle's mu and sigma^2; at least 10 candidates must qualify.
    On the CPU the twin's draws alone (joint_reference.joint_draws on the oracle's posterior, seed 7) give 17 of 200 qualifying
    candidates with worst |z| = 1.29."""
    X, y, Xs = synth(300, 4, 200, seed=44)
    m = bohip.ElasticGPE(4, mean=bohip.MeanConst(BETA), kernel=bohip.SEArd(LL, LSIG), logNoise=LNOISE, capacity=len(y))
    m.append_(X.T, y)
    L, alpha = orc.fit(X, y, LL, LSIG, LNOISE, BETA, kern="SEArd")
    mu, cov = orc.predict_cov(X, LL, LSIG, BETA, L, alpha, Xs, kern="SEArd")
    tau, S = float(y.max()), 4096
    res = m.qei_batch(Xs.T, 1, S, 7, want_samples=True)                 # tau defaults to max y
    U = np.maximum(res.samples - tau, 0.0)
    ok = (U > 0).mean(axis=0) > 0.02
    ei = qr.textbook_ei(mu, np.diag(cov), tau)
    se = U.std(axis=0, ddof=1) / math.sqrt(S)
    z = (U.mean(axis=0)[ok] - ei[ok]) / se[ok]
    print(f"anchor: {int(ok.sum())} of 200 candidates qualify, worst |z| = {np.abs(z).max():.2f}")
    assert ok.sum() >= 10
    assert np.all(np.abs(z) <= 5.0)
    ri, rg = qr.qei_greedy(res.samples, tau, 1)
    assert res.idx.tolist() == ri.tolist() and res.gain.tolist() == rg.tolist() and ok[res.idx[0]]
    assert res.gain[0] == pytest.approx(U.mean(axis=0).max(), rel=1e-12)
    m.close()


# ---- 5. the host route ----------------------------------------------------------------------------------------------------------
def test_acquire_batch_qei_routes(bohip):
    m, Xs, y = model_of(bohip, "SEArd")
    xs = np.asfortranarray(Xs[:, :300])
    lb, ub = np.zeros(4), np.ones(4)
    seed = int(np.random.default_rng(3).integers(0, 2 ** 63 - 1))
    a = bohip.ExpectedImprovement()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                 # (the dropped-pick warning: tests/test_qei_host.py)
        val, X = bohip.acquire_batch(a, m, lb, ub, 4, {"method": "qei", "draws": 64, "xs": xs}, np.random.default_rng(3))
    assert a.tau == y.max()
    res = m.qei_batch(xs, 4, 64, seed, tau=a.tau)
    keep = res.idx >= 0                                                 # (at tau = max y, 64 draws may leave fewer than 4 picks with a gain)
    assert keep[0] and X.shape[1] == int(keep.sum())
    np.testing.assert_array_equal(X, xs[:, res.idx[keep]])
    np.testing.assert_array_equal(val, res.gain[keep])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        val, X = bohip.acquire_batch(a, m, lb, ub, 4, {"method": "qei", "draws": 64, "xs": xs, "pathwise": True, "features": 512},
                                     np.random.default_rng(3))
    with m.draw_paths(64, 512, seed) as paths:
        F, _, _ = paths.eval(xs)
    idx, gain = m.qei_select(F, a.tau, 4)
    ri, rg = qr.qei_greedy(F, a.tau, 4)
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(gain, rg)
    keep = idx >= 0
    np.testing.assert_array_equal(X, xs[:, idx[keep]])
    np.testing.assert_array_equal(val, gain[keep])


def test_one_bopt_iteration_with_the_qei_method(bohip):
    from test_bo_loop_gpu import branin

    model = bohip.ElasticGPE(2, mean=bohip.MeanConst(-10.0), kernel=bohip.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=64)
    opt = bohip.BOpt(lambda x: branin(x), model, bohip.ExpectedImprovement(), bohip.NoModelOptimizer(), [-5.0, 0.0], [10.0, 15.0],
                     sense=bohip.Min, verbosity=bohip.Silent, rng=np.random.default_rng(5), maxiterations=11, initializer_iterations=10,
                     repetitions=2, batchsize=4, batchoptions={"method": "qei", "candidates": 512, "draws": 128})
    sizes, real = [], model.append_
    model.append_ = lambda x, y: (sizes.append(np.atleast_1d(y).size), real(x, y))[1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # no pick is dropped
        bohip.boptimize_(opt)
    assert len(model.y) == 10 * 2 + 4 * 2                               # (the initial design is evaluated `repetitions` times too)
    assert sizes[-1] == 4 * 2 and sum(sizes) == 28                      # ONE update with 4 x repetitions observations
    new = model.x[:, 20:]
    assert len({tuple(c) for c in new.T}) == 4                          # four distinct points, each evaluated twice
    model.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
def test_errors(bohip):
    from bohip import _lib

    m, Xs, y = model_of(bohip, "SEArd")
    xs = np.asfortranarray(Xs[:, :10])
    F = np.zeros((4, 10))
    for call in (lambda: m.qei_batch(xs, 11, 8, 0), lambda: m.qei_select(F, 0.0, 11),                   # q > R
                 lambda: m.qei_batch(xs, 0, 8, 0), lambda: m.qei_select(F, 0.0, 0),                     # q < 1
                 lambda: m.qei_batch(xs, 2, 8, 0, tau=math.nan), lambda: m.qei_select(F, math.nan, 2),  # tau not finite
                 lambda: m.qei_batch(xs, 2, 8, 0, tau=math.inf), lambda: m.qei_select(F, -math.inf, 2),
                 lambda: m.qei_batch(xs, 2, 0, 0), lambda: m.qei_select(np.zeros((0, 10)), 0.0, 2),     # S < 1
                 lambda: m.qei_batch(xs, 2, 8, 0, jitter=-1.0), lambda: m.qei_batch(xs, 2, 8, 0, max_tries=-1)):
        with pytest.raises(_lib.BohipError) as e:
            call()
        assert e.value.code == _lib.E_ARG
    big = np.zeros((4, 70000), order="F")                               # one candidate chunk holds at most 65536
    with pytest.raises(_lib.BohipError, match="qei_batch: R exceeds one candidate chunk") as e:
        m.qei_batch(big, 2, 1, 0)
    assert e.value.code == _lib.E_UNSUPPORTED
    lib = _lib.load()                                                   # 2^31 draws of 8 candidates: 128 GiB, refused before any read
    idx, gain = np.zeros(2, dtype=np.int64), np.zeros(2)
    import ctypes as C
    rc = lib.bohip_gp_qei_select(m._h, F.ctypes.data_as(C.POINTER(C.c_double)), 2 ** 31, 8, 0.0, 2,
                                 idx.ctypes.data_as(C.POINTER(C.c_int64)), gain.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == _lib.E_UNSUPPORTED and b"largest S at R = 8 is 2097120" in lib.bohip_last_error()
    empty = empty_model(bohip)
    with pytest.raises(_lib.BohipError) as e:
        empty.qei_batch(xs, 2, 8, 0)
    assert e.value.code == _lib.E_STATE
    idx, gain = empty.qei_select(np.array([[1.0, 2.0]]), 0.0, 1)        # ... while the selection alone needs no observations
    assert idx.tolist() == [1] and gain.tolist() == [2.0]
    empty.close()
    ok = m.qei_batch(xs, 2, 8, 0, tau=float(y.max()) - 1.0)             # the handle works on
    assert ok.idx.shape == (2,) and ok.idx[0] >= 0
