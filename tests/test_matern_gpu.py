"""Matérn 1/2, 3/2 and the iso Matérn kernels (ids 3-7) on the device, against the NumPy model of tests/matern_reference.py.

Sizes are chosen so that every schedule the library picks by size runs for each new family: the row-wise small batch
(R <= 32), split-K (N = 1100, R = 700; N = 1500, R = 300), whole-K (N = 3000, R = 4096), the factorisation with 3 row tiles
(N = 300) and the production executor form (N = 3000), the one-workgroup-per-start ascent (N = 200) and the batched one
(N = 600)."""
import math

import numpy as np
import pytest
from scipy.optimize import minimize

from conftest import synth, var_tol
from matern_reference import NEW_KERNELS, MaternGP, first_argmax
from test_parity_gpu import bohip, mu_floor  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

LSIG, LNOISE, BETA = 0.1, -2.0, 0.05
BIG = ["Mat32Ard", "Mat12Iso"]   # the two families at N = 3000
ACQS = [("EI", None), ("UCB", [2.5]), ("PI", None), ("MI", [1.0, 0.3]), ("MaxMean", [])]


def loglen(kern, d):
    return np.array([-0.5]) if kern.endswith("Iso") else np.linspace(-0.8, -0.2, d)


def build(bohip, kern, X, y, ll=None, capacity=None):
    d = X.shape[1]
    ll = loglen(kern, d) if ll is None else ll
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(ll, LSIG), logNoise=LNOISE,
                         capacity=capacity or len(y))
    m.append_(X.T, y)
    return m, MaternGP(kern, X, y, ll, LSIG, LNOISE, BETA)


def params(acq, p, y):
    return [float(np.median(y))] if p is None else p


# ---- refit and append ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N", [(k, 300) for k in NEW_KERNELS] + [(k, 3000) for k in BIG])
def test_refit_factor_and_alpha(bohip, kern, N):
    X, y, _ = synth(N, 5, 1, seed=40 + N)
    m, ref = build(bohip, kern, X, y)
    m.fit_()
    np.testing.assert_allclose(m.alpha(), ref.alpha, rtol=1e-9, atol=1e-9 * np.abs(ref.alpha).max())
    if N <= 300:
        np.testing.assert_allclose(m.factor(), ref.L, rtol=1e-9, atol=1e-12)
    else:
        L = m.factor()
        np.testing.assert_allclose(np.diag(L), np.diag(ref.L), rtol=1e-9)
        np.testing.assert_allclose(L[-5:], ref.L[-5:], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("kern", NEW_KERNELS)
def test_append_in_batches_equals_refit(bohip, kern):
    X, y, Xs = synth(260, 4, 50, seed=7)
    ll = loglen(kern, 4)
    m = bohip.ElasticGPE(4, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(ll, LSIG), logNoise=LNOISE, capacity=300)
    m.append_(X[:200].T, y[:200])
    n0 = m.info(3)
    for a, b in ((200, 220), (220, 235), (235, 259), (259, 260)):
        m.append_(X[a:b].T, y[a:b])
    assert m.info(3) - n0 == 4   # four incremental extensions, no refit
    ref = MaternGP(kern, X, y, ll, LSIG, LNOISE, BETA)
    np.testing.assert_allclose(m.alpha(), ref.alpha, rtol=1e-9, atol=1e-9 * np.abs(ref.alpha).max())
    mu, var = m.predict_f(Xs.T)
    mu_r, var_r = ref.predict(Xs)
    np.testing.assert_allclose(mu, mu_r, rtol=1e-9, atol=mu_floor(ref.alpha, ref.s2f))
    assert np.all(np.abs(var - var_r) <= var_tol(var_r, 260, ref.s2f))


# ---- scoring ------------------------------------------------------------------------------------------------------------
SCORE_CASES = [(k, N, R) for k in NEW_KERNELS for N, R in ((400, 17), (1100, 700), (1500, 300))] + \
              [(k, 3000, 4096) for k in BIG]


@pytest.mark.parametrize("kern,N,R", SCORE_CASES)
def test_score_and_argmax(bohip, kern, N, R):
    d = 5
    X, y, Xs = synth(N, d, R, seed=N + R)
    m, ref = build(bohip, kern, X, y)
    mu_r, var_r = ref.predict(Xs)
    mu, var = m.predict_f(Xs.T)
    floor = mu_floor(ref.alpha, ref.s2f)
    np.testing.assert_allclose(mu, mu_r, rtol=1e-6, atol=floor)
    assert np.all(np.abs(var - var_r) <= var_tol(var_r, N, ref.s2f))
    for acq, p in ACQS:
        p = params(acq, p, y)
        sc, bv, bi = m.score(acq, p, Xs.T)
        sc_r = ref.score(acq, p, Xs)
        assert np.all(np.abs(sc - sc_r) <= 1e-6 * np.abs(sc_r) + floor + 1e-12), (acq, np.abs(sc - sc_r).max())
        assert (bv, bi) == first_argmax(sc)
        assert bi == first_argmax(sc_r)[1], acq


@pytest.mark.parametrize("kern", BIG)
def test_pruned_value_only_record_equals_full_pass(bohip, kern):
    X, y, Xs = synth(3000, 8, 4096, seed=11)
    m, _ = build(bohip, kern, X, y, ll=(np.array([math.log(0.5)]) if kern.endswith("Iso") else np.full(8, math.log(0.5))))
    tau = [float(y.max())]
    _, bv_full, bi_full = m.score("EI", tau, Xs.T, want_scores=True)
    for _ in range(3):
        _, bv, bi = m.score("EI", tau, Xs.T, want_scores=False)
        assert (bv, bi) == (bv_full, bi_full)
    assert np.float64(bv).tobytes() == np.float64(bv_full).tobytes()


# ---- gradient -----------------------------------------------------------------------------------------------------------
GRAD_CASES = [(k, 400, 10) for k in NEW_KERNELS] + [(k, 1100, 700) for k in NEW_KERNELS] + [(k, 3000, 4096) for k in BIG]


@pytest.mark.parametrize("kern,N,R", GRAD_CASES)
def test_score_grad(bohip, kern, N, R):
    d = 4
    X, y, Xs = synth(N, d, R, seed=3 * N + R)
    m, ref = build(bohip, kern, X, y)
    floor = mu_floor(ref.alpha, ref.s2f)
    sub = np.arange(R) if R <= 64 else np.random.default_rng(0).choice(R, 48, replace=False)
    for acq, p in ACQS:
        p = params(acq, p, y)
        sc, g = m.score_grad(acq, p, Xs.T)
        sc_r, g_r = ref.score_grad(acq, p, Xs[sub])
        np.testing.assert_allclose(sc[sub], sc_r, rtol=1e-6, atol=floor + 1e-12)
        np.testing.assert_allclose(g.T[sub], g_r, rtol=1e-6, atol=1e-9 * np.abs(g_r).max() + 1e-12)
        np.testing.assert_array_equal(sc, m.score(acq, p, Xs.T)[0])   # value path == gradient path, bit for bit
    if R <= 64:   # batch == single
        sc, g = m.score_grad("UCB", [2.5], Xs.T)
        for i in (0, R - 1):
            s1, g1 = m.score_grad("UCB", [2.5], Xs[i:i + 1].T)
            np.testing.assert_array_equal(s1[0], sc[i])
            np.testing.assert_array_equal(g1[:, 0], g[:, i])


@pytest.mark.parametrize("kern", ["Mat12Ard", "Mat12Iso"])
@pytest.mark.parametrize("R", [3, 700])
def test_mat12_gradient_on_an_observation(bohip, kern, R):
    X, y, Xs = synth(300, 3, R, seed=9)
    Xs[1] = X[17]
    m, ref = build(bohip, kern, X, y)
    for acq, p in (("UCB", [2.5]), ("EI", [float(y.max())])):
        _, g = m.score_grad(acq, p, Xs.T)
        assert np.all(np.isfinite(g))
        _, g_r = ref.score_grad(acq, p, Xs[1:2])
        np.testing.assert_allclose(g[:, 1], g_r[0], rtol=1e-6, atol=1e-9 * np.abs(g_r).max() + 1e-12)


# ---- ascent -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", NEW_KERNELS)
@pytest.mark.parametrize("N", [200, 600])
def test_acquire_max(bohip, kern, N):
    from bohip.utils import latin_hypercube_sampling

    d = 3
    X, y, _ = synth(N, d, 1, seed=N + 1)
    m, ref = build(bohip, kern, X, y)
    lb, ub = np.zeros(d), np.ones(d)
    starts = latin_hypercube_sampling(lb, ub, 10, np.random.default_rng(2))
    for acq, p in (("UCB", [2.0]), ("EI", [float(np.median(y))])):
        f, Xo, bv, bi, bx, ev = m.ascend(acq, p, lb, ub, starts)
        assert np.all(np.isfinite(f)) and np.all(Xo >= lb[:, None]) and np.all(Xo <= ub[:, None])
        f0 = ref.score(acq, p, starts.T)
        fe = ref.score(acq, p, Xo.T)
        assert np.all(fe >= f0 - 1e-9 * np.abs(f0).max())
        assert (bv, bi) == first_argmax(f)
        if kern.startswith("Mat12"):
            continue   # kinks at the observations: no KKT point to assert
        _, g = ref.score_grad(acq, p, Xo.T)   # KKT: the projected gradient has all but vanished against the starts'
        _, g0 = ref.score_grad(acq, p, starts.T)
        free = (Xo.T > lb + 1e-7) & (Xo.T < ub - 1e-7)
        assert np.all(np.abs(g[free]) <= 1e-3 * np.abs(g0).max()), (np.abs(g[free]).max(), np.abs(g0).max())
        hit = 0
        for i in range(10):
            res = minimize(lambda x: (-ref.score(acq, p, x)[0], -ref.score_grad(acq, p, x[None, :])[1][0]), starts[:, i],
                           jac=True, method="L-BFGS-B", bounds=list(zip(lb, ub)), options=dict(ftol=1e-15, gtol=1e-12))
            hit += fe[i] >= -res.fun - 1e-9 * abs(res.fun)
        assert hit >= 8, hit


# ---- marginal likelihood --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", NEW_KERNELS)
def test_mll_and_gradient(bohip, kern):
    X, y, _ = synth(257, 4, 1, seed=21)
    m, ref = build(bohip, kern, X, y)
    mll, dn, dm, dk = m.mll_grad()
    mr, dnr, dmr, dkr = ref.mll_grad()
    assert dk.size == (2 if kern.endswith("Iso") else 5)
    assert mll == pytest.approx(mr, rel=1e-9)
    assert m.mll() == pytest.approx(mr, rel=1e-9)
    g, gr = np.concatenate([[dn, dm], dk]), np.concatenate([[dnr, dmr], dkr])
    np.testing.assert_allclose(g, gr, rtol=1e-6, atol=1e-8 * np.abs(gr).max())


@pytest.mark.parametrize("kern", ["Mat32Ard", "Mat52Iso"])
def test_mll_grad_central_differences_n3000(bohip, kern):
    X, y, _ = synth(3000, 3, 1, seed=5)
    ll = loglen(kern, 3)
    m, _ = build(bohip, kern, X, y, ll=ll)
    _, dn, dm, dk = m.mll_grad()
    g = np.concatenate([[dn], dk])
    theta = np.concatenate([[LNOISE], ll, [LSIG]])
    h = 1e-5
    fd = []
    for e in np.eye(theta.size):
        vals = []
        for t in (theta + h * e, theta - h * e):
            m.set_params_(ll=t[1:-1], lsigma=t[-1], logNoise=t[0])
            vals.append(m.mll())
        fd.append((vals[0] - vals[1]) / (2 * h))
    np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-6 * np.abs(fd).max())


def test_map_round_raises_mll(bohip):
    from bohip.bopt import optimizemodel_, MAPGPOptimizer

    X, y, _ = synth(120, 2, 1, seed=8)
    m, _ = build(bohip, "Mat32Ard", X, y, ll=np.zeros(2))
    before = m.mll()
    opt = MAPGPOptimizer(every=1, noisebounds=[-4, 3], kernbounds=[[-3, -3, -2], [3, 3, 3]], maxeval=60)
    optimizemodel_(opt, m)
    assert m.mll() > before
    assert np.all(m.kernel.ll >= -3) and np.all(m.kernel.ll <= 3) and -2 <= m.kernel.lsigma <= 3 and -4 <= m.logNoise <= 3
    iso, _ = build(bohip, "Mat12Iso", X, y, ll=np.zeros(1))   # kernel bounds of length 2 for an iso model
    before = iso.mll()
    optimizemodel_(MAPGPOptimizer(every=1, noisebounds=[-4, 3], kernbounds=[[-3, -2], [3, 3]], maxeval=60), iso)
    assert iso.mll() > before and iso.kernel.ll.size == 1


# ---- joint covariance, Thompson, DIRECT-L ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", NEW_KERNELS)
def test_predict_cov_thompson_direct(bohip, kern):
    from bohip import _lib

    X, y, Xs = synth(300, 3, 200, seed=13)
    m, ref = build(bohip, kern, X, y)
    mu, cv = m.predict_cov(Xs.T)
    mu_r, cv_r = ref.predict_cov(Xs)
    np.testing.assert_allclose(mu, mu_r, rtol=1e-6, atol=mu_floor(ref.alpha, ref.s2f))
    assert np.all(np.abs(cv - cv_r) <= var_tol(cv_r, 300, ref.s2f))
    S, seed = 3, 77
    bv, bi = m.thompson(Xs.T, S, seed=seed)
    mu_d, var_d = m.predict_f(Xs.T)
    lib = _lib.load()
    for s in range(S):
        z = np.array([lib.bohip_thompson_normal(seed, s, j) for j in range(len(Xs))])
        draw = mu_d + np.sqrt(var_d) * z
        assert (bv[s], bi[s]) == first_argmax(draw)
    # DIRECT-L on x -> myrand(model, x): the e-th evaluated point draws z = bohip_thompson_normal(seed, 0, e).  Replaying the search
    # with the same draws on the host gives the same (best_f, evaluations, best_x), so best_f is the draw at best_x.
    from bohip.acquisition import _batched_direct_l

    lb, ub, seed, cnt = np.zeros(3), np.ones(3), 5, [0]

    def f_draw(Z):
        mu_z, var_z = m.predict_f(Z)
        z = np.array([lib.bohip_thompson_normal(seed, 0, cnt[0] + j) for j in range(Z.shape[1])])
        cnt[0] += Z.shape[1]
        return mu_z + np.sqrt(np.maximum(var_z, 0.0)) * z

    f1, x1, e1 = _batched_direct_l(f_draw, lb, ub, 300)
    bf, bx, ev, _ = m.direct_max("ThompsonDraw", None, lb, ub, maxeval=300, seed=seed)
    assert (bf, ev) == (f1, e1) and np.array_equal(bx, x1) and cnt[0] == ev
    assert np.isfinite(bf) and np.all((bx >= lb) & (bx <= ub))


# ---- multi-GPU exchange ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["Mat32Ard", "Mat12Iso"])
def test_multigpu_winner_bit_identical(bohip, kern):
    X, y, Xs = synth(900, 4, 4099, seed=3)
    ll = loglen(kern, 4)
    single, _ = build(bohip, kern, X, y, ll=ll)
    mg = bohip.MultiGPE(4, devices=[0], shards_per_device=8, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(ll, LSIG),
                        logNoise=LNOISE, capacity=len(y))
    mg.append_(X.T, y)
    for acq, p in (("EI", [float(y.max())]), ("UCB", [2.0])):
        _, bv, bi = single.score(acq, p, Xs.T)
        _, bv2, bi2 = mg.score(acq, p, Xs.T)
        assert bi2 == bi and np.float64(bv2).tobytes() == np.float64(bv).tobytes()


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_boptimize_branin_mat32(bohip):
    bo = bohip

    def branin(x):
        x1, x2 = x
        return (x2 - 5.1 / (4 * math.pi ** 2) * x1 ** 2 + 5 / math.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * math.pi)) * math.cos(x1) + 10

    model = bo.ElasticGPE(2, mean=bo.MeanConst(-10.0), kernel=bo.Mat32Ard([0.0, 0.0], 5.0), logNoise=-2.0, capacity=100)
    start = np.array([0.0, 0.0, 5.0])
    opt = bo.BOpt(branin, model, bo.UpperConfidenceBound(),
                  bo.MAPGPOptimizer(every=2, noisebounds=[-4, 3], kernbounds=[[-1, -1, 0], [4, 4, 10]], maxeval=40),
                  [-5.0, 0.0], [10.0, 15.0], sense=bo.Min, maxiterations=15, initializer_iterations=10,
                  acquisitionoptions=dict(method="LD_LBFGS", restarts=5, maxeval=500), verbosity=bo.Silent,
                  rng=np.random.default_rng(4))
    res = bo.boptimize_(opt)
    assert bo.dims(model) == (2, 15)
    now = np.concatenate([model.kernel.ll, [model.kernel.lsigma]])
    assert np.any(now != start)
    assert np.all(now >= [-1, -1, 0]) and np.all(now <= [4, 4, 10])
    assert np.isfinite(res["model_optimum"])
    assert np.all(res["model_optimizer"] >= [-5.0, 0.0]) and np.all(res["model_optimizer"] <= [10.0, 15.0])
