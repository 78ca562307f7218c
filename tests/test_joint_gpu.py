"""Joint posterior draws over a candidate set on the device (bohip_gp_sample_joint, ElasticGPE.sample_joint, the "joint"
acquisition option, acquire_thompson_batch, BOpt(batchsize) with ThompsonSamplingSimple).

Reference: the oracle's predict_cov (SE, Matérn 5/2) or tests/matern_reference.py (ids 3-7) for (mu, Sigma); the library's own
generator (NumPy twin in tests/joint_reference.py) for z.  Tolerances, eps = 2^-52:
  factor residual  |C C' - (Sigma_o + jitter I)| <= var_tol(Sigma_o, N, s_f^2) + 64 R eps (max diag Sigma_o + jitter)
                   (what the project grants the device's Sigma, plus the 64 n eps scale form it grants a factor)
  draw identity    |f_sj - (mu_j + sum_k C_jk z_sk)| <= 2 (R + 2) eps (|mu_j| + sum_k |C_jk| |z_sk|)   (C, mu: the call's own)
  arg-max          bit for bit the first maximum of the returned samples
Both precision checks are backward-error statements, so they hold whatever the conditioning of Sigma and whichever jitter the
call needed."""
import math
import warnings

import numpy as np
import pytest

from conftest import synth, var_tol
from joint_reference import (EPS, distinct_picks, draw_identity_bound, first_argmax_rows, normals)
from matern_reference import MaternGP
from test_parity_gpu import bohip, mu_floor  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

LSIG, LNOISE, BETA = 0.2, -1.0, 0.1
S2F = math.exp(2 * LSIG)
ORACLE_KERNELS = ("SEArd", "SEIso", "Mat52Ard")


def build(bohip, kern, X, y, ll):
    m = bohip.ElasticGPE(X.shape[1], mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(ll, LSIG), logNoise=LNOISE,
                         capacity=len(y))
    m.append_(X.T, y)
    return m


def posterior(orc, kern, X, y, ll, Xs):
    """(mu_o, Sigma_o, alpha) of the reference."""
    if kern in ORACLE_KERNELS:
        L, alpha = orc.fit(X, y, ll, LSIG, LNOISE, BETA, kern=kern)
        mu, cov = orc.predict_cov(X, ll, LSIG, BETA, L, alpha, Xs, kern=kern)
        return mu, cov, alpha
    ref = MaternGP(kern, X, y, ll, LSIG, LNOISE, BETA)
    mu, cov = ref.predict_cov(Xs)
    return mu, cov, ref.alpha


def factor_bound(cov_o, N, jitter):
    R = cov_o.shape[0]
    return var_tol(cov_o, N, S2F) + 64 * R * EPS * (float(np.max(np.diag(cov_o))) + jitter)


def check_factor(js, cov_o, N):
    C = js.factor
    R = C.shape[0]
    assert np.all(np.diag(C) > 0)
    assert not np.any(np.triu(C, 1))                                   # exactly zero above the diagonal
    res = np.abs(C @ C.T - (cov_o + js.jitter * np.eye(R)))
    bound = factor_bound(cov_o, N, js.jitter)
    print(f"  factor residual: worst {res.max():.3e}, worst share of the bound {(res / bound).max():.3f} (R = {R}, jitter {js.jitter:.3e}, "
          f"tries {js.tries})")
    assert np.all(res <= bound)


def check_draws(js, seed):
    S, R = js.samples.shape
    Z = normals(seed, S, R)
    ref = js.mu[None, :] + Z @ js.factor.T
    err = np.abs(js.samples - ref)
    bound = draw_identity_bound(js.mu, js.factor, Z)
    print(f"  draw identity: worst {err.max():.3e}, worst share of the bound {(err / bound).max():.3f} (S = {S}, R = {R})")
    assert np.all(err <= bound)
    return Z


def check_best(js):
    bv, bi = first_argmax_rows(js.samples)
    np.testing.assert_array_equal(js.best_idx, bi)
    np.testing.assert_array_equal(js.best_val, bv)


# ---- 1-3. factor residual, draw identity, arg-max over the tile edges -------------------------------------------------------
RS = [1, 5, 128, 129, 257, 1024, 1500]
SS = [1, 3, 64, 1000]
SHAPES = {"SEArd": (4, np.full(4, -0.4)), "Mat52Ard": (4, np.full(4, -0.4)), "Mat12Ard": (4, np.full(4, -0.4))}
_post = {}


def shape_case(bohip, orc, kern):
    """model + reference posterior at the 1500 candidates, once per kernel (the posterior of the first R candidates is the
    leading block)."""
    if kern not in _post:
        d, ll = SHAPES[kern]
        X, y, Xs = synth(300, d, max(RS), seed=31)
        _post[kern] = (build(bohip, kern, X, y, ll), Xs, posterior(orc, kern, X, y, ll, Xs), len(y))
    return _post[kern]


@pytest.mark.parametrize("kern", list(SHAPES))
@pytest.mark.parametrize("R", RS)
def test_factor_draws_and_argmax(bohip, orc, kern, R):
    m, Xs, (mu_o, cov_o, alpha), N = shape_case(bohip, orc, kern)
    xs = np.asfortranarray(Xs[:R].T)
    mu_pc, _ = m.predict_cov(xs)
    for S in SS:
        seed = 1000 * R + S
        js = m.sample_joint(xs, S, seed, want_factor=True)
        print(f"{kern} R = {R} S = {S}:")
        np.testing.assert_array_equal(js.mu, mu_pc)                    # predict_cov's mean, bit for bit
        check_factor(js, cov_o[:R, :R], N)
        check_draws(js, seed)
        check_best(js)
        only = m.sample_joint(xs, S, seed, want_samples=False)         # the winners alone: same records
        assert only.samples is None and only.factor is None
        np.testing.assert_array_equal(only.best_idx, js.best_idx)
        np.testing.assert_array_equal(only.best_val, js.best_val)
        assert (only.jitter, only.tries) == (js.jitter, js.tries)


@pytest.mark.parametrize("kern", ["SEArd", "Mat12Ard"])
def test_draws_are_keyed_by_the_draw_number(bohip, orc, kern):
    """A call with fewer draws reproduces the leading rows of a call with more: bit for bit inside one kernel form (2 and 3 draws
    take the row-panel form, 256 and 1000 the MFMA form), within the draw-identity bound across the two (4 against 1000)."""
    m, Xs, _, _ = shape_case(bohip, orc, kern)
    for R in (129, 1024):
        xs = np.asfortranarray(Xs[:R].T)
        a, b = m.sample_joint(xs, 2, 9), m.sample_joint(xs, 3, 9)
        np.testing.assert_array_equal(a.samples, b.samples[:2])
        a, big = m.sample_joint(xs, 256, 9), m.sample_joint(xs, 1000, 9)
        np.testing.assert_array_equal(a.samples, big.samples[:256])
        np.testing.assert_array_equal(a.best_idx, big.best_idx[:256])
        a, b = m.sample_joint(xs, 4, 9, want_factor=True), big
        bound = draw_identity_bound(a.mu, a.factor, normals(9, 4, R))
        assert np.all(np.abs(a.samples - b.samples[:4]) <= bound)


# ---- 4. end to end against the reference arithmetic on well-conditioned shapes ---------------------------------------------
@pytest.mark.parametrize("kern,d,ll", [("SEArd", 8, -1.0), ("Mat52Ard", 8, -0.4), ("Mat12Ard", 4, -0.4)])
def test_end_to_end_vs_reference_factor(bohip, orc, kern, d, ll):
    """samples against mu_o + chol(Sigma_o) z.  Bound: the first-order perturbation bound of the Cholesky factor (Sun 1991; Higham,
    Accuracy and Stability, Thm 10.8)  ||dC||_F <= kappa_2 / sqrt2 * ||dSigma||_F / ||Sigma||_2 * ||C||_2  with dSigma the bound of
    the factor-residual check, times ||z_s||_2, plus the mean's tolerance.  It is loose (of the order of 1e-3): it catches a wrong
    triangle, a wrong draw index, a transposed output; the precision claims rest on the two backward-error checks."""
    N, R, S, seed = 300, 1024, 64, 12
    X, y, Xs = synth(N, d, R, seed=31)
    llv = np.full(d, ll)
    m = build(bohip, kern, X, y, llv)
    mu_o, cov_o, alpha = posterior(orc, kern, X, y, llv, Xs)
    js = m.sample_joint(Xs.T, S, seed, want_factor=True)
    assert js.tries == 0 and js.jitter == 0.0
    w = np.linalg.eigvalsh(cov_o)
    kappa = w[-1] / w[0]
    assert w[0] > 0 and kappa <= 1e4, kappa
    C_o = np.linalg.cholesky(cov_o)
    Z = normals(seed, S, R)
    ref = mu_o[None, :] + Z @ C_o.T
    dC = kappa / math.sqrt(2.0) * np.linalg.norm(factor_bound(cov_o, N, 0.0)) / w[-1] * np.linalg.norm(C_o, 2)
    bound = dC * np.linalg.norm(Z, axis=1)[:, None] + 1e-6 * np.abs(mu_o)[None, :] + mu_floor(alpha, S2F)
    err = np.abs(js.samples - ref)
    print(f"{kern}: kappa_2 {kappa:.3g}, lambda_min {w[0]:.3g}; worst |samples - reference| {err.max():.3e} "
          f"(bound {bound.min():.3e} .. {bound.max():.3e}); worst |C - C_o| {np.abs(js.factor - C_o).max():.3e}")
    assert np.all(err <= bound)
    check_factor(js, cov_o, N)


# ---- 5. joint, not independent ----------------------------------------------------------------------------------------------
def test_twins_move_together(bohip, orc):
    """256 candidates, each followed by its twin x + 1e-3 e_1: under a JOINT draw the twins' deviations from their means differ by
    a few standard deviations of (f_a - f_b), which is tiny; under independent per-candidate draws (model.thompson's construction,
    recomputed here) they differ by the candidates' own standard deviations."""
    N, d, seed, S = 300, 4, 7, 64
    X, y, Xa = synth(N, d, 256, seed=31)
    Xb = Xa.copy()
    Xb[:, 0] += 1e-3
    Xs = np.empty((512, d))
    Xs[0::2], Xs[1::2] = Xa, Xb
    ll = np.full(d, -0.4)
    m = build(bohip, "Mat52Ard", X, y, ll)
    _, cov_o, _ = posterior(orc, "Mat52Ard", X, y, ll, Xs)
    js = m.sample_joint(Xs.T, S, seed)
    t = float(var_tol(np.abs(cov_o).max(), N, S2F))
    a, b = np.arange(0, 512, 2), np.arange(1, 512, 2)
    var_ab = cov_o[a, a] + cov_o[b, b] - 2 * cov_o[a, b]
    bound = 6 * np.sqrt(var_ab + 2 * js.jitter + 4 * t)
    dev = js.samples - js.mu[None, :]
    diff = np.abs(dev[:, a] - dev[:, b])
    print(f"twins: worst share of the bound {(diff / bound[None, :]).max():.3f}, jitter {js.jitter:.3e}, t = {t:.3e}")
    assert np.all(diff <= bound[None, :])
    Z = normals(seed, S, 512)
    sd = np.sqrt(np.maximum(np.diag(cov_o), 0.0))
    indep = np.abs(sd[a][None, :] * Z[:, a] - sd[b][None, :] * Z[:, b])
    share = float(np.mean(indep > bound[None, :]))
    print(f"twins: independent draws exceed the bound for {100 * share:.1f} % of (draw, pair) combinations")
    assert share > 0.5


# ---- 6. moments -------------------------------------------------------------------------------------------------------------
def test_moments_of_one_call(bohip):
    """test_joint_draw_has_posterior_moments' shape and thresholds, with ONE device call of 4000 draws."""
    X, y, Xs = synth(120, 2, 6, seed=4)
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.array([-0.5, -0.5]), 0.0), logNoise=-1.0, capacity=120)
    m.append_(X.T, y)
    S = 4000
    draws = m.sample_joint(Xs.T, S, seed=0).samples
    assert draws.shape == (S, 6)
    mu, cov = m.predict_cov(Xs.T)
    sd = np.sqrt(np.diag(cov))
    dm = np.abs(draws.mean(0) - mu) / (sd / math.sqrt(S))
    dc = np.abs(np.cov(draws.T) - cov) / np.outer(sd, sd)
    print(f"moments: worst mean deviation {dm.max():.2f} (limit 5), worst covariance deviation {dc.max():.3f} (limit 0.15)")
    assert np.all(np.abs(draws.mean(0) - mu) <= 5 * sd / math.sqrt(S))
    assert np.all(np.abs(np.cov(draws.T) - cov) <= 0.15 * np.outer(sd, sd) + 1e-12)
    one = bohip.myrand(m, Xs.T, seed=0)                                 # the seeded generic function is the device draw
    np.testing.assert_array_equal(one, draws[0])


# ---- 7. jitter --------------------------------------------------------------------------------------------------------------
def jitter_case(bohip, m, Xs, cov_o, N, seed=3, S=5):
    from bohip import _lib

    try:
        js0 = m.sample_joint(Xs.T, S, seed, max_tries=0, want_factor=True)
    except _lib.NotPositiveDefinite:
        js0 = None
        assert m.info(_lib.INFO_PIVOT) >= 1
    if js0 is not None:                                                # rounding left a positive pivot: then it is a factor
        assert js0.tries == 0 and js0.jitter == 0.0
        check_factor(js0, cov_o, N)
    js = m.sample_joint(Xs.T, S, seed, want_factor=True)
    check_factor(js, cov_o, N)
    check_draws(js, seed)
    check_best(js)
    assert np.all(np.isfinite(js.samples))
    if js.tries == 0:
        assert js.jitter == 0.0
    else:
        want = 1e-12 * 10.0 ** (js.tries - 1) * float(np.max(np.diag(cov_o)))
        assert abs(js.jitter - want) <= 1e-5 * want, (js.jitter, want, js.tries)
    print(f"  jitter case: max_tries = 0 -> {'NotPositiveDefinite' if js0 is None else 'a factor'}; defaults -> tries {js.tries}, "
          f"jitter {js.jitter:.3e}")
    return js


def test_jitter_on_an_exactly_singular_sigma(bohip, orc):
    N, d, R = 300, 8, 1024
    X, y, Xs = synth(N, d, R, seed=31)
    Xs = np.concatenate([Xs, Xs[:8]])                                   # 8 duplicated candidates: Sigma is exactly singular
    ll = np.full(d, -1.0)
    m = build(bohip, "SEArd", X, y, ll)
    _, cov_o, _ = posterior(orc, "SEArd", X, y, ll, Xs)
    jitter_case(bohip, m, Xs, cov_o, N)


def test_jitter_on_a_numerically_singular_sigma(bohip, orc):
    N, d, R = 129, 2, 257
    X, y, Xs = synth(N, d, R, seed=31)
    m = build(bohip, "SEIso", X, y, -0.4)
    _, cov_o, _ = posterior(orc, "SEIso", X, y, -0.4, Xs)
    jitter_case(bohip, m, Xs, cov_o, N)


# ---- 8. the model is untouched; argument errors -----------------------------------------------------------------------------
def test_model_is_untouched_and_errors(bohip):
    from bohip import _lib

    N, d = 300, 4
    X, y, Xs = synth(N, d, 700, seed=2)
    ll = np.full(d, -0.4)
    m = build(bohip, "SEArd", X, y, ll)
    m.fit_()

    def state():
        sc = m.score("EI", [float(y.max())], Xs[:300].T)
        return m.factor(), m.alpha(), m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS), m.info(_lib.INFO_CHOL_FORM), sc

    before = state()
    m.sample_joint(Xs[:130].T, 3, 1)
    m.sample_joint(Xs.T, 40, 2, want_factor=True)
    after = state()
    for a, b in zip(before[:2], after[:2]):
        np.testing.assert_array_equal(a, b)
    assert before[2:5] == after[2:5]
    np.testing.assert_array_equal(before[5][0], after[5][0])
    assert before[5][1:] == after[5][1:]
    m.fit_()                                                            # a refit after the sampler: the same factor, bit for bit
    np.testing.assert_array_equal(m.factor(), before[0])
    np.testing.assert_array_equal(m.alpha(), before[1])
    # errors
    for kw in (dict(S=0), dict(jitter=-1.0), dict(jitter=float("nan")), dict(jitter=float("inf")), dict(max_tries=-1)):
        with pytest.raises(_lib.BohipError) as e:
            m.sample_joint(Xs[:10].T, **{"S": 1, **kw})
        assert e.value.code == _lib.E_ARG, kw
    with pytest.raises(_lib.BohipError) as e:
        m.sample_joint(np.zeros((d, 0), order="F"), 1)
    assert e.value.code == _lib.E_ARG
    big = np.zeros((d, 70000), order="F")                               # one candidate chunk holds at most 65536
    with pytest.raises(_lib.BohipError, match="sample_joint: R exceeds one candidate chunk") as e:
        m.sample_joint(big, 1, want_samples=False)
    assert e.value.code == _lib.E_UNSUPPORTED
    empty = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(ll, 0.0), logNoise=-1.0, capacity=8)
    with pytest.raises(_lib.BohipError) as e:
        empty.sample_joint(Xs[:10].T, 1)
    assert e.value.code == _lib.E_STATE
    ok = m.sample_joint(Xs[:10].T, 1)                                   # the handle works on
    assert ok.samples.shape == (1, 10)
    m.close(); empty.close()


def test_multigpe_runs_it_on_the_first_replica(bohip):
    X, y, Xs = synth(200, 3, 140, seed=8)
    ll = np.full(3, -0.4)
    one = build(bohip, "SEArd", X, y, ll)
    mg = bohip.MultiGPE(3, mean=bohip.MeanConst(BETA), kernel=bohip.SEArd(ll, LSIG), logNoise=LNOISE, capacity=200, devices=[0])
    mg.append_(X.T, y)
    a, b = one.sample_joint(Xs.T, 5, 4), mg.sample_joint(Xs.T, 5, 4)
    np.testing.assert_array_equal(a.samples, b.samples)
    np.testing.assert_array_equal(a.best_idx, b.best_idx)
    one.close(); mg.close()


# ---- 9. the loop --------------------------------------------------------------------------------------------------------------
def test_distinct_picks_on_a_repeating_winner(bohip):
    """Mat52Ard d = 8, N = 300, R = 1024, seed 5: in the NumPy twin draws 0 and 3 both pick candidate 529, so the raw winners
    repeat and the greedy rule has something to do."""
    from bohip.acquisition import _distinct_picks

    N, d, R = 300, 8, 1024
    X, y, Xs = synth(N, d, R, seed=31)
    m = build(bohip, "Mat52Ard", X, y, np.full(d, -0.4))
    js = m.sample_joint(Xs.T, 8, 5)
    print("raw winners:", js.best_idx.tolist())
    assert len(set(js.best_idx.tolist())) < 8                           # (the case is chosen for this)
    picks = _distinct_picks(js.samples)
    np.testing.assert_array_equal(picks, distinct_picks(js.samples))
    assert len(set(picks.tolist())) == 8 and picks.min() >= 0
    np.testing.assert_array_equal(picks[:3], js.best_idx[:3])
    xs = np.asfortranarray(Xs.T)
    vals, Xq = bohip.acquire_thompson_batch(m, np.zeros(d), np.ones(d), 8, {"xs": xs}, rng=np.random.default_rng(1))
    assert Xq.shape == (d, 8) and len(vals) == 8
    cols = [int(np.flatnonzero(np.all(xs == Xq[:, [j]], axis=0))[0]) for j in range(8)]   # columns of xs ...
    assert len(set(cols)) == 8                                                              # ... all different
    m.close()


def test_acquire_max_joint_option_returns_a_candidate(bohip):
    from bohip.utils import latin_hypercube_sampling

    X, y, _ = synth(150, 2, 1, seed=3)
    m = build(bohip, "SEArd", X, y, np.full(2, -0.4))
    opts = {"method": "LN_COBYLA", "restarts": 2, "maxeval": 300, "joint": True}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f, x = bohip.acquire_max(bohip.ThompsonSamplingSimple(), m, [0.0, 0.0], [1.0, 1.0], opts, rng=np.random.default_rng(11))
    rng = np.random.default_rng(11)                                     # replay the candidate sets the call drew
    found = False
    for _ in range(2):
        starts = latin_hypercube_sampling(np.zeros(2), np.ones(2), 300, rng)
        rng.integers(0, 2 ** 63 - 1)
        found = found or bool(np.any(np.all(starts == x[:, None], axis=0)))
    assert found and np.isfinite(f)
    m.close()


def test_branin_thompson_batches(bohip):
    """BOpt(batchsize = 4) with ThompsonSamplingSimple: every iteration appends 4 distinct points."""
    from test_bo_loop_gpu import make_opt

    bo = bohip
    model = bo.ElasticGPE(2, mean=bo.MeanConst(-10.0), kernel=bo.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=200)
    batches = 5
    opt = make_opt(bo, model, bo.ThompsonSamplingSimple(), maxiterations=10 + batches, batchsize=4, batchoptions={"candidates": 512})
    bo.boptimize_(opt)
    assert len(model.y) == 10 + 4 * batches
    for b in range(batches):
        cols = model.x[:, 10 + 4 * b: 14 + 4 * b]
        assert len({tuple(c) for c in cols.T}) == 4
    model.close()
