"""d = 17 ... 64, the two widest dimension buckets (DT = 32, 64) and the DMAX = 64 edge, on every route that dispatches on d.

Inputs: tests/high_dim_inputs.py (length-scales that grow like sqrt(d); tests/test_high_dim_host.py shows on the CPU that a
dropped coordinate moves mu and sigma^2 by >= 100 x the tolerances below).  References: the NumPy twin
(tests/matern_reference.py) for all kernels, the C oracle for the three it has and for the N = 1500 / 1600 models.

Every tolerance is the one the named existing test applies to the same quantity:
  factor, alpha, mu, sigma^2, scores, arg-max   test_parity_gpu.test_seeded_vs_oracle (with its near-tie exemption)
  LogEI scores                                  test_logei_gpu.test_scores_on_every_route (8 x the twin's worst error)
  gradients                                     test_parity_gpu.test_score_grad_vs_oracle, the variance mask of
                                                test_split_k_path_vs_oracle_and_whole_k where the model is large
  split-K against whole-K                       test_parity_gpu.test_split_k_path_vs_oracle_and_whole_k
  posterior covariance                          test_parity_gpu.test_full_posterior_covariance_vs_oracle
  joint-draw factor                             test_joint_gpu.factor_bound, on the device's own Sigma
  knowledge gradient                            test_kg_gpu.check_against_twin
  marginal likelihood                           test_parity_gpu.test_mll_gradient_vs_oracle, test_fit_gpu.check_row
  ascent                                        test_parity_gpu.test_device_ascent_matches_host_restatement
  sample paths                                  path_reference's value_bound / grad_bound / frequencies_tol / normal_tol
  append                                        test_parity_gpu.test_incremental_append_is_used_and_matches_refit

The route of every call is read from the stage labels of enable_timing (bohip.hip t_begin), never inferred from the shape.
Lines starting with "HD" print the worst observed share of each tolerance (pytest -s).
"""
import functools
import math

import numpy as np
import pytest

import high_dim_inputs as hd
import logei_reference as lr
import path_reference as pr
from conftest import var_tol
from high_dim_inputs import BETA, LNOISE, LSIG, N0, S2F
from matern_reference import MaternGP, acq_value, first_argmax
from test_parity_gpu import bohip, check_scores, mu_floor  # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
DEV = 8.0   # test_logei_gpu.DEV


def build(bohip, kern, X, y, capacity=None):
    d = X.shape[1]
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(BETA), kernel=getattr(bohip, kern)(hd.loglen_of(kern, d), LSIG), logNoise=LNOISE,
                         capacity=capacity or len(y))
    m.append_(X.T, y)
    m.enable_timing(True)
    return m


def labels(m):
    """stage labels of the handle's last call"""
    return [name for name, _ in m.timing(cap=4096)]


SMALL, WHOLE, SPLIT = ("small_V", "small_V+U"), ("trigemm_sq", "trigemm_sq+V", "gemm_U"), ("split_V", "split_U")


def assert_route(m, must, never=()):
    lab = labels(m)
    assert all(x in lab for x in must) and not any(x in lab for x in never), (lab, must, never)


def note(what, d, err, tol):
    share = float(np.max(np.asarray(err) / np.maximum(np.asarray(tol), 1e-300))) if np.size(err) else 0.0
    print(f"HD d={d} {what}: worst share of the tolerance {share:.3e}")
    return share


def oracle_ll(kern, d):
    ll = hd.loglen_of(kern, d)
    return float(ll[0]) if kern == "SEIso" else ll


# ---- 1. factor, alpha, posterior and scores per route ------------------------------------------------------------------------------
_EXEMPT = []   # (kernel, d, R, acquisition) that took the near-tie exemption in this run; bounded from the twin alone below


@pytest.mark.parametrize("kern,d", hd.PAIRS + [hd.PAIR_63])
def test_scores_small_route_and_whole_k(bohip, orc, kern, d):
    c, ref, mu_r, var_r = hd.twin_case(kern, d)
    X, y, Xs = c["X"], c["y"], c["Xs"]
    m = build(bohip, kern, X, y)
    refs = [("twin", ref.L, ref.alpha, mu_r, var_r, lambda acq, p, R: acq_value(acq, p, mu_r[:R], var_r[:R]))]
    if kern in hd.ORACLE_KERNELS:
        ll = oracle_ll(kern, d)
        L, alpha = orc.fit(X, y, ll, LSIG, LNOISE, BETA, kern=kern)
        mu_o, var_o = orc.predict(X, ll, LSIG, BETA, L, alpha, Xs, kern=kern, nthreads=8)
        refs.append(("oracle", L, alpha, mu_o, var_o,
                     lambda acq, p, R: orc.score(X, ll, LSIG, BETA, L, alpha, acq, p, Xs[:R], kern=kern, nthreads=8)[0]))
    Lg, ag = m.factor(), m.alpha()
    for name, L, alpha, _, _, _ in refs:
        np.testing.assert_allclose(Lg, L, rtol=1e-9, atol=1e-11 * math.sqrt(S2F), err_msg=name)
        np.testing.assert_allclose(ag, alpha, rtol=1e-6, atol=1e-9 * np.abs(alpha).max(), err_msg=name)
    Rs = [R for k_, d_, R in hd.score_cases() if (k_, d_) == (kern, d)]
    for R in Rs:
        xs = np.asfortranarray(Xs[:R].T)
        mu, var = m.predict_f(xs)
        for name, _, alpha, mu_ref, var_ref, score_ref in refs:
            fl = mu_floor(alpha, S2F)
            mu_ref, var_ref = mu_ref[:R], var_ref[:R]
            note(f"{kern} R={R} mu vs {name}", d, np.abs(mu - mu_ref), 1e-6 * np.abs(mu_ref) + fl)
            note(f"{kern} R={R} sigma^2 vs {name}", d, np.abs(var - var_ref), var_tol(var_ref, N0, S2F))
            assert np.all(np.abs(mu - mu_ref) <= 1e-6 * np.abs(mu_ref) + fl), (name, R)
            assert np.all(np.abs(var - var_ref) <= var_tol(var_ref, N0, S2F)), (name, R)
            for acq in hd.ACQS:
                p = hd.acq_params(acq, y, d, N0)
                sc, bv, bi = m.score(acq, p, xs)
                if R <= 256:   # the small route: values, scores and the record in k_small_v
                    assert_route(m, ["small_V"], WHOLE + SPLIT + ("kstar", "score"))
                else:          # the fused whole-K pass: no k_score launch, no split-K planes
                    assert_route(m, ["kstar", "trigemm_sq"], SMALL + SPLIT + ("score",))
                sc_ref = score_ref(acq, p, R)
                floor = hd.score_floor(acq, p, fl, var_ref, N0, S2F)
                note(f"{kern} R={R} {acq} vs {name}", d, np.abs(sc - sc_ref), 1e-6 * np.abs(sc_ref) + floor)
                check_scores(sc, sc_ref, floor)
                if not hd.near_tie(sc_ref, floor):
                    assert bi == first_argmax(sc_ref)[1], (name, acq, R, bi)
                elif name == "twin":
                    _EXEMPT.append((kern, d, R, acq))
                assert sc[bi] == bv and (bv, bi) == first_argmax(sc)
        # LogEI on the device's own posterior (the functor's twin), as test_logei_gpu.test_scores_on_every_route
        for shift in (0.0, 5.0):
            tau = float(np.median(y)) + shift
            sc, bv, bi = m.score("LogEI", [tau], xs)
            assert_route(m, *((["small_V"], WHOLE + SPLIT) if R <= 256 else (["kstar", "trigemm_sq"], SMALL + SPLIT + ("score",))))
            lr.assert_close("value", sc, lr.logei(mu, var, tau)[0], DEV, f"{kern} d={d} R={R} LogEI tau+{shift}")
            assert bi == int(np.argmax(sc)) and np.float64(bv).tobytes() == sc[bi].tobytes()
    print(f"HD d={d} {kern}: arg-max exemptions in this run so far {len(_EXEMPT)}")
    m.close()


def test_argmax_exemptions_are_rare():
    """The exemption criterion looks at the twin's scores only, so it is recomputed here from the same cases (no module state: it
    holds under -k too); what this run exempted must be among them."""
    exempt, total = hd.reference_exemptions()
    print(f"HD arg-max exemptions: {len(exempt)} of {total} (case, acquisition) pairs; taken in this run: {len(_EXEMPT)}")
    assert 10 * len(exempt) <= total, exempt
    assert set(_EXEMPT) <= set(exempt)


# ---- the large SEArd models: oracle fits once per module ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large(N, d, R):
    from oracle.oracle import COracle

    orc = COracle()
    c = hd.hd_case(N, d, R, seed=N + d)
    ll = hd.loglen_ard(d)
    L, alpha = orc.fit(c["X"], c["y"], ll, LSIG, LNOISE, BETA)
    return c["X"], c["y"], c["Xs"], ll, L, alpha


@pytest.fixture(scope="module")
def large():
    return _large


@pytest.mark.parametrize("d", [33, 64])
def test_split_k_scores_and_gradients(bohip, orc, large, d):
    """N = 1500, R = 300: the contraction cut into slices (k_gemm_nt over slices + k_split_combine_v / u), k_score and
    k_grad_finish<DT> as launches of their own; against the oracle and against the whole-K schedule through the batch hint."""
    N, R = 1500, 300
    X, y, Xs, ll, L, alpha = large(N, d, R)
    m = build(bohip, "SEArd", X, y)
    np.testing.assert_allclose(m.factor(), L, rtol=1e-9, atol=1e-11 * math.sqrt(S2F))
    np.testing.assert_allclose(m.alpha(), alpha, rtol=1e-6, atol=1e-9 * np.abs(alpha).max())
    fl = mu_floor(alpha, S2F)
    mu_o, var_o = orc.predict(X, ll, LSIG, BETA, L, alpha, Xs, nthreads=8)
    mu, var = m.predict_f(Xs.T)
    assert np.all(np.abs(mu - mu_o) <= 1e-6 * np.abs(mu_o) + fl)
    assert np.all(np.abs(var - var_o) <= var_tol(var_o, N, S2F))
    note("SEArd split-K mu", d, np.abs(mu - mu_o), 1e-6 * np.abs(mu_o) + fl)
    note("SEArd split-K sigma^2", d, np.abs(var - var_o), var_tol(var_o, N, S2F))
    for acq in hd.ACQS:
        p = hd.acq_params(acq, y, d, N)
        sc, bv, bi = m.score(acq, p, Xs.T)
        assert_route(m, ["kstar", "split_V", "score"], SMALL + WHOLE)
        sc_o, _, bi_o = orc.score(X, ll, LSIG, BETA, L, alpha, acq, p, Xs, nthreads=8)
        floor = hd.score_floor(acq, p, fl, var_o, N, S2F)
        note(f"SEArd split-K {acq}", d, np.abs(sc - sc_o), 1e-6 * np.abs(sc_o) + floor)
        check_scores(sc, sc_o, floor)
        if not hd.near_tie(sc_o, floor):
            assert bi == bi_o, (acq, bi, bi_o)
        assert sc[bi] == bv and (bv, bi) == first_argmax(sc)
    # values and gradients as test_split_k_path_vs_oracle_and_whole_k: the oracle on a 120-candidate subset
    sc, g = m.score_grad("UCB", [2.0], Xs.T)
    assert_route(m, ["kstar", "split_V", "split_U", "score+grad"], SMALL + WHOLE)
    sub = np.random.default_rng(1).choice(R, 120, replace=False)
    sc_o, g_o = orc.score_grad(X, ll, LSIG, BETA, L, alpha, "UCB", [2.0], Xs[sub])
    floor = fl + 2.0 * np.sqrt(var_tol(var_o[sub], N, S2F, rel=0))
    check_scores(sc[sub], sc_o, floor)
    good = var_o[sub] > 1e3 * var_tol(var_o[sub], N, S2F)
    assert good.sum() >= 100
    scale = np.abs(g_o).max()
    note("SEArd split-K UCB gradient (R = 300: untiled k_grad_finish, S = 1)", d, np.abs(g.T[sub][good] - g_o[good]),
         1e-6 * np.abs(g_o[good]) + 1e-9 * scale + 1e-12)
    np.testing.assert_allclose(g.T[sub][good], g_o[good], rtol=1e-6, atol=1e-9 * scale + 1e-12)
    sv, bv, bi = m.score("UCB", [2.0], Xs.T)
    np.testing.assert_array_equal(sv, sc)                                  # value path == gradient path, bit for bit
    assert bi == int(np.argmax(sv)) and bv == sv[bi]
    np.testing.assert_array_equal(m.score("UCB", [2.0], Xs[40:R - 3].T)[0], sv[40:R - 3])   # batch-independent (same schedule)
    m.set_batch_hint(1 << 20)                                              # whole-K schedule
    sw, gw = m.score_grad("UCB", [2.0], Xs.T)
    assert_route(m, ["kstar", "trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT)
    m.set_batch_hint(0)
    np.testing.assert_allclose(sc, sw, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(g, gw, rtol=1e-7, atol=1e-10 * np.abs(gw).max())
    m.close()


@pytest.mark.parametrize("kern,d", [("SEArd", 33), ("Mat32Ard", 64)])
def test_pruned_value_only_record(bohip, kern, d):
    """N = 300, R = 257: the smallest shape of tests/test_prune_select_gpu.py that prunes (three row tiles; R > 256).  k_kstar<DT> writes
    the partial sums the bounds are made of.  The record equals the first arg-max of the full-score call, which is held to the twin."""
    from test_prune_select_gpu import assert_record, value_only

    N, R = 300, 257
    c, ref, mu_r, var_r = hd.twin_case(kern, d, N, R)
    fl = mu_floor(ref.alpha, S2F)
    for acq in ("EI", "UCB"):
        m = build(bohip, kern, c["X"], c["y"])                             # (a handle of its own: the back-off after a long round 2)
        p = hd.acq_params(acq, c["y"], d, N)
        sc, v_full, i_full = m.score(acq, p, c["Xs"].T, want_scores=True)
        assert_route(m, ["kstar", "trigemm_sq"], SMALL + SPLIT + ("score",))
        check_scores(sc, acq_value(acq, p, mu_r, var_r), hd.score_floor(acq, p, fl, var_r, N, S2F))
        assert (v_full, i_full) == first_argmax(sc)
        v, i, n2 = value_only(m, acq, p, c["Xs"])                           # asserts that the pruned pass ran
        print(f"HD d={d} {kern} {acq}: pruned pass, round 2 listed {n2} of {R - 64}")
        assert_record(v, i, v_full, i_full, (kern, d, acq))
        m.close()


# ---- 2. gradients ----------------------------------------------------------------------------------------------------------------------
def logei_grad_ref(ref, Xs, tau):
    """twin partials x the twin's grad mu and grad sigma^2 (test_logei_gpu.test_gradient_is_the_chain_rule)"""
    post = [ref.posterior_grad(x) for x in Xs]
    mu, s2 = np.array([q[0] for q in post]), np.array([q[1] for q in post])
    _, a, b = lr.logei(mu, s2, tau)
    return a[:, None] * np.array([q[2] for q in post]) + b[:, None] * np.array([q[3] for q in post])


@pytest.mark.parametrize("kern,d", hd.PAIRS)
def test_score_grad(bohip, orc, kern, d):
    """R = 7, 70 (and 32 at d = 64: the pinned block's gradient area exactly full): k_small_u<DT> / k_small_u_logei64.
    R = 300: k_grad_finish<32|64>, the untiled form (the tiled one exists for DT <= 16 only), one workgroup per candidate."""
    c, ref, _, _ = hd.twin_case(kern, d)
    X, y, Xs = c["X"], c["y"], c["Xs"]
    m = build(bohip, kern, X, y)
    floor = mu_floor(ref.alpha, S2F)
    tau = float(np.median(y))
    g_refs = {"UCB": ref.score_grad("UCB", [2.5], Xs), "LogEI": (None, logei_grad_ref(ref, Xs, tau))}
    if kern in hd.ORACLE_KERNELS:
        ll = oracle_ll(kern, d)
        L, alpha = orc.fit(X, y, ll, LSIG, LNOISE, BETA, kern=kern)
        g_refs["UCB (oracle)"] = orc.score_grad(X, ll, LSIG, BETA, L, alpha, "UCB", [2.5], Xs, kern=kern)
    for R in (7, 70, 300) + ((32,) if d == 64 else ()):
        xs = np.asfortranarray(Xs[:R].T)
        for what, (sc_r, g_r) in g_refs.items():
            acq, p = (("LogEI", [tau]) if what == "LogEI" else ("UCB", [2.5]))
            sc, g = m.score_grad(acq, p, xs)
            assert_route(m, *((["small_V+U"], WHOLE + SPLIT) if R <= 256 else (["trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT)))
            assert g.shape == (d, R)
            if sc_r is not None:
                np.testing.assert_allclose(sc, sc_r[:R], rtol=1e-6, atol=floor + 1e-12)
            scale = np.abs(g_r[:R]).max()
            note(f"{kern} R={R} gradient {what}", d, np.abs(g.T - g_r[:R]), 1e-6 * np.abs(g_r[:R]) + 1e-9 * scale + 1e-12)
            np.testing.assert_allclose(g.T, g_r[:R], rtol=1e-6, atol=1e-9 * scale + 1e-12, err_msg=f"{what} R={R}")
            np.testing.assert_array_equal(sc, m.score(acq, p, xs)[0])      # value path and gradient path agree bit for bit
    m.close()


def test_score_grad_with_the_observations_split_over_two_workgroups(bohip, orc, large):
    """N = 1600, d = 64: k_grad_finish<64> with S = min(16, N / 768) = 2 workgroups per candidate, so the dgparts rows
    [candidate][slice][2 DMAX] are written at full width.  R = 40 on its own takes the small route at this N (small_limit = 176),
    where no k_grad_finish runs: checked as such, then pushed onto the whole-K schedule by the batch hint (R <= SMALL_MAX keeps
    S = 2); R = 200 reaches the same kernel on the split-K schedule without a hint."""
    N, d = 1600, 64
    X, y, Xs, ll, L, alpha = large(N, d, 200)
    m = build(bohip, "SEArd", X, y)
    assert N // 768 == 2
    fl = mu_floor(alpha, S2F)
    sc_o, g_o = orc.score_grad(X, ll, LSIG, BETA, L, alpha, "UCB", [2.0], Xs)
    _, var_o = orc.predict(X, ll, LSIG, BETA, L, alpha, Xs, nthreads=8)
    good = var_o > 1e3 * var_tol(var_o, N, S2F)
    assert good[:40].sum() >= 30
    scale = np.abs(g_o).max()
    for R, hint, want, never in ((40, 0, ["small_V+U"], WHOLE + SPLIT), (40, 1 << 20, ["trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT),
                                 (200, 0, ["split_V", "split_U", "score+grad"], SMALL + WHOLE)):
        m.set_batch_hint(hint)
        sc, g = m.score_grad("UCB", [2.0], Xs[:R].T)
        assert_route(m, want, never)
        m.set_batch_hint(0)
        check_scores(sc, sc_o[:R], fl + 2.0 * np.sqrt(var_tol(var_o[:R], N, S2F, rel=0)))
        gd, gr = g.T[good[:R]], g_o[:R][good[:R]]
        note(f"SEArd N=1600 R={R} hint={hint} UCB gradient", d, np.abs(gd - gr), 1e-6 * np.abs(gr) + 1e-9 * scale + 1e-12)
        np.testing.assert_allclose(gd, gr, rtol=1e-6, atol=1e-9 * scale + 1e-12, err_msg=f"R={R} hint={hint}")
    m.close()


# ---- 3. covariance routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d,R", [("SEIso", 17, 129), ("Mat32Iso", 32, 257), ("Mat32Ard", 33, 129), ("SEArd", 64, 257), ("Mat12Iso", 64, 129)])
def test_predict_cov_and_joint_factor(bohip, kern, d, R):
    """k_post_cov<DT> (predict_cov) against the twin; k_sample_cov<DT> + the factorisation of sample_joint against the device's own
    Sigma + jitter I."""
    c, ref, _, _ = hd.twin_case(kern, d)
    Xs = c["Xs"][:R]
    m = build(bohip, kern, c["X"], c["y"])
    mu_r, cov_r = ref.predict_cov(Xs)
    mu, cov = m.predict_cov(Xs.T)
    assert "post_cov" in labels(m), labels(m)
    note(f"{kern} R={R} predict_cov", d, np.abs(cov - cov_r), var_tol(cov_r, N0, S2F))
    np.testing.assert_allclose(mu, mu_r, rtol=1e-6, atol=mu_floor(ref.alpha, S2F))
    assert np.all(np.abs(cov - cov_r) <= var_tol(cov_r, N0, S2F)), np.abs(cov - cov_r).max()
    np.testing.assert_array_equal(cov, cov.T)
    _, var = m.predict_f(Xs.T)
    pos = np.diag(cov) > 0
    assert np.all(np.abs(np.diag(cov)[pos] - var[pos]) <= var_tol(var[pos], N0, S2F))
    js = m.sample_joint(Xs.T, 3, seed=d + R, want_factor=True)
    assert "sample_cholesky" in labels(m), labels(m)
    np.testing.assert_array_equal(js.mu, mu)                               # predict_cov's mean, bit for bit
    C = js.factor
    assert np.all(np.diag(C) > 0) and not np.any(np.triu(C, 1))
    res = np.abs(C @ C.T - (cov + js.jitter * np.eye(R)))
    bound = var_tol(cov, N0, S2F) + 64 * R * EPS * (float(np.max(np.diag(cov))) + js.jitter)   # test_joint_gpu.factor_bound
    note(f"{kern} R={R} joint factor (jitter {js.jitter:.1e}, tries {js.tries})", d, res, bound)
    assert np.all(res <= bound)
    m.close()


@pytest.mark.parametrize("kern,d", [("Mat32Iso", 32), ("Mat52Ard", 64)])
def test_kg(bohip, kern, d):
    """bohip_gp_kg, R = 130: its own k_post_cov<DT> call site; the march against the twin on the device's Sigma."""
    import kg_reference as kr
    from test_kg_gpu import check_against_twin

    R = 130
    c, ref, _, _ = hd.twin_case(kern, d)
    xs = np.asfortranarray(c["Xs"][:R].T)
    m = build(bohip, kern, c["X"], c["y"])
    mu, cov = m.predict_cov(xs)
    res = m.kg(xs)
    lab = labels(m)
    assert "post_cov" in lab and "kg" in lab, lab
    assert res.mu.tobytes() == mu.tobytes()                                 # mu is predict_cov's, bit for bit
    nu = math.exp(2.0 * LNOISE) + EPS
    out = [kr.kg_march(mu, cov[e] / math.sqrt(cov[e, e] + nu)) for e in range(R)]
    tkg, tseg = np.array([v for v, _ in out]), np.array([n for _, n in out], dtype=np.int32)
    check_against_twin(res.values, res.nseg, tkg, tseg, f"{kern} d = {d} R = E = {R}")
    assert res.best_idx == int(np.argmax(tkg)) and res.best_val == res.values[res.best_idx]
    mu_r, cov_r = ref.predict_cov(c["Xs"][:R])                              # ... and that Sigma is the twin's
    assert np.all(np.abs(cov - cov_r) <= var_tol(cov_r, N0, S2F))
    m.close()


# ---- 4. marginal likelihood --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d", [("Mat12Ard", 17), ("SEArd", 33), ("Mat52Ard", 64), ("Mat12Iso", 64)])
def test_mll_gradient(bohip, orc, kern, d):
    """bohip_gp_mll_grad: k_dmll_parts<DT>; at d = 64 the row red[4][DMAX + 3] and the host's hbuf[DMAX + 4] are exactly full."""
    c, ref, _, _ = hd.twin_case(kern, d)
    m = build(bohip, kern, c["X"], c["y"])
    mll, dn, dm, dk = m.mll_grad()
    m.synchronize()                                                         # (collects the call's stage labels)
    assert_route(m, ["kinv", "dmll_reduce"])
    g = np.concatenate([[dn, dm], dk])
    mr_, dnr, dmr, dkr = ref.mll_grad()
    refs = [("twin", mr_, np.concatenate([[dnr, dmr], dkr]))]
    if kern in hd.ORACLE_KERNELS:
        refs.append(("oracle",) + tuple(orc.mll_grad(c["X"], c["y"], oracle_ll(kern, d), LSIG, LNOISE, BETA, kern=kern)))
    assert dk.size == (2 if kern.endswith("Iso") else d + 1)
    for name, mll_ref, g_ref in refs:
        note(f"{kern} mll_grad vs {name}", d, np.abs(g - g_ref), 1e-6 * np.abs(g_ref) + 1e-8 * np.abs(g_ref).max())
        assert mll == pytest.approx(mll_ref, rel=1e-9), name
        np.testing.assert_allclose(g, g_ref, rtol=1e-6, atol=1e-8 * np.abs(g_ref).max(), err_msg=name)
    assert mll == m.mll()
    m.close()


@pytest.mark.parametrize("kern", ["SEArd", "Mat52Ard"])   # one LOW and one standard instantiation of the fit kernel
def test_mll_grad_batch_at_dmax(bohip, kern):
    """(N, d) = (64, 64), three settings: kernels_fit.hip's red 8 x (DMAX + 3) exactly full.  Settings around the recipe's
    hyper-parameters (those of tests/test_fit_gpu.py sit at ll = -0.6, where K is the identity at this d)."""
    from test_fit_gpu import check_row, twin

    N, d = 64, 64
    c = hd.hd_case(N, d, 1, seed=164)
    m = build(bohip, kern, c["X"], c["y"])
    centre = np.concatenate([[LNOISE, BETA], hd.loglen_of(kern, d), [LSIG]])
    Theta = centre + np.random.default_rng(N + d).uniform(-0.3, 0.3, (3, centre.size))
    assert m.mll_batch_dims() == (d + 3, 512)
    mll, G, piv = m.mll_grad_batch(Theta)
    assert np.all(piv == 0) and G.shape == Theta.shape
    for h in range(3):
        check_row(mll[h], G[h], *twin(kern, c["X"], c["y"], Theta[h]), f"{kern} N={N} d={d} row {h}")
    m.close()


# ---- 5. ascent ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d", hd.ASCENT_PAIRS)
def test_ascent(bohip, kern, d):
    """d = 16: k_ascent_wg<16> with DT == d (and k_ascent_wg_logei16); d = 17: use_wg is false for every d > 16, the batched driver
    (k_small_v / k_small_u<32> + k_asc_step) is the only ascent; d = 64: the same with asc_bounds (3 DMAX) and every state row full."""
    from bohip.acquisition import _batched_lbfgs_ascent

    c, ref, _, _ = hd.twin_case(kern, d)
    y = c["y"]
    m = build(bohip, kern, c["X"], y)
    lb, ub = np.zeros(d), np.ones(d)
    R, maxeval = 10, 1000
    # tau = min y: EI is alive at every start.  With a higher incumbent some starts sit where EI ~ 1e-20 at d = 64 and creep under the
    # relative stopping test until maxeval (seen on the twin with the host restatement), and neither driver stops on its own
    tau = float(np.min(y))
    starts = np.asfortranarray(np.random.default_rng(d).random((d, R)) * 1.4 - 0.2)      # partly outside the box
    assert np.any(starts < 0) and np.any(starts > 1)
    clipped = np.asfortranarray(np.clip(starts, 0.0, 1.0))
    acqs = [("UCB", [2.0]), ("EI", [tau])] + ([("LogEI", [tau])] if d == 16 else [])
    for acq, p in acqs:
        f0, _ = m.score_grad(acq, p, clipped)
        f, Xb, bf, bi, bx, ev = m.ascend(acq, p, lb, ub, starts, maxeval=maxeval)
        lab = labels(m)
        if d <= 16:
            assert "ascent_wg" in lab and "small_V+U" not in lab, lab
        else:
            assert "ascent_wg" not in lab and "small_V+U" in lab, lab
        calls = [0]

        def fg(Z):
            calls[0] += 1
            return m.score_grad(acq, p, Z)

        fh, Xh = _batched_lbfgs_ascent(fg, starts, lb, ub, maxeval)
        print(f"HD d={d} {kern} {acq}: device passes {ev}, host passes {calls[0]}, best {bf:.6g}, "
              f"worst |f - f_host| / max(|f_host|, 1e-3) {np.max(np.abs(f - fh) / np.maximum(np.abs(fh), 1e-3)):.2e}")
        assert 1 <= ev < maxeval and calls[0] < maxeval                     # both drivers stopped on their own
        assert np.all(f >= f0 - 1e-12) and np.all(Xb >= lb[:, None]) and np.all(Xb <= ub[:, None])
        fchk, _ = m.score_grad(acq, p, Xb)
        np.testing.assert_allclose(fchk, f, rtol=1e-9, atol=1e-12)          # the returned value is the score at the returned point
        np.testing.assert_allclose(f, fh, rtol=1e-5, atol=1e-8)             # same maxima as the host restatement
        # ... and, beyond the restated assertions, the TWIN's score there (test_score_grad_vs_oracle's bound on a score): the checks
        # above compare the device with itself and cannot see a posterior that is wrong in every kernel alike
        f_twin = lr.logei(*ref.predict(Xb.T), p[0])[0] if acq == "LogEI" else ref.score(acq, p, Xb.T)
        np.testing.assert_allclose(f, f_twin, rtol=1e-6, atol=mu_floor(ref.alpha, S2F) + 1e-12)
        j = int(np.argmax(f))                                               # first maximum wins
        assert bi == j and bf == f[j]
        np.testing.assert_array_equal(bx, Xb[:, j])
    m.close()


# ---- 6. sample paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["Mat32Ard", "SEArd"])
def test_sample_paths_at_dmax(bohip, kern):
    """d = 64: x_l[PR_CAND][DMAX], x_l[DMAX] and PathLen::inv[DMAX] of kernels_path.hip are exactly full.  S = 3: the row form,
    S = 64: the MFMA form; M = 16, the smallest tests/test_path_gpu.py uses above N = 100."""
    d, M, seed = 64, 16, 4321
    c, _, _, _ = hd.twin_case(kern, d)
    X, y = c["X"], c["y"]
    ll = hd.loglen_of(kern, d)
    m = build(bohip, kern, X, y)
    tw = pr.PathTwin(kern, X, y, ll, LSIG, LNOISE, BETA, M, seed)
    om_twin = tw.Om
    worst = {}

    def share(name, frac):
        worst[name] = max(worst.get(name, 0.0), float(np.max(frac)))

    for S in (3, 64):
        with m.draw_paths(S, M, seed) as p:
            assert any(name.startswith("path_") for name in labels(m)), labels(m)
            assert (p.S, p.M, p.N, p.dim) == (S, M, N0, d)
            for R in (1, 129):
                xs = c["Xs"][:R]
                vals, bv, bi = p.eval(xs.T)
                assert_route(m, ["path_eval"])
                assert vals.shape == (S, R)
                np.testing.assert_array_equal(bi, np.argmax(vals, axis=1))
                np.testing.assert_array_equal(bv, vals[np.arange(S), bi])
                for s in sorted({0, S // 2, S - 1}):
                    om, w, u = p.coef(s)
                    share("omega", np.abs(om - om_twin) / pr.frequencies_tol(kern, ll, d, M // 2, seed))
                    tw.Om = om                                               # the twin with the device's own coefficients
                    wt = tw.w(s)
                    share("w", np.abs(w - wt) / pr.normal_tol(wt))
                    share("values", np.abs(vals[s] - tw.value(xs, u, w)) / tw.value_bound(xs, u, w))
                    f, g = p.eval_grad(xs.T, np.full(R, s))
                    assert_route(m, ["path_grad"])
                    share("grad values", np.abs(f - tw.value(xs, u, w)) / tw.value_bound(xs, u, w))
                    share("gradients", np.abs(g.T - tw.grad(xs, u, w)) / tw.grad_bound(xs, u, w))
    print(f"HD d={d} {kern} paths: worst fraction of each bound: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
    m.close()


# ---- 7. append at the staging edge -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["SEArd", "Mat32Ard"])
def test_append_at_the_staging_edge(bohip, kern):
    """d = 64 from N = 100.  32 points in one call: 32 x 64 = SMALL_R x DMAX, the pinned stage exactly full, and the largest
    batch the incremental extension takes (APPEND_PMAX = 32).  33 points: past both, a pageable copy and a refit.  After
    either the factor and alpha are those of a model built from scratch."""
    from bohip import _lib

    d = 64
    c = hd.hd_case(165, d, 40, seed=65)
    X, y, Xs = c["X"], c["y"], c["Xs"]
    ll = hd.loglen_of(kern, d)
    m = build(bohip, kern, X[:100], y[:100], capacity=256)                    # (room for both appends: no growth, no re-upload)
    refits0, appends0 = m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS)
    for n0, n1 in ((100, 132), (132, 165)):
        m.append_(X[n0:n1].T, y[n0:n1])
        lab = labels(m)
        if n1 - n0 <= 32:
            assert m.info(_lib.INFO_REFITS) == refits0 and m.info(_lib.INFO_APPENDS) == appends0 + 1
            assert "append_cov_rows" in lab and "append_L21" in lab and "build_cov" not in lab, lab
        else:
            assert m.info(_lib.INFO_REFITS) == refits0 + 1 and m.info(_lib.INFO_APPENDS) == appends0 + 1
            assert "build_cov" in lab and "append_L21" not in lab, lab
        ref = MaternGP(kern, X[:n1], y[:n1], ll, LSIG, LNOISE, BETA)
        note(f"{kern} append to N={n1}: factor", d, np.abs(m.factor() - ref.L), 1e-9 * np.abs(ref.L) + 1e-12)
        np.testing.assert_allclose(m.factor(), ref.L, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(m.alpha(), ref.alpha, rtol=1e-7, atol=1e-10 * np.abs(ref.alpha).max())
        mu_r, var_r = ref.predict(Xs)
        mu, var = m.predict_f(Xs.T)
        np.testing.assert_allclose(mu, mu_r, rtol=1e-6, atol=mu_floor(ref.alpha, S2F))
        assert np.all(np.abs(var - var_r) <= var_tol(var_r, n1, S2F))
        np.testing.assert_array_equal(m.x, X[:n1].T)
    m.close()
