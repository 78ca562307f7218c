"""Replicated sites on the device (include/bohip_rep.h): r evaluations at one position as ONE row with noise nu / r.

References and bounds.  Every posterior and likelihood number of the collapsed handle is compared with the model that holds every
evaluation as a row of its own, by the suite's independent references (rep_reference.Expanded: the C oracle for SEArd, MaternGP for
Mat32Iso, which the C oracle does not have) at the suite's existing bounds: test_seeded_vs_oracle's for mu, sigma^2 and the scores,
1e-9 relative for mll, test_mll_gradient_vs_oracle's for its gradient.  Only L and alpha, whose shape differs, are compared with the
NumPy twin of cK_w (rep_reference.RepTwin), at test_seeded_vs_oracle's bounds for them; tests/test_rep_host.py holds that twin to the
expanded model and to np.longdouble, and shows that a twin without the weights misses these bounds a hundred times over.
Inputs: rep_reference (d = 3, SEArd and Mat32Iso, reps from {1 ... 5} with a quarter at 1, three (logNoise, log sigma_f) settings)."""
import ctypes as C
import math

import numpy as np
import pytest

import rep_reference as rr
from matern_reference import acq_value
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
CASES = [(kern, h) for kern in rr.KERNS for h in rr.HYPERS]


def new_handle(bohip, kern, hyp, capacity, **kw):
    ll, lsig, lnoise, beta = hyp
    m = bohip.ElasticGPE(rr.D, mean=bohip.MeanConst(beta), kernel=getattr(bohip, kern)(ll, lsig), logNoise=lnoise, capacity=capacity, **kw)
    m.enable_timing(True)
    return m


def labels(m):
    """stage labels of the handle's last append or refit"""
    return [n for n, _ in m.timing(cap=4096)]


def counters(m):
    from bohip import _lib

    return m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS), m.info(_lib.INFO_CAPACITY)


def xs_of(Xs, R):
    return np.asfortranarray(Xs[:R].T)


# ---- 1. identity: all reps = 1 on an unweighted handle IS append_ -------------------------------------------------------------------
@pytest.mark.parametrize("kern", rr.KERNS)
def test_sites_of_one_evaluation_are_plain_appends(bohip, kern):
    lnoise, lsig = rr.HYPERS[0]
    pos, _, evals, _ = rr.raw(127, lnoise, lsig)
    y = np.array([v[0] for v in evals])
    hyp = (rr.LL[kern], lsig, lnoise, rr.BETA)
    a, b = new_handle(bohip, kern, hyp, 100), new_handle(bohip, kern, hyp, 100)
    try:
        lo = 0
        for p in (90, 5, 32):                                               # a first fill, an incremental append, a growth
            x = np.asfortranarray(pos[lo:lo + p].T)
            a.append_(x, y[lo:lo + p])
            la = labels(a)
            b.append_sites_(x, y[lo:lo + p], np.ones(p, dtype=np.int64), np.zeros(p))
            assert labels(b) == la and "rep_diag" not in la, (p, la, labels(b))
            lo += p
            assert counters(a) == counters(b)
            assert a.factor().tobytes() == b.factor().tobytes() and a.alpha().tobytes() == b.alpha().tobytes()
            ga, gb = a.mll_grad(), b.mll_grad()
            assert ga[:3] == gb[:3] and ga[3].tobytes() == gb[3].tobytes() and a.mll() == b.mll()
            assert b.sites_info() == (lo, lo, 0.0, 0.0, 0) and not b.weighted and np.all(b.get_reps() == 1)
        assert counters(a) == (2, 1, 200)
        with pytest.raises(bohip.BohipError) as e:                          # nothing is stored on an argument error
            b.append_sites_(np.zeros((rr.D, 2)), [0.0, 0.0], [2, 1], [0.5, 0.25])
        assert e.value.code == -1 and "ss must be 0" in str(e.value) and b.nobs == 127 and b.sites_info()[0] == 127
        for reps, ss in (([0], [0.0]), ([2], [-1.0]), ([2], [np.nan]), ([2], [np.inf])):
            with pytest.raises(bohip.BohipError) as e:
                b.append_sites_(np.zeros((rr.D, 1)), [0.0], reps, ss)
            assert e.value.code == -1
        assert not b.weighted and b.factor().tobytes() == a.factor().tobytes()
    finally:
        a.close()
        b.close()


# ---- 2. the history ----------------------------------------------------------------------------------------------------------------------
def check_state(m, kern, hyp, pos, evals, Xs, n, what, orc):
    """L and alpha against the twin; mu, sigma^2, EI / UCB / PI at R = 40 (row-wise route, and the whole-K route by hint) and 700, mll
    and its gradient against the expanded reference."""
    ll, lsig, lnoise, beta = hyp
    _, ybar, reps, ss, ymax = rr.sites_of(pos, evals, 0, n)
    tw = rr.RepTwin(kern, pos[:n], ybar, reps, ss, ll, lsig, lnoise, beta)
    X, y = rr.expand(pos, evals, 0, n)
    ex = rr.Expanded(kern, X, y, ll, lsig, lnoise, beta, orc)
    s2f = ex.s2f
    np.testing.assert_allclose(m.factor(), tw.L, rtol=1e-9, atol=1e-11 * math.sqrt(s2f), err_msg=what)
    np.testing.assert_allclose(m.alpha(), tw.alpha, rtol=1e-6, atol=1e-9 * np.abs(tw.alpha).max(), err_msg=what)
    assert (m.nobs, m.nevals) == (n, len(y)) and np.array_equal(m.get_reps(), reps) and np.array_equal(m.reps, reps)
    ns, ne, sst, slr, w = m.sites_info()
    assert (ns, ne, w) == (n, len(y), int(np.any(reps > 1)))
    assert sst == pytest.approx(ss.sum(), rel=1e-12) and slr == pytest.approx(np.log(reps).sum(), rel=1e-12, abs=1e-300)
    import bohip as b_

    assert b_.maxy(m) == y.max() == ymax.max()
    tau = float(y.max())
    worst = {}
    for R, hint in ((40, 0), (40, 700), (700, 0)):
        m.set_batch_hint(hint)
        xs = xs_of(Xs, R)
        mu_o, var_o = ex.predict(Xs[:R])
        mu, var = m.predict_f(xs)
        e_mu, e_var = np.abs(mu - mu_o) / rr.mu_bound(mu_o, ex.alpha, s2f), np.abs(var - var_o) / rr.var_tol(var_o, ex.N, s2f)
        worst["mu"], worst["var"] = max(worst.get("mu", 0), e_mu.max()), max(worst.get("var", 0), e_var.max())
        assert e_mu.max() <= 1 and e_var.max() <= 1, (what, R, hint, e_mu.max(), e_var.max())
        for acq, p in (("EI", [tau]), ("UCB", [2.0]), ("PI", [tau])):
            sc_o = ex.score(acq, p, Xs[:R])
            sc, bv, bi = m.score(acq, p, xs)
            e_sc = np.abs(sc - sc_o) / rr.score_bound(acq, p, sc_o, var_o, ex.alpha, ex.N, s2f)
            worst[acq] = max(worst.get(acq, 0), e_sc.max())
            assert e_sc.max() <= 1 and sc[bi] == bv, (what, acq, R, hint, e_sc.max())
    m.set_batch_hint(0)
    mll_o, g_o = ex.mll_grad()
    mll, dn, dm, dk = m.mll_grad()
    g = np.concatenate([[dn, dm], dk])
    e_g = np.abs(g - g_o) / rr.grad_bound(g_o)
    worst["mll"], worst["grad"] = abs(mll - mll_o) / (rr.MLL_RTOL * abs(mll_o)), e_g.max()
    print(f"  {what}: n = {n}, N = {ex.N}; worst shares of the bounds: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["mll"] <= 1 and e_g.max() <= 1, (what, mll, mll_o, g, g_o)
    assert mll == m.mll()


@pytest.mark.parametrize("kern,h", CASES)
def test_history(bohip, orc, kern, h):
    lnoise, lsig = h
    pos, evals, Xs = rr.history_data(lnoise, lsig)
    hyp = (rr.LL[kern], lsig, lnoise, rr.BETA)
    m = new_handle(bohip, kern, hyp, rr.CAPACITY)
    try:
        for k, step in enumerate(rr.history_plan()):
            lo, n = step["lo"], step["n"]
            what = f"{kern} {h} step {k} ({step['kind']} {step['arg']})"
            if step["kind"] == "hyper":
                hyp = rr.hyper_after(kern, lnoise, lsig)
                m.set_params_(ll=hyp[0], lsigma=hyp[1], logNoise=hyp[2], beta=hyp[3])          # no fit_(): the next reader factors again
            else:
                x, ybar, reps, ss, ymax = rr.sites_of(pos, evals, lo, n)
                if step["kind"] == "plain":
                    assert np.all(reps == 1)
                    m.append_(x, ybar)
                else:
                    assert np.any(reps > 1)
                    m.append_sites_(x, ybar, reps, ss, ymax)
                lab = labels(m)
                if step["route"] == "incremental":
                    assert "append_cov_rows" in lab and "append_W21" in lab and "build_cov" not in lab, (what, lab)
                else:
                    assert "build_cov" in lab and "append_W21" not in lab, (what, lab)
                # the weighted diagonal follows the covariance build of either route, on a weighted handle only
                assert ("rep_diag" in lab) == step["weighted"], (what, lab)
                if step["weighted"]:
                    i = lab.index("rep_diag")
                    assert lab[i - 1] == ("append_cov_rows" if step["route"] == "incremental" else "build_cov"), (what, lab)
            assert m.weighted == step["weighted"]
            check_state(m, kern, hyp, pos, evals, Xs, n, what, orc)
            assert counters(m) == (step["refits"], step["appends"], step["cap"]), (what, counters(m), step)
    finally:
        m.close()


# ---- 3. the features that read the resident L, W, W', alpha ---------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=rr.KERNS)
def pair(request, bohip):  # noqa: F811
    """(collapsed handle, expanded handle, twin, X, y, Xs, hyp) on the (-2, 0) input at 130 sites."""
    kern = request.param
    lnoise, lsig = rr.HYPERS[0]
    pos, _, evals, Xs = rr.raw(130, lnoise, lsig)
    hyp = (rr.LL[kern], lsig, lnoise, rr.BETA)
    X, y = rr.expand(pos, evals)
    w, e = new_handle(bohip, kern, hyp, 130), new_handle(bohip, kern, hyp, len(y))
    sites = rr.sites_of(pos, evals)
    w.append_sites_(*sites)
    e.append_(X.T, y)
    tw = rr.RepTwin(kern, pos, *sites[1:4], *hyp)
    assert w.weighted and not e.weighted and w.nobs == 130 and e.nobs == len(y) == w.nevals
    yield w, e, tw, X, y, Xs, hyp
    w.close()
    e.close()


def floor_of(e, s2f):
    return 64 * EPS * s2f * np.abs(e.alpha()).sum()                         # test_parity_gpu.mu_floor


def test_score_grad(pair):
    w, e, tw, X, y, Xs, hyp = pair
    s2f, xs = math.exp(2 * hyp[1]), xs_of(Xs, 300)
    for acq, p in (("EI", [float(y.max())]), ("UCB", [2.0])):
        sw, gw = w.score_grad(acq, p, xs)
        se, ge = e.score_grad(acq, p, xs)
        assert np.all(np.abs(sw - se) <= 1e-6 * np.abs(se) + floor_of(e, s2f) + 1e-12)
        assert np.all(np.abs(gw - ge) <= 1e-6 * np.abs(ge) + 1e-9 * np.abs(ge).max() + 1e-12)
        assert np.abs(ge).max() > 0


def test_ascend(pair):
    """8 starts: the twin's score at the returned points."""
    w, e, tw, X, y, Xs, hyp = pair
    s2f = math.exp(2 * hyp[1])
    lb, ub = np.zeros(rr.D), np.ones(rr.D)
    starts = np.asfortranarray(np.random.default_rng(8).random((rr.D, 8)) * 1.4 - 0.2)
    for acq, p in (("UCB", [2.0]), ("EI", [float(np.min(y))])):
        f, Xb, bf, bi, bx, ev = w.ascend(acq, p, lb, ub, starts, maxeval=1000)
        assert 1 <= ev < 1000 and np.all(Xb >= lb[:, None]) and np.all(Xb <= ub[:, None])
        mu_t, var_t = tw.predict(Xb.T)
        f_twin = acq_value(acq, p, mu_t, var_t)
        assert np.all(np.abs(f - f_twin) <= 1e-6 * np.abs(f_twin) + floor_of(e, s2f) + 1e-12), (acq, f, f_twin)
        assert bi == int(np.argmax(f)) and bf == f[bi]


def test_predict_cov_and_sample_joint(pair):
    w, e, tw, X, y, Xs, hyp = pair
    s2f, R = math.exp(2 * hyp[1]), 200
    xs = xs_of(Xs, R)
    mu_w, cov_w = w.predict_cov(xs)
    mu_e, cov_e = e.predict_cov(xs)
    assert np.all(np.abs(mu_w - mu_e) <= 1e-6 * np.abs(mu_e) + floor_of(e, s2f))
    assert np.all(np.abs(cov_w - cov_e) <= rr.var_tol(cov_e, len(y), s2f))
    js = w.sample_joint(xs, 3, 77, want_factor=True)                        # the same seed on both: the factor against Sigma
    je = e.sample_joint(xs, 3, 77, want_factor=True)
    Cf = js.factor
    bound = rr.var_tol(cov_e, len(y), s2f) + 64 * R * EPS * (float(np.max(np.diag(cov_e))) + js.jitter)      # test_joint_gpu.factor_bound
    assert np.all(np.abs(Cf @ Cf.T - (cov_e + js.jitter * np.eye(R))) <= bound)
    assert js.mu.tobytes() == mu_w.tobytes() and js.samples.shape == je.samples.shape == (3, R)


def test_kg(pair):
    """E = 8, as test_lifecycle_gpu.test_kg: test_kg_gpu's twin on the handle's own posterior (TWIN_REL) and the hull on the NumPy
    twin's posterior (ORACLE_ABS), both with the noise of ONE evaluation; the expanded handle picks the same candidate."""
    import kg_reference as kr
    import test_kg_gpu as tk

    w, e, tw, X, y, Xs, hyp = pair
    E, R = 8, 200
    # candidates in a box of side 0.1 around the best of the 700 by the twin's mean: on candidates spread over the cube this model is
    # so sure of its maximiser that every knowledge gradient is exactly 0 and the comparison says nothing (asserted below)
    base = Xs[int(np.argmax(np.asarray(tw.predict(Xs)[0])))]
    cand = np.clip(base + 0.1 * (Xs[:R] - 0.5), 0.0, 1.0)
    xs = np.asfortranarray(cand.T)
    rw, re_ = w.kg(xs, E), e.kg(xs, E)
    mu, cov = w.predict_cov(xs)
    assert rw.mu.tobytes() == mu.tobytes()
    nu = math.exp(2.0 * hyp[2]) + EPS                                       # NOT nu / r: the next evaluation is one evaluation
    tkg, tseg = tk.twin_of(mu, np.stack([cov[i] / math.sqrt(cov[i, i] + nu) for i in range(E)]))
    assert tk.check_against_twin(rw.values, rw.nseg, tkg, tseg, "collapsed kg") <= tk.TWIN_REL
    mu_r, cov_r = tw.predict_cov(cand)
    hull = np.array([kr.kg_hull(mu_r, cov_r[i] / math.sqrt(cov_r[i, i] + nu))[0] for i in range(E)])
    scale = max(1.0, float(np.abs(mu_r).max()))
    print(f"  kg {tw.kern}: values {rw.values.min():.2e} .. {rw.values.max():.2e}; |collapsed - hull on the twin| / scale "
          f"{np.max(np.abs(rw.values - hull)) / scale:.2e}, |collapsed - expanded| / scale {np.max(np.abs(rw.values - re_.values)) / scale:.2e} "
          f"(ORACLE_ABS {tk.ORACLE_ABS:.2e})")
    assert np.all(hull > 1e-8) and np.all(tkg > 0.0)                         # non-vacuity: far above ORACLE_ABS
    assert np.max(np.abs(rw.values - hull)) / scale <= tk.ORACLE_ABS
    assert np.max(np.abs(rw.values - re_.values)) / scale <= 2 * tk.ORACLE_ABS      # (each handle within ORACLE_ABS of the exact model's hull)
    assert rw.best_idx == re_.best_idx == int(np.argmax(tkg))


def test_select_batch(pair):
    """q = 4: the picks of the expanded handle (the fantasy's noise is that of one evaluation on both)."""
    w, e, tw, X, y, Xs, hyp = pair
    xs = xs_of(Xs, 300)
    for acq, p, fv in (("UCB", [2.0], "believer"), ("EI", [float(y.max())], float(y.max()))):
        gw = w.select_batch(acq, p, xs, 4, fantasy=fv)
        ge = e.select_batch(acq, p, xs, 4, fantasy=fv)
        np.testing.assert_array_equal(gw[0], ge[0])
        assert len(set(gw[0].tolist())) == 4


def test_loo_leaves_one_site_out(pair):
    """bohip_gp_loo on cK_w: test_loo_gpu.check_values' bounds against the twin's formulas."""
    w, e, tw, X, y, Xs, hyp = pair
    res = w.loo()
    mu, var, logp, total = tw.loo()
    ybar = np.asarray(tw.ybar)
    for got, want, scale in ((res.mu, mu, max(np.abs(mu).max(), np.abs(ybar).max())), (res.var, var, np.abs(var).max()),
                             (res.logp, logp, np.abs(logp).max())):
        assert np.abs(got - want).max() <= 1e-9 * scale
    assert abs(res.total - total) <= 1e-9 * abs(total)
    np.testing.assert_array_equal(res.z, (w.y - res.mu) / np.sqrt(res.var))


def test_mes_gumbel(pair):
    import mes_reference as mr
    import test_mes_gpu as tm

    w, e, tw, X, y, Xs, hyp = pair
    s2f, xs = math.exp(2 * hyp[1]), xs_of(Xs, 300)
    rw, re_ = w.mes(xs, samples=16, mode="gumbel", seed=21), e.mes(xs, samples=16, mode="gumbel", seed=21)
    assert np.all(np.abs(rw.mu - re_.mu) <= 1e-6 * np.abs(re_.mu) + floor_of(e, s2f))
    assert np.all(np.abs(rw.var - re_.var) <= rr.var_tol(re_.var, len(y), s2f))
    assert tm.rel_err(rw.values, mr.values(rw.mu, rw.var, rw.maxvals)[0]) <= tm.REL
    assert (rw.best_val, rw.best_idx) == mr.record(rw.values) and np.all(rw.values >= 0.0)


def test_direct_max(pair):
    w, e, tw, X, y, Xs, hyp = pair
    lb, ub = np.full(rr.D, -0.2), np.full(rr.D, 1.1)
    for acq, p in (("UCB", [2.0]), ("EI", [float(np.median(y))])):
        f, x, ev, dc = w.direct_max(acq, p, lb, ub, 300)
        assert ev <= 300 and np.all(x >= lb) and np.all(x <= ub)
        sc_t = acq_value(acq, p, *tw.predict(x[None, :]))[0]
        assert abs(f - sc_t) <= 1e-6 * abs(sc_t) + 1e-9                      # test_lifecycle_gpu.test_direct_max's bound


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused_calls(bohip, m):
    """name -> a call of every refused single-handle entry point, through the thinnest Python layer that reaches the symbol."""
    from bohip import model as bm

    P = m.mll_batch_dims()[0]
    Theta = np.tile(np.concatenate([[m.logNoise, m.mean.beta], m.kernel.ll, [m.kernel.lsigma]]), (2, 1))
    assert Theta.shape[1] == P
    xs = np.asfortranarray(np.random.default_rng(1).random((rr.D, 20)))
    return {"bohip_gp_mll_grad_batch": lambda: bm._mll_grad_batch(m._lib, m._h, Theta, True),
            "bohip_gp_loo_grad": lambda: bm._loo_grad(m._lib, m._h, m.kernel.ll.size + 1),
            "bohip_gp_loo_grad_batch": lambda: bm._loo_grad_batch(m._lib, m._h, m.nobs, Theta, True, False),
            "bohip_gp_score_ens": lambda: bm.score_ensemble(m, "EI", [0.0], xs, Theta),
            "bohip_gp_score_ens_grad": lambda: bm.score_ensemble_grad(m, "EI", [0.0], xs, Theta),
            "bohip_gp_paths_draw": lambda: bm.PosteriorPaths(m._lib, m._h, m.dim, 1, 256, 0).close()}


def test_refusals_leave_the_model_untouched(bohip, pair):
    from bohip import _lib

    w, e, tw, X, y, Xs, hyp = pair
    before = (w.factor().tobytes(), w.alpha().tobytes(), counters(w), w.sites_info())
    for name, call in refused_calls(bohip, w).items():
        with pytest.raises(bohip.BohipError) as err:
            call()
        assert err.value.code == _lib.E_UNSUPPORTED and "replicated sites" in str(err.value) and name in str(err.value), (name, str(err.value))
        assert (w.factor().tobytes(), w.alpha().tobytes(), counters(w), w.sites_info()) == before, name
    small = new_handle(bohip, pair[2].kern, hyp, 64)
    try:
        small.append_(X[:60].T, y[:60])
        for name, call in refused_calls(bohip, small).items():              # ... and every one of them still serves an unweighted handle
            call()
    finally:
        small.close()


def test_a_device_list_with_a_weighted_replica_refuses(bohip):
    from bohip import _lib

    lnoise, lsig = rr.HYPERS[0]
    pos, _, evals, Xs = rr.raw(40, lnoise, lsig)
    mg = bohip.MultiGPE(rr.D, devices=(0,), mean=bohip.MeanConst(rr.BETA), kernel=bohip.SEArd(rr.LL["SEArd"], lsig), logNoise=lnoise, capacity=64)
    try:
        x, ybar, reps, ss, _ = rr.sites_of(pos, evals)
        mg.append_(x[:, :8], ybar[:8])
        xs = xs_of(Xs, 50)
        ok = mg.score("EI", [0.0], xs)
        lib = mg._lib
        lib.bohip_mgp_handle.restype = C.c_void_p
        h = C.c_void_p(lib.bohip_mgp_handle(mg._h, 0))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        sel = np.flatnonzero(reps > 1)[:4]
        xa, ya, ra, sa = np.asfortranarray(x[:, sel]), np.ascontiguousarray(ybar[sel]), np.ascontiguousarray(reps[sel]), np.ascontiguousarray(ss[sel])
        assert lib.bohip_gp_append_sites(h, xa.ctypes.data_as(dp), ya.ctypes.data_as(dp), ra.ctypes.data_as(ip), sa.ctypes.data_as(dp), 4) == 0
        for call in (lambda: mg.score("EI", [0.0], xs), lambda: mg.append_(x[:, 8:9], ybar[8:9]), mg.fit_):
            with pytest.raises(bohip.BohipError) as err:
                call()
            assert err.value.code == _lib.E_UNSUPPORTED and "replicated sites" in str(err.value) and "bohip_mgp_" in str(err.value)
        assert ok[2] >= 0
    finally:
        mg.close()


# ---- 5. the README's shape -------------------------------------------------------------------------------------------------------------
def test_bopt_with_five_repetitions(bohip):
    """BOpt(..., repetitions = 5) on a collapse=True model against collapse=False: the same posterior after the initial design, a fifth
    of the rows after ten iterations, and the raw maximum as the incumbent."""
    noise = np.random.default_rng(12)

    def f(x):
        return float(-np.sum((x - 0.3) ** 2) + 0.1 * noise.standard_normal())

    def run(collapse, iters):
        noise.bit_generator.state = np.random.default_rng(12).bit_generator.state
        m = bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd([0.0, 0.0], 0.0), logNoise=-2.0, capacity=64, collapse=collapse)
        o = bohip.BOpt(f, m, bohip.ExpectedImprovement(), bohip.NoModelOptimizer(), [-1.0, -1.0], [1.0, 1.0], repetitions=5,
                       maxiterations=iters, sense=bohip.Max, verbosity=bohip.Silent, initializer_iterations=8,
                       acquisitionoptions=dict(restarts=2, maxeval=200), rng=np.random.default_rng(3))
        bohip.boptimize_(o)
        return m, o

    gx = np.linspace(-1, 1, 8)
    grid = np.asfortranarray(np.stack(np.meshgrid(gx, gx), axis=0).reshape(2, 64))
    mc, oc = run(True, 8)                                                   # 8 = the initial design alone
    me, oe = run(False, 8)
    try:
        assert (mc.nobs, mc.nevals, me.nobs) == (8, 40, 40) and mc.weighted and np.all(mc.reps == 5)
        np.testing.assert_array_equal(np.repeat(mc.x, 5, axis=1), me.x)
        mu_c, var_c = mc.predict_f(grid)
        mu_e, var_e = me.predict_f(grid)
        assert np.all(np.abs(mu_c - mu_e) <= 1e-6 * np.abs(mu_e) + 64 * EPS * np.abs(me.alpha()).sum())
        assert np.all(np.abs(var_c - var_e) <= rr.var_tol(var_e, 40, 1.0))
        assert bohip.maxy(mc) == bohip.maxy(me) == me.y.max() and bohip.maxy(mc) > mc.y.max()
        assert oc.observed_optimum == oe.observed_optimum
    finally:
        mc.close()
        me.close()
    m, o = run(True, 18)                                                    # ... and ten iterations
    try:
        assert m.nevals == 90 and m.nobs == m.nevals // 5 == 18 and m.sites_info()[:2] == (18, 90)
        assert bohip.maxy(m) == m.ymax.max() == o.observed_optimum
        bohip.setparams_(o.acquisition, m)
        assert o.acquisition.tau == bohip.maxy(m) > m.y.max()                # EI's incumbent: the raw maximum
    finally:
        m.close()
