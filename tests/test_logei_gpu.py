"""LogEI on the device (csrc/acq_log.h): the functor against the 80-digit table through bohip_acq_eval, then every
route that inlines acq_eval / acq_partials -- scores (large, small-batch, one candidate, ragged tile), pruned arg-max == full pass,
the gradient by the chain rule, the ascent on a model where EI and its gradient are exactly zero, greedy batch selection, logical
shards, and the record of a batch whose scores are all -inf.  Device tolerance: 8 x the twin's measured worst error
(logei_reference.WORST; the host test holds the twin to 2 x)."""
import math
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logei_reference as lr   # noqa: E402
from conftest import load_golden, synth   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 8.0   # device tolerance = DEV x WORST


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def make_model(bohip, X, y, ll, lsig=0.0, lnoise=-2.0, beta=0.0, kern="SEArd", capacity=None):
    m = bohip.ElasticGPE(X.shape[1], mean=bohip.MeanConst(beta), kernel=getattr(bohip, kern)(ll, lsig), logNoise=lnoise,
                         capacity=capacity or len(y))
    m.append_(X.T, y)
    return m


def twin_scores(m, Xs, tau):
    mu, var = m.predict_f(Xs.T)
    return lr.logei(mu, var, tau)[0], mu, var


# ---- 1. the functor against the table -----------------------------------------------------------------------------------------------
def test_functor_matches_the_80_digit_table(bohip):
    """Measured on an MI355X (printed; DESIGN.md 6k records the figures)."""
    from bohip import _lib

    t = load_golden("logei_table")
    got = {k: np.empty(len(t["mu"])) for k in ("value", "dmu", "ds2")}
    for tau in np.unique(t["tau"]):
        m = t["tau"] == tau
        v, a, b = _lib.acq_eval("LogEI", [tau], t["mu"][m], t["s2"][m])
        got["value"][m], got["dmu"][m], got["ds2"][m] = v, a, b
        v_only, none_a, none_b = _lib.acq_eval("LogEI", [tau], t["mu"][m], t["s2"][m], partials=False)
        assert none_a is None and none_b is None and v_only.tobytes() == v.tobytes()
    for name in ("value", "dmu", "ds2"):
        worst = lr.assert_close(name, got[name], t[name], DEV, "device")
        print(f"device vs table, {name}: worst {worst:.3e} (twin WORST {lr.WORST[name]:.1e}, bound {DEV:g} x)")
    twin = lr.logei(t["mu"], t["s2"], t["tau"])
    for name, tw in zip(("value", "dmu", "ds2"), twin):      # same branches, same order: device and twin differ by libm vs OCML only
        lr.assert_close(name, got[name], np.where(np.isfinite(t[name]), tw, t[name]), DEV, "device vs twin")


def test_functor_entry_point_serves_the_reference_functors(bohip):
    """ids 0-4 on the table's inputs against the oracle's verbatim functors, to the score tolerance of tests/test_parity_gpu.py
    (1e-6 relative plus a floor of 64 eps of the operands' scale)."""
    from bohip import _lib
    from oracle.oracle import np_acq

    t = load_golden("logei_table")
    keep = t["tau"] == 0.0
    mu, s2 = t["mu"][keep], t["s2"][keep]
    eps = np.finfo(np.float64).eps
    floor = 64 * eps * np.maximum(np.maximum(np.abs(mu), np.sqrt(s2)), 1.0) + 1e-12
    for acq, p in [("EI", [0.0]), ("PI", [0.0]), ("UCB", [2.5]), ("MI", [1.5, 0.3]), ("MaxMean", [])]:
        ref = np.array([np_acq(acq, p, float(a), float(b)) for a, b in zip(mu, s2)])
        got, dmu, ds2 = _lib.acq_eval(acq, p, mu, s2)
        assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref) + floor), (acq, np.nanmax(np.abs(got - ref)))
        assert not np.isnan(dmu).any() and not np.isnan(ds2).any()
    assert np.array_equal(_lib.acq_eval("MaxMean", [], mu, s2)[1], np.ones(len(mu)))


# ---- 2. scores ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,R", [(200, 3, 300), (200, 3, 32), (200, 3, 1), (130, 1, 65)])
def test_scores_on_every_route(bohip, N, d, R):
    from scipy.special import erfc

    X, y, Xs = synth(N, d, R, seed=N + R)
    ll = np.linspace(-0.8, -0.3, d)
    m = make_model(bohip, X, y, ll, 0.1, -2.0, 0.05)
    for shift in (0.0, 5.0, 1e3):
        tau = float(y.max()) + shift
        sc, bv, bi = m.score("LogEI", [tau], Xs.T)
        ref, mu, var = twin_scores(m, Xs, tau)
        lr.assert_close("value", sc, ref, DEV, f"score tau+{shift}")
        assert np.all(np.isfinite(sc[var > 0]))
        assert bi == int(np.argmax(sc)) and np.float64(bv).tobytes() == sc[bi].tobytes()      # the first maximum of the scores
        sg, g = m.score_grad("LogEI", [tau], Xs.T)
        np.testing.assert_array_equal(sg, sc)                    # value route and gradient route: bit for bit
        assert g.shape == (d, R) and np.all(np.isfinite(g))
        _, bv2, bi2 = m.score("LogEI", [tau], Xs.T, want_scores=False)
        assert (bi2, np.float64(bv2).tobytes()) == (bi, np.float64(bv).tobytes())
        # the ordering is the textbook EI's wherever that does not underflow
        s = np.sqrt(var)
        z = (mu - tau) / s
        ei = (mu - tau) * (0.5 * erfc(-z / math.sqrt(2))) + s * np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
        e = np.exp(sc)
        top = np.sort(e)[::-1]
        if top[0] > 1e-290 and (R == 1 or top[0] > top[1]):
            assert int(np.argmax(e)) == bi
            order = np.argsort(-ei, kind="stable")
            if R == 1 or ei[order[0]] - ei[order[1]] > 1e-9 * ei[order[0]]:
                assert int(order[0]) == bi
        if shift == 1e3:
            assert np.all(e == 0.0) and np.all(sc < -1e4)        # deep tail: EI is dead, LogEI still ranks
    m.close()


# ---- 3. pruned arg-max == full pass --------------------------------------------------------------------------------------------------
def assert_same_record(m, acq, params, Xs):
    sc, v_full, i_full = m.score(acq, params, Xs.T, want_scores=True)
    _, v, i = m.score(acq, params, Xs.T, want_scores=False)
    assert i == i_full, (acq, i, i_full)
    assert np.float64(v).tobytes() == np.float64(v_full).tobytes(), (acq, v, v_full)
    s = np.where(np.isnan(sc), -np.inf, sc)
    assert i == (int(np.argmax(s)) if s.max() > -np.inf else -1)           # first maximum (the reference's strict '>'); -1: nobody won
    return sc


def prune_bounds(m, acq, params, Xs):
    import ctypes as C
    from bohip import _lib

    f = _lib.load().bohip_debug_prune_bounds
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    p = np.zeros(2)
    p[:len(params)] = params
    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    ub = np.empty(len(xs))
    rc = f(m._h, _lib.ACQ[acq], p.ctypes.data, xs.ctypes.data, len(xs), ub.ctypes.data)
    return rc, ub


@pytest.mark.parametrize("N", [100, 300])
def test_pruned_record_equals_full_pass(bohip, N):
    """A model without noise (exp(-60) + eps on the diagonal, length 0.2 so that it still factors): on an observation the true
    variance is ~2e-16 and the computed s_f^2 - v'v clamps to exactly 0 for about a third of them (CPU oracle: 27 of 100, 101 of
    300), so with every observation among the candidates the call sees scores of -inf (mu <= tau) and of log(mu - tau) (mu > tau,
    at tau = median y) beside the ordinary ones.  N = 300 is three row tiles: the value-only call prunes and the bounds exist
    (rc == 0 is asserted).  N = 100 is one row tile: the full pass, and bohip_debug_prune_bounds says E_UNSUPPORTED."""
    from bohip import _lib

    d, R = 4, 3000
    rng = np.random.default_rng(N)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    m = make_model(bohip, X, y, np.full(d, math.log(0.2)), 0.0, -30.0, 0.0)
    Xs = np.random.default_rng(N + 1).random((R, d))
    Xs[200:200 + N] = X                                          # every observation is a candidate
    Xs[600:3000:41] = Xs[599]                                    # many copies of one candidate
    on = np.arange(200, 200 + N)
    clamped = None
    for tau in (float(y.max()) + 2.0, float(y.max()), float(np.median(y))):
        sc = assert_same_record(m, "LogEI", [tau], Xs)
        assert not np.isnan(sc).any()
        dead = sc[on] == -np.inf
        if clamped is None:                                      # tau above every mean: -inf marks exactly the clamped variances
            clamped = dead
            assert clamped.sum() >= 8, f"only {clamped.sum()} of {N} observations clamp to sigma^2 = 0"
        elif tau < y.max():                                      # tau below some of their means: those score log(mu - tau)
            alive = clamped & ~dead
            assert alive.sum() >= 4 and dead.sum() >= 4
            np.testing.assert_allclose(sc[on][alive], np.log(y[alive] - tau), rtol=1e-6, atol=1e-9)
        rc, ub = prune_bounds(m, "LogEI", [tau], Xs)
        if N == 300:
            assert rc == 0, rc
            assert not np.isnan(ub).any() and not (ub < sc).any(), np.flatnonzero(ub < sc)[:5]      # -inf >= -inf allowed
            print(f"N = {N}, tau = {tau:.4g}: {int(dead.sum())} scores of -inf among the observations, {int((ub == -np.inf).sum())} bounds of -inf")
        else:
            assert rc == _lib.E_UNSUPPORTED, rc
        _, _, i = m.score("LogEI", [tau], Xs.T, want_scores=False)
        Xs2 = Xs.copy()
        Xs2[i + 1:] = Xs[i]                                      # the winner duplicated behind its first position
        assert_same_record(m, "LogEI", [tau], Xs2)
    # nothing but clamped candidates below tau (and copies of them, to stay a pruning call's size): nobody wins, on either pass
    tau = float(y.max()) + 2.0
    only = np.tile(X[clamped], (R // int(clamped.sum()) + 1, 1))[:R]
    sc = assert_same_record(m, "LogEI", [tau], only)
    assert np.all(sc == -np.inf)                                 # (the copies sit in other tiles: the same sums, the same clamp)
    assert m.score("LogEI", [tau], only.T, want_scores=False)[1:] == (-np.inf, -1)
    m.close()


# ---- 4. gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d,R", [("SEArd", 300, 5, 40), ("Mat52Ard", 300, 5, 40), ("SEArd", 40, 1, 7), ("Mat52Ard", 40, 1, 7),
                                        ("SEArd", 150, 40, 7)])   # (d = 40: k_small_u_logei64, LogEI's own instantiation)
def test_gradient_is_the_chain_rule(bohip, orc, kern, N, d, R):
    """twin partials x the oracle's grad mu and grad sigma^2 (the latter from its UCB gradient: grad UCB = grad mu +
    beta grad sigma^2 / (2 sigma))."""
    X, y, Xs = synth(N, d, R, seed=31 + d)
    ll = np.linspace(-0.8, -0.2, d)
    L, alpha = orc.fit(X, y, ll, 0.1, -2.0, 0.05, kern=kern)
    m = make_model(bohip, X, y, ll, 0.1, -2.0, 0.05, kern=kern)
    mu, var = orc.predict(X, ll, 0.1, 0.05, L, alpha, Xs, kern=kern)
    _, gmu = orc.score_grad(X, ll, 0.1, 0.05, L, alpha, "MaxMean", [], Xs, kern=kern)
    beta_u = 2.0
    _, gucb = orc.score_grad(X, ll, 0.1, 0.05, L, alpha, "UCB", [beta_u], Xs, kern=kern)
    gs2 = (gucb - gmu) * (2.0 * np.sqrt(var) / beta_u)[:, None]
    for shift in (0.0, 5.0):
        tau = float(y.max()) + shift
        _, a, b = lr.logei(mu, var, tau)
        g_ref = a[:, None] * gmu + b[:, None] * gs2
        sc, g = m.score_grad("LogEI", [tau], Xs.T)
        scale = np.abs(g_ref).max()
        np.testing.assert_allclose(g.T, g_ref, rtol=1e-6, atol=1e-9 * scale + 1e-12)
        np.testing.assert_array_equal(sc, m.score("LogEI", [tau], Xs.T)[0])
    m.close()


# ---- 5. the ascent where EI is dead ----------------------------------------------------------------------------------------------------
def dead_ei_problem(N):
    """d = 2, SEArd with length 0.3, signal 0.1, noise exp(-3): a smooth bump of height 5 at (0.8, 0.8) seen on an 8 x 5 grid (plus
    uniform filler for N > 40), tau = max y.  The model cannot believe in anything near tau except at the bump: z ~ -120 ... -450
    over [0, 0.45]^2, three to six length-scales away.  (Checked on the CPU with the oracle's predict + the twin: the host
    restatement of the ascent, and SciPy's L-BFGS-B, climb to (0.80, 0.80) from most of these starts; textbook EI there 3e-3 at
    N = 40 and 1e-2 at N = 300.)"""
    gx, gy = np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 5))
    X = np.stack([gx.ravel(), gy.ravel()], axis=1)
    if N > 40:
        X = np.vstack([X, np.random.default_rng(6).random((N - 40, 2))])
    y = 5.0 * np.exp(-((X - 0.8) ** 2).sum(1) / (2 * 0.4 ** 2))
    starts = np.asfortranarray((np.random.default_rng(7).random((10, 2)) * 0.45).T)
    return X, y, starts


@pytest.mark.parametrize("N", [40, 300])       # the one-workgroup-per-start ascent; the two-kernel pass
def test_ascent_climbs_where_ei_is_dead(bohip, N):
    X, y, starts = dead_ei_problem(N)
    m = make_model(bohip, X, y, np.full(2, math.log(0.3)), math.log(0.1), -3.0, 0.0)
    tau = float(y.max())
    lb, ub = np.zeros(2), np.ones(2)
    # preconditions
    f_ei, g_ei = m.score_grad("EI", [tau], starts)
    assert np.all(f_ei == 0.0) and np.all(g_ei == 0.0)
    f_le, g_le = m.score_grad("LogEI", [tau], starts)
    assert np.all(np.isfinite(f_le)) and np.all(np.isfinite(g_le)) and np.all(np.abs(g_le).max(axis=0) > 0)
    # EI: every start is "converged at once" where it stands
    f, Xo, bf, bi, bx, _ = m.ascend("EI", [tau], lb, ub, starts)
    assert bf == 0.0 and np.all(f == 0.0) and np.array_equal(Xo, starts)
    # LogEI: climbs, and ends where the reference's EI is alive again
    f, Xo, bf, bi, bx, ev = m.ascend("LogEI", [tau], lb, ub, starts)
    print(f"N = {N}: best start {f_le.max():.6g} -> {bf:.6g} at {bx} in {ev} passes; per start {np.round(f, 3)}")
    assert bi >= 0 and bf > f_le.max()
    at_x = m.score("LogEI", [tau], bx)[0][0]                    # (the one-workgroup form sums in its own order: to rounding, not bit for bit)
    assert abs(bf - at_x) <= 1e-9 * max(1.0, abs(at_x))
    assert m.score("EI", [tau], bx)[0][0] > 0
    # the same through the host entry point (its own Latin-hypercube starts): EI over the dead corner returns 0.0 ...
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # (0.0 is a finite value: no "no finite value" warning)
        f_host, x_host = bohip.acquire_max(bohip.ExpectedImprovement(), m, lb, np.full(2, 0.45),
                                           {"method": "LD_LBFGS", "restarts": 10, "maxeval": 2000}, np.random.default_rng(3))
    assert f_host == 0.0 and np.all(x_host <= 0.45)
    # ... LogEI over the box finds where EI is alive, by the ascent and by dividing rectangles (bohip_gp_direct_max)
    a = bohip.LogExpectedImprovement()
    f_dir, x_dir = bohip.acquire_max(a, m, lb, ub, {"method": "GN_DIRECT_L", "restarts": 1, "maxeval": 500}, np.random.default_rng(3))
    print(f"N = {N}: GN_DIRECT_L {f_dir:.6g} at {x_dir}")
    at_dir = m.score("LogEI", [tau], x_dir)[0][0]
    assert np.isfinite(f_dir) and f_dir > f_le.max() and abs(f_dir - at_dir) <= 1e-9 * max(1.0, abs(at_dir))
    assert m.score("EI", [tau], x_dir)[0][0] > 0
    a = bohip.LogExpectedImprovement()
    maxf, maxx = bohip.acquire_max(a, m, lb, ub, {"method": "LD_LBFGS", "restarts": 10, "maxeval": 2000}, np.random.default_rng(3))
    assert a.tau == tau and np.isfinite(maxf) and m.score("EI", [tau], maxx)[0][0] > 0
    m.close()


def test_ascent_in_the_widest_one_workgroup_bucket(bohip):
    """d = 12 runs k_ascent_wg_logei16, the instantiation LogEI has to itself (the d <= 16 bucket of the other functors compiles the
    LogEI call out): values are the scoring kernels' to rounding, no start ends below where it began, the best is the first maximum."""
    N, d, R = 100, 12, 10
    X, y, Xs = synth(N, d, R, seed=12)
    m = make_model(bohip, X, y, np.full(d, math.log(0.7)), 0.0, -2.0, 0.0)
    starts = np.asfortranarray(Xs.T)
    for shift in (0.0, 30.0):
        tau = float(y.max()) + shift
        f0 = m.score("LogEI", [tau], starts)[0]
        f, Xo, bf, bi, bx, ev = m.ascend("LogEI", [tau], np.zeros(d), np.ones(d), starts, maxeval=200)
        at = m.score("LogEI", [tau], Xo)[0]
        print(f"d = 12, tau + {shift}: {ev} passes, start {np.round(f0, 3)} -> {np.round(f, 3)}")
        assert np.all(np.isfinite(f)) and np.all(np.abs(f - at) <= 1e-9 * np.maximum(1.0, np.abs(at)))
        assert np.all(f >= f0 - 1e-9 * np.maximum(1.0, np.abs(f0))) and np.any(f > f0)
        assert bi == int(np.argmax(f)) and bf == f[bi] and np.array_equal(bx, Xo[:, bi])
        assert np.all(Xo >= 0.0) and np.all(Xo <= 1.0)
    m.close()


# ---- 6. batch ---------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_greedy_conditioning_scored_by_the_twin(bohip):
    N, d, R, q = 200, 3, 300, 3
    X, y, Xs = synth(N, d, R, seed=9)
    ll = np.linspace(-0.8, -0.3, d)
    m = make_model(bohip, X, y, ll, 0.1, -2.0, 0.05)
    tau0 = float(y.max()) - 0.5
    for raise_tau in (True, False):
        idx, val, mu_p, var_p = m.select_batch("LogEI", [tau0], Xs.T, q, fantasy="believer", raise_tau=raise_tau)
        m2 = make_model(bohip, X, y, ll, 0.1, -2.0, 0.05, capacity=N + q)
        picked = np.zeros(R, bool)
        tau = tau0
        for t in range(q):
            sc, mu, var = twin_scores(m2, Xs, tau)
            s = np.where(picked | np.isnan(sc), -np.inf, sc)
            i = int(np.argmax(s))
            second = np.sort(s)[-2]
            print(f"raise_tau={raise_tau} round {t}: twin idx {i} val {s[i]:.12g} gap {s[i] - second:.3g} | batch idx {idx[t]} val {val[t]:.12g}")
            assert s[i] - second > 1e-6 * max(abs(s[i]), 1.0), "test inputs: the top two are too close to call"
            assert idx[t] == i
            assert abs(val[t] - s[i]) <= 1e-6 * abs(s[i]) + 1e-9
            picked[i] = True
            yf = float(mu[i])
            if raise_tau:
                tau = max(tau, yf)
            m2.append_(Xs[i], [yf])
        assert m.nobs == N
        m2.close()
    m.close()


# ---- 7. shards ------------------------------------------------------------------------------------------------------------------------
def test_logical_shards_give_the_single_handle_record(bohip):
    N, d, R = 200, 3, 1024
    X, y, Xs = synth(N, d, R, seed=77)
    ll = np.linspace(-0.8, -0.3, d)
    one = make_model(bohip, X, y, ll, 0.1, -2.0, 0.05)
    mg = bohip.MultiGPE(d, devices=(0,), shards_per_device=4, mean=bohip.MeanConst(0.05), kernel=bohip.SEArd(ll, 0.1), logNoise=-2.0,
                        capacity=N)
    mg.append_(X.T, y)
    for shift in (0.0, 5.0):
        tau = float(y.max()) + shift
        sc1, bv1, bi1 = one.score("LogEI", [tau], Xs.T)
        scg, bvg, big = mg.score("LogEI", [tau], Xs.T)
        np.testing.assert_array_equal(scg, sc1)
        assert (np.float64(bvg).tobytes(), big) == (np.float64(bv1).tobytes(), bi1)
    a1, ag = bohip.LogExpectedImprovement(), bohip.LogExpectedImprovement()
    opts = {"method": "LD_LBFGS", "restarts": 10, "maxeval": 200}
    f1, x1 = bohip.acquire_max(a1, one, np.zeros(d), np.ones(d), opts, np.random.default_rng(5))
    fg, xg = bohip.acquire_max(ag, mg, np.zeros(d), np.ones(d), opts, np.random.default_rng(5))
    assert np.isfinite(f1) and f1 == fg and np.array_equal(x1, xg)
    mg.close(); one.close()


# ---- 8. every score -inf ----------------------------------------------------------------------------------------------------------------
def test_every_score_minus_inf_gives_the_nobody_won_record(bohip):
    """Candidates ON observations of a model without noise (exp(-60) + eps on the diagonal) have a true variance of ~2e-16, and the
    computed s_f^2 - v'v lands on either side of 0: where it is <= 0 the variance clamps to exactly 0 (28 of these 120 observations
    with the CPU oracle's summation order), and with tau above every mean such a candidate scores -inf.  The candidates are the
    observations whose variance the device's own predict_f reports as 0."""
    rng = np.random.default_rng(2)
    N, d = 120, 2
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1)
    m = make_model(bohip, X, y, np.full(d, math.log(0.1)), 0.0, -30.0, 0.0)
    mu, var = m.predict_f(X.T)
    on = np.flatnonzero(var == 0.0)
    assert on.size >= 8, f"only {on.size} of {N} observations clamp to sigma^2 = 0"
    tau = float(mu.max()) + 1.0
    for R in (on.size, 1):                                       # small-batch route; one candidate
        Xs = X[on[:R]]
        sc, bv, bi = m.score("LogEI", [tau], Xs.T)
        assert np.all(sc == -np.inf) and bv == -np.inf and bi == -1
        _, bv, bi = m.score("LogEI", [tau], Xs.T, want_scores=False)
        assert bv == -np.inf and bi == -1
    # the large route (R > 256) sums in its own order: its clamped candidates are found on that route
    pool = np.tile(X, (12, 1))
    dead = m.score("LogEI", [tau], pool.T)[0] == -np.inf
    assert dead.sum() > 256, f"only {dead.sum()} of {len(pool)} candidates clamp on the large route"
    big = pool[dead]
    sc, bv, bi = m.score("LogEI", [tau], big.T)
    assert np.all(sc == -np.inf) and (bv, bi) == (-np.inf, -1)
    _, bv, bi = m.score("LogEI", [tau], big.T, want_scores=False)
    assert (bv, bi) == (-np.inf, -1)
    sc, g = m.score_grad("LogEI", [tau], X[on].T)
    assert np.all(sc == -np.inf) and np.all(g == 0.0)
    # one candidate that can win beside them wins
    mixed = np.vstack([X[on[:5]], [[0.5, 0.5]], X[on[5:8]]])
    sc, bv, bi = m.score("LogEI", [tau], mixed.T)
    assert np.isfinite(sc[5]) and np.all(sc[np.arange(9) != 5] == -np.inf)
    assert bi == 5 and bv == sc[5]
    # the Python call: a warning, (-inf, the lower bounds)
    lo = X[on[0]]
    with pytest.warns(UserWarning, match="no finite value"):
        f, x = bohip.acquire_max(bohip.LogExpectedImprovement(tau), m, lo, lo, {"method": "LD_LBFGS", "restarts": 3},
                                 np.random.default_rng(0))
    assert f == -math.inf and np.array_equal(x, lo)
    m.close()
