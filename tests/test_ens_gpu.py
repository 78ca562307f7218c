"""bohip_gp_score_ens (kernels_ens.hip: factor per setting, V = W K* on the matrix pipe per candidate tile and setting, weighted sum)
and the marginalised acquisition through the BO loop.

Shapes: N below, at and across the 16-wide blocks (1, 2, 17, 64, 65, 200) and at the cap (512), one d from every dimension bucket;
R = 1, 17 and 700 (700 crosses candidate tiles and is a multiple of none; 300 at N = 512).  Reference: the NumPy twin
(tests/ens_reference.py).  Tolerances are those of tests/test_matern_gpu.py::test_score_and_argmax against the same twin, per
setting: mu rtol 1e-6 + mu_floor, sigma^2 var_tol, scores 1e-6 |ref| + floor + 1e-12; the average is a convex combination of the
per-setting scores, so its bound is the same combination of theirs."""
import ctypes as C
import functools

import numpy as np
import pytest

import ens_reference as er
from conftest import synth, var_tol
from matern_reference import KERNELS, first_argmax
from test_fit_gpu import centre, model_of, settings
from test_parity_gpu import bohip, mu_floor  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

ALL = list(KERNELS)
SHAPES = {(1, 1): ["SEArd", "Mat12Iso"], (2, 2): ["SEIso", "Mat32Ard"], (17, 3): ["Mat52Ard", "Mat12Ard", "Mat32Iso"], (65, 8): ALL,
          (200, 17): ["Mat52Iso", "Mat12Ard", "SEIso"], (64, 33): ["Mat32Ard", "Mat52Ard", "Mat12Iso"], (512, 8): ["SEArd", "Mat32Iso"]}
CASES = [(k, N, d, R) for (N, d), ks in SHAPES.items() for k in ks for R in (1, 17, 300 if N == 512 else 700)]
ACQS = [("EI", None), ("PI", None), ("UCB", [2.5]), ("MI", [1.0, 0.3]), ("MaxMean", []), ("LogEI", None)]


def params(p, y):
    return [float(np.median(y))] if p is None else p


# Seeds.  Trial t of a case draws the data with seed 1000 + 7 N + 3 d + R + 10007 t and the settings with seed N + d + t.  Trial 0
# unless the twin ALONE (no device) shows a near tie at the top for some acquisition there -- a winner that leads its runner-up by
# less than four times the sum of their tolerances (700 candidates on a line at d = 1; EI and PI below the floor under the short
# length-scales at d = 33) -- then the first trial without one.  The parity test asserts the lead again, so no tie is exempted.
TRIAL = {("SEArd", 1, 1, 700): 11, ("Mat12Iso", 1, 1, 700): 8, ("SEArd", 65, 8, 700): 1, ("SEIso", 200, 17, 700): 2,
         ("Mat32Ard", 64, 33, 17): 4, ("Mat32Ard", 64, 33, 700): 16, ("Mat52Ard", 64, 33, 17): 16, ("Mat52Ard", 64, 33, 700): 16}


@functools.lru_cache(maxsize=None)
def twin_moments(kern, N, d, R, H=3):
    """(X, y, Xs, Theta, [row models], mu[H, R], var[H, R]) of one case: computed once, never written to."""
    t = TRIAL.get((kern, N, d, R), 0)
    X, y, Xs = synth(N, d, R, seed=1000 + 7 * N + 3 * d + R + 10007 * t)
    Theta = settings(kern, d, H, seed=N + d + t)
    refs = [er.row_model(kern, X, y, t) for t in Theta]
    mv = [r.predict(Xs) for r in refs]
    out = (X, y, Xs, Theta, refs, np.array([m for m, _ in mv]), np.array([v for _, v in mv]))
    for a in (X, y, Xs, Theta, out[5], out[6]):
        a.setflags(write=False)
    return out


def close(got, ref, tol, what):
    """|got - ref| <= tol where the reference is finite; the same value (a -Inf of LogEI) where it is not."""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), (what, "non-finite entries differ")
    err = np.abs(got[fin] - ref[fin])
    tol = np.broadcast_to(tol, ref.shape)[fin]
    if err.size:
        print(f"{what}: worst error / bound {np.max(err / tol):.3g}")
    assert np.all(err <= tol), (what, float(np.max(err / tol)))


def score_tols(refs, each_r):
    return np.array([1e-6 * np.abs(e) + mu_floor(r.alpha, r.s2f) + 1e-12 for r, e in zip(refs, each_r)])


def check_rows(res, refs, mu_r, var_r, each_r, N, what, rows=None):
    rows = range(len(refs)) if rows is None else rows
    tol = score_tols(refs, each_r)
    for h in rows:
        r = refs[h]
        close(res.mu[h], mu_r[h], 1e-6 * np.abs(mu_r[h]) + mu_floor(r.alpha, r.s2f), f"{what} mu[{h}]")
        close(res.var[h], var_r[h], var_tol(var_r[h], N, r.s2f), f"{what} var[{h}]")
        close(res.each[h], each_r[h], tol[h], f"{what} each[{h}]")
    return tol


# ---- 1. parity over shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d,R", CASES)
def test_ensemble_matches_the_twin(bohip, kern, N, d, R):
    X, y, Xs, Theta, refs, mu_r, var_r = twin_moments(kern, N, d, R)
    m = model_of(bohip, kern, X, y)
    piv0 = np.zeros(3, dtype=np.int64)
    for acq, p in ACQS:
        p = params(p, y)
        res = m.score_ensemble(acq, p, Xs.T, Theta, want_each=True, want_moments=True)
        assert res.route == "device" and np.all(res.pivot == 0)
        each_r = np.array([er.from_moments(acq, p, mu_r[h], var_r[h]) for h in range(3)])
        what = f"{kern} N={N} d={d} R={R} {acq}"
        tol = check_rows(res, refs, mu_r, var_r, each_r, N, what)
        sc_r = er.average(each_r, None, piv0)
        tol_avg = tol.sum(axis=0) / 3.0
        close(res.scores, sc_r, tol_avg, f"{what} scores")
        assert (res.best_val, res.best_idx) == first_argmax(res.scores)
        bv, bi = first_argmax(sc_r)
        if R > 1:   # the twin's winner leads its runner-up by more than the two can move: the seeds were chosen so (twin alone)
            rest = np.delete(np.arange(R), bi)
            ru = rest[np.argmax(sc_r[rest])]
            assert sc_r[bi] - sc_r[ru] > tol_avg[bi] + tol_avg[ru], (what, "near tie in the twin", sc_r[bi] - sc_r[ru])
        assert res.best_idx == bi, what
    m.close()


# ---- 2. H = 1 reproduces a model built with that setting ----------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d", [("Mat52Ard", 200, 17), ("SEIso", 65, 8), ("Mat12Ard", 17, 3), ("Mat32Iso", 64, 33)])
def test_one_setting_is_a_model_with_those_parameters(bohip, kern, N, d):
    X, y, Xs, Theta, refs, mu_r, var_r = twin_moments(kern, N, d, 700)
    m, second = model_of(bohip, kern, X, y), model_of(bohip, kern, X, y, theta=Theta[0])
    mu2, var2 = second.predict_f(Xs.T)
    for acq, p in ACQS:
        p = params(p, y)
        res = m.score_ensemble(acq, p, Xs.T, Theta[:1], weights=[1.0], want_each=True, want_moments=True)
        sc2 = second.score(acq, p, Xs.T)[0]
        r = refs[0]
        floor = mu_floor(r.alpha, r.s2f)
        close(res.mu[0], mu2, 1e-6 * np.abs(mu2) + floor, f"{kern} {acq} mu vs model")
        close(res.var[0], var2, var_tol(var2, N, r.s2f), f"{kern} {acq} var vs model")
        close(res.each[0], sc2, 1e-6 * np.abs(sc2) + floor + 1e-12, f"{kern} {acq} each vs model")
        np.testing.assert_array_equal(res.scores, res.each[0])          # one setting of weight 1: 0.0 + 1.0 a
    m.close()
    second.close()


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------
def launches(m, label):
    return sum(1 for name, _ in m.timing() if name == label)


@pytest.mark.parametrize("kern,N,d", [("Mat52Ard", 200, 17), ("SEArd", 65, 8), ("Mat12Iso", 17, 3)])
def test_a_value_depends_on_its_setting_and_its_candidate_only(bohip, kern, N, d, monkeypatch):
    X, y, Xs, _, _, _, _ = twin_moments(kern, N, d, 700)
    Theta = settings(kern, d, 5, seed=77)
    p = [float(np.median(y))]
    m = model_of(bohip, kern, X, y)
    m.enable_timing(True)
    full = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)
    assert launches(m, "ens_factor") == 1 and launches(m, "ens_score") == 1 and launches(m, "ens_reduce") >= 1
    for h in (0, 3):                                                # the same setting alone ...
        one = m.score_ensemble("EI", p, Xs.T, Theta[h:h + 1], want_each=True, want_moments=True)
        for a, b in ((one.each, full.each), (one.mu, full.mu), (one.var, full.var)):
            np.testing.assert_array_equal(a[0], b[h])
    perm = np.array([3, 4, 0, 2, 1])                                # ... and at another position, next to a failed row
    moved = Theta[perm].copy()
    moved[3, 0] = np.nan
    other = m.score_ensemble("EI", p, Xs.T, moved, want_each=True, want_moments=True)
    assert other.pivot.tolist() == [0, 0, 0, 1, 0]
    for k in (0, 1, 2, 4):
        for a, b in ((other.each, full.each), (other.mu, full.mu), (other.var, full.var)):
            np.testing.assert_array_equal(a[k], b[perm[k]])
    for j in (0, 17, 335, 699):                                     # one candidate alone
        one = m.score_ensemble("EI", p, Xs[j:j + 1].T, Theta, want_each=True, want_moments=True)
        for a, b in ((one.each, full.each), (one.mu, full.mu), (one.var, full.var)):
            np.testing.assert_array_equal(a[:, 0], b[:, j])
        assert one.scores[0] == full.scores[j]
    M = -(-N // 16) * 16
    slab_mb = (2 * M + 1) * (M + 8) * 8 / 2 ** 20
    monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")                  # read at every call
    assert 2 * slab_mb > 1.0 or N < 100                             # (at N = 200 one setting fits, two do not: 5 launches)
    capped = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)
    if N >= 100:
        assert launches(m, "ens_factor") == 5 and launches(m, "ens_score") == 5
    for name in ("scores", "each", "mu", "var", "pivot"):
        np.testing.assert_array_equal(getattr(capped, name), getattr(full, name))
    assert (capped.best_val, capped.best_idx) == (full.best_val, full.best_idx)
    m.close()


def test_candidates_beyond_one_chunk(bohip, monkeypatch):
    """R = 16384 + 77 is two candidate chunks inside the call; with the workspace capped as well, every chunk factors and scores the
    settings one launch at a time.  Against the twin, and the same bytes as the calls on the two parts and as the uncapped call."""
    kern, N, d, R = "Mat52Iso", 200, 17, 16384 + 77
    X, y, Xs, Theta, refs, mu_r, var_r = twin_moments(kern, N, d, R)
    p = [float(np.median(y))]
    m = model_of(bohip, kern, X, y)
    m.enable_timing(True)
    full = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)
    assert launches(m, "ens_factor") == 1 and launches(m, "ens_score") == 2
    each_r = np.array([er.from_moments("EI", p, mu_r[h], var_r[h]) for h in range(3)])
    tol = check_rows(full, refs, mu_r, var_r, each_r, N, "two chunks")
    close(full.scores, er.average(each_r, None, np.zeros(3, dtype=np.int64)), tol.sum(axis=0) / 3.0, "two chunks scores")
    assert (full.best_val, full.best_idx) == first_argmax(full.scores)
    for lo, hi in ((0, 16384), (16384, R)):
        part = m.score_ensemble("EI", p, Xs[lo:hi].T, Theta, want_each=True, want_moments=True)
        for name in ("each", "mu", "var"):
            np.testing.assert_array_equal(getattr(part, name), getattr(full, name)[:, lo:hi])
        np.testing.assert_array_equal(part.scores, full.scores[lo:hi])
    monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")
    capped = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)
    assert launches(m, "ens_factor") == 6 and launches(m, "ens_score") == 6      # three settings, one at a time, per chunk
    for name in ("scores", "each", "mu", "var", "pivot"):
        np.testing.assert_array_equal(getattr(capped, name), getattr(full, name))
    assert (capped.best_val, capped.best_idx) == (full.best_val, full.best_idx)
    m.close()


# ---- 4. weights ---------------------------------------------------------------------------------------------------------------------
def test_weights(bohip):
    kern, N, d, R = "Mat52Ard", 65, 8, 700
    X, y, Xs, Theta, refs, mu_r, var_r = twin_moments(kern, N, d, R)
    m = model_of(bohip, kern, X, y)
    piv0 = np.zeros(3, dtype=np.int64)
    for acq, p in (("EI", None), ("LogEI", None), ("UCB", [2.5])):
        p = params(p, y)
        each_r = np.array([er.from_moments(acq, p, mu_r[h], var_r[h]) for h in range(3)])
        tol = score_tols(refs, each_r)
        w = np.array([0.2, 3.0, 0.7])
        res = m.score_ensemble(acq, p, Xs.T, Theta, weights=w)
        close(res.scores, er.average(each_r, w, piv0), (w[:, None] * tol).sum(axis=0) / w.sum(), f"{acq} unequal weights")
        assert (res.best_val, res.best_idx) == first_argmax(res.scores)
        none = m.score_ensemble(acq, p, Xs.T, Theta)
        ones = m.score_ensemble(acq, p, Xs.T, Theta, weights=np.ones(3))
        np.testing.assert_array_equal(none.scores, ones.scores)
        assert (none.best_val, none.best_idx) == (ones.best_val, ones.best_idx)
        zero = m.score_ensemble(acq, p, Xs.T, Theta, weights=[0.5, 0.0, 1.5])       # a weight of 0 removes the row exactly
        two = m.score_ensemble(acq, p, Xs.T, Theta[[0, 2]], weights=[0.5, 1.5])
        np.testing.assert_array_equal(zero.scores, two.scores)
        assert (zero.best_val, zero.best_idx) == (two.best_val, two.best_idx)
    m.close()


# ---- 5. failed rows -----------------------------------------------------------------------------------------------------------------
def test_failed_rows_and_the_untouched_model(bohip):
    kern, N, d, R = "SEArd", 65, 8, 700
    X, y, Xs, Theta, refs, mu_r, var_r = twin_moments(kern, N, d, R)
    m = model_of(bohip, kern, X, y)
    m.fit_()
    alpha0, mll0, refits0 = m.alpha(), m.mll(), m.info(bohip._lib.INFO_REFITS)
    p = [float(np.median(y))]
    bad = Theta.copy()
    bad[1, 2] = np.nan
    res = m.score_ensemble("EI", p, Xs.T, bad, want_each=True, want_moments=True)
    assert res.pivot.tolist() == [0, 1, 0]
    assert np.all(np.isnan(res.each[1])) and np.all(np.isnan(res.mu[1])) and np.all(np.isnan(res.var[1]))
    each_r = np.array([er.from_moments("EI", p, mu_r[h], var_r[h]) for h in range(3)])
    tol = check_rows(res, refs, mu_r, var_r, each_r, N, "one NaN row", rows=(0, 2))
    ref = er.score_ens(kern, X, y, bad, "EI", p, Xs)
    assert ref["pivot"].tolist() == [0, 1, 0]
    close(res.scores, ref["scores"], (tol[0] + tol[2]) / 2.0, "average over the two survivors")
    assert (res.best_val, res.best_idx) == first_argmax(res.scores) and res.best_idx == ref["best_idx"]
    allbad = Theta.copy()
    allbad[:, 0] = [np.nan, np.inf, -np.inf]
    with pytest.raises(bohip.NotPositiveDefinite) as e:
        m.score_ensemble("EI", p, Xs.T, allbad)
    assert e.value.code == bohip._lib.E_NOTPD
    np.testing.assert_array_equal(m.alpha(), alpha0)                # the resident model: the same bytes
    assert m.mll() == mll0 and m.info(bohip._lib.INFO_REFITS) == refits0
    assert (m.kernel.ll.tolist(), m.kernel.lsigma, m.logNoise, m.mean.beta) == (centre(kern, d)[2:-1].tolist(), 0.3, -1.5, 0.2)
    m.close()


# ---- 6. limits and errors -----------------------------------------------------------------------------------------------------------
def raw(bohip, m, acq_id, H, Theta, w, Xs, R):
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)   # noqa: E731
    prm, best, sc = np.zeros(2), bohip._lib.Best(), np.zeros(max(R, 1))
    rc = m._lib.bohip_gp_score_ens(m._h, acq_id, ptr(prm), H, ptr(Theta), ptr(w), ptr(Xs), R, ptr(sc), None, None, None, None, C.byref(best))
    return rc, m._lib.bohip_last_error().decode()


def test_limits_and_errors(bohip):
    L = bohip._lib
    kern, d = "Mat52Ard", 3
    X, y, Xs = synth(513, d, 40, seed=2)
    Theta = settings(kern, d, 2, seed=6)
    big = model_of(bohip, kern, X, y)
    rc, msg = raw(bohip, big, L.ACQ["EI"], 2, Theta, None, Xs, 40)
    assert rc == L.E_UNSUPPORTED and "512" in msg
    p = [float(np.median(y))]
    res = big.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)       # the host route: any N
    assert res.route == "host" and np.all(res.pivot == 0)
    ref = er.score_ens(kern, X, y, Theta, "EI", p, Xs)
    tol = check_rows(res, ref["models"], ref["mu"], ref["var"], ref["each"], 513, "host route N=513")
    close(res.scores, ref["scores"], tol.sum(axis=0) / 2.0, "host route scores")
    assert res.best_idx == ref["best_idx"]
    c = centre(kern, d)
    assert (big.kernel.ll.tolist(), big.kernel.lsigma, big.logNoise, big.mean.beta) == (c[2:-1].tolist(), c[-1], c[0], c[1])
    big.close()
    m = model_of(bohip, kern, X[:20], y[:20])
    for args, word in (((L.ACQ["ThompsonDraw"], 2, Theta, None, Xs, 40), "acq_id"), ((99, 2, Theta, None, Xs, 40), "acq_id"),
                       ((L.ACQ["EI"], 0, Theta, None, Xs, 40), "H must"), ((L.ACQ["EI"], 2, Theta, None, Xs, 0), "R must"),
                       ((L.ACQ["EI"], 2, Theta, [1.0, -0.5], Xs, 40), "weights"), ((L.ACQ["EI"], 2, Theta, [1.0, np.nan], Xs, 40), "weights"),
                       ((L.ACQ["EI"], 2, Theta, [0.0, 0.0], Xs, 40), "sum to 0"), ((L.ACQ["EI"], 2, None, None, Xs, 40), "null")):
        rc, msg = raw(bohip, m, *args)
        assert rc == L.E_ARG and word in msg, (args[0], args[1], msg)
    empty = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.Mat52Ard(np.zeros(d), 0.0), capacity=8)
    rc, msg = raw(bohip, empty, L.ACQ["EI"], 2, Theta, None, Xs, 40)
    assert rc == L.E_STATE and "no observations" in msg
    empty.close()
    ok = m.score_ensemble("EI", p, Xs.T, Theta)                     # the handle works on
    assert ok.best_idx >= 0 and np.all(np.isfinite(ok.scores))
    m.close()


# ---- 7. through the loop ------------------------------------------------------------------------------------------------------------
def test_bopt_loop_with_the_marginalised_acquisition(bohip):
    from test_bo_loop_gpu import branin

    lb, ub = [-5.0, 0.0], [10.0, 15.0]
    nb, mb, kb = [-4.0, 3.0], [[-20.0], [0.0]], [[-1.0, -1.0, 0.0], [4.0, 4.0, 10.0]]
    model = bohip.ElasticGPE(2, mean=bohip.MeanConst(-10.0), kernel=bohip.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=64)
    mo = bohip.MarginalGPOptimizer(every=5, samples=8, burn=5, seed=1, noisebounds=nb, meanbounds=mb, kernbounds=kb)
    opt = bohip.BOpt(lambda x: branin(x), model, bohip.Marginalised(bohip.ExpectedImprovement()), mo, lb, ub, sense=bohip.Min,
                     verbosity=bohip.Silent, rng=np.random.default_rng(5), maxiterations=15, initializer_iterations=10,
                     acquisitionoptions=dict(restarts=2, maxeval=500))
    model.enable_timing(True)
    calls, real = [], model.score_ensemble

    def spy(*a, **k):
        res = real(*a, **k)
        calls.append((np.asarray(a[2]).shape, a[3].shape, res.route, sorted({name for name, _ in model.timing()})))
        return res

    model.score_ensemble = spy
    bohip.boptimize_(opt)
    assert len(model.y) == 15 and len(calls) == 10                  # five proposals, two restarts each
    assert all(c == ((2, 500), (8, 5), "device", ["ens_factor", "ens_reduce", "ens_score"]) for c in calls), calls[0]
    Theta, w = model.hyper_samples
    assert Theta.shape == (8, 5) and mo.i == 6                      # sampled after the initial design and after the fifth proposal
    np.testing.assert_array_equal(w, np.full(8, 0.125))
    lo = np.array([nb[0], mb[0][0]] + kb[0])
    hi = np.array([nb[1], mb[1][0]] + kb[1])
    assert np.all(Theta >= lo) and np.all(Theta <= hi) and len({tuple(t) for t in Theta}) == 8
    mine = np.concatenate([[model.logNoise, model.mean.beta], model.kernel.ll, [model.kernel.lsigma]])
    assert any(np.array_equal(mine, t) for t in Theta)              # the model sits at one of its samples
    new = model.x[:, 10:]
    assert np.all(new >= np.array(lb)[:, None]) and np.all(new <= np.array(ub)[:, None])
    model.close()
