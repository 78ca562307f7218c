"""bohip_gp_score_ens_grad (kernels_ens.hip: k_ens_alpha, k_ens_grad, k_ens_reduce_grad): the gradient of the marginalised acquisition,
the factor reuse across calls, and the "refine" ascent of acquire_max.

Shapes: the smallest that cross the 16-row block (1, 2, 17, 65), the 16-candidate tile (R = 1, 17, 40), every dimension bucket
(d = 1, 2, 3, 8, 17, 33) and reach the LDS plan's cap (N = 512).  Reference: the NumPy twin (tests/ens_grad_reference.py), itself
checked against central differences in tests/test_ens_grad_host.py.  Per-setting gradient tolerance: that of
tests/test_matern_gpu.py::test_score_grad against the same twin, rtol 1e-6 and atol 1e-9 max|g_ref| + 1e-12; the average is a convex
combination of the per-setting gradients, so its bound is the same combination of theirs."""
import functools
import math

import numpy as np
import pytest

import ens_grad_reference as eg
import ens_reference as er
from conftest import synth
from test_ens_gpu import ACQS, SHAPES, check_rows, close, launches, params, score_tols
from test_fit_gpu import centre, model_of, settings
from test_parity_gpu import bohip, mu_floor  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

CASES = [(k, N, d, R) for (N, d), ks in SHAPES.items() for k in ks for R in (1, 17, 40)]


@functools.lru_cache(maxsize=None)
def twin_case(kern, N, d, R, H=3):
    """(X, y, Xs, Theta, row models) of one case: computed once, never written to."""
    X, y, Xs = synth(N, d, R, seed=2000 + 7 * N + 3 * d + R)
    Theta = settings(kern, d, H, seed=N + d)
    refs = [er.row_model(kern, X, y, t) for t in Theta]
    for a in (X, y, Xs, Theta):
        a.setflags(write=False)
    return X, y, Xs, Theta, refs


@functools.lru_cache(maxsize=None)
def twin_grads(kern, N, d, R, acq, p):
    """(each[H, R], each_grad[H, R, d]) of the twin for one case and acquisition."""
    X, y, Xs, Theta, refs = twin_case(kern, N, d, R)
    sg = [eg.row_score_grad(r, acq, list(p), Xs) for r in refs]
    out = np.array([s for s, _ in sg]), np.array([g for _, g in sg])
    for a in out:
        a.setflags(write=False)
    return out


def grad_tols(g_ref):
    """[H, R, d] bounds of the per-setting gradients."""
    return np.array([1e-6 * np.abs(g) + 1e-9 * np.abs(g).max() + 1e-12 for g in g_ref])


def avg(arr, w):
    """ens_reference.average over the leading axis of an [H, ...] array, every row alive."""
    H = arr.shape[0]
    return er.average(arr.reshape(H, -1), w, np.zeros(H, dtype=np.int64)).reshape(arr.shape[1:])


# ---- 1. parity with the twin, 2. the values are score_ens's ------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d,R", CASES)
def test_gradient_matches_the_twin_and_values_are_score_ens(bohip, kern, N, d, R):
    X, y, Xs, Theta, refs = twin_case(kern, N, d, R)
    m = model_of(bohip, kern, X, y)
    for acq, p in ACQS:
        p = params(p, y)
        what = f"{kern} N={N} d={d} R={R} {acq}"
        res, grad, each_grad = m.score_ensemble_grad(acq, p, Xs.T, Theta, want_each=True)
        assert res.route == "device" and np.all(res.pivot == 0)
        assert grad.shape == (d, R) and each_grad.shape == (3, d, R)
        each_r, g_r = twin_grads(kern, N, d, R, acq, tuple(p))
        tol = grad_tols(g_r)
        for h in range(3):
            close(each_grad[h].T, g_r[h], tol[h], f"{what} each_grad[{h}]")
        close(grad.T, avg(g_r, None), tol.sum(axis=0) / 3.0, f"{what} grad")
        val = m.score_ensemble(acq, p, Xs.T, Theta, want_each=True, want_moments=True)
        np.testing.assert_array_equal(res.scores, val.scores)
        np.testing.assert_array_equal(res.each, val.each)
        np.testing.assert_array_equal(res.pivot, val.pivot)
        assert (res.best_val, res.best_idx) == (val.best_val, val.best_idx)
        o = raw_grad(bohip, m, acq, p, Xs, Theta)                   # every output of the symbol, mu and var among them
        assert o["rc"] == 0
        for name in ("scores", "each", "mu", "var", "pivot"):
            np.testing.assert_array_equal(o[name], getattr(val, name), err_msg=f"{what} {name}")
        assert o["best"] == (val.best_val, val.best_idx)
        np.testing.assert_array_equal(o["grad"], grad.T)
        np.testing.assert_array_equal(o["each_grad"], each_grad.transpose(0, 2, 1))
    m.close()


def raw_grad(bohip, m, acq, p, Xs, Theta, w=None):
    """Every output of the symbol: dict(scores, grad[R, d], each, each_grad[H, R, d], mu, var, pivot, best)."""
    import ctypes as C

    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    Xs, Theta = np.ascontiguousarray(Xs, dtype=np.float64), np.ascontiguousarray(Theta, dtype=np.float64)
    R, d = Xs.shape
    H = Theta.shape[0]
    prm = np.concatenate([np.asarray(p, dtype=np.float64), np.zeros(2)])[:2].copy()
    o = dict(scores=np.empty(R), grad=np.empty((R, d)), each=np.empty((H, R)), each_grad=np.empty((H, R, d)), mu=np.empty((H, R)),
             var=np.empty((H, R)), pivot=np.zeros(H, dtype=np.int64))
    best = bohip._lib.Best()
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    rc = m._lib.bohip_gp_score_ens_grad(m._h, bohip._lib.ACQ[acq], ptr(prm), H, ptr(Theta), ptr(w), ptr(Xs), R, ptr(o["scores"]), ptr(o["grad"]),
                                        ptr(o["each"]), ptr(o["each_grad"]), ptr(o["mu"]), ptr(o["var"]),
                                        o["pivot"].ctypes.data_as(C.POINTER(C.c_int64)), C.byref(best))
    o["rc"], o["best"] = rc, (best.val, best.idx)
    return o


def test_candidates_beyond_one_chunk(bohip, monkeypatch):
    """R = 16384 + 77 is two candidate chunks inside the call (the gradient counterpart of tests/test_ens_gpu.py's test); with the
    workspace capped as well, every chunk factors the settings one launch at a time.  The same bytes as the calls on the two parts and
    as the uncapped call, the values those of score_ensemble, and 48 candidates on both sides of the chunk boundary against the twin."""
    kern, N, d, R = "Mat52Iso", 200, 17, 16384 + 77
    X, y, Xs, Theta, refs = twin_case(kern, N, d, R)
    p = [float(np.median(y))]
    m = model_of(bohip, kern, X, y)
    m.enable_timing(True)
    full = raw_grad(bohip, m, "EI", p, Xs, Theta)
    assert full["rc"] == 0 and launches(m, "ens_factor") == 1 and launches(m, "ens_alpha") == 1 and launches(m, "ens_grad") == 2
    val = m.score_ensemble("EI", p, Xs.T, Theta, want_each=True, want_moments=True)
    for name in ("scores", "each", "mu", "var", "pivot"):
        np.testing.assert_array_equal(full[name], getattr(val, name))
    assert full["best"] == (val.best_val, val.best_idx)
    for lo, hi in ((0, 16384), (16384, R)):
        part = raw_grad(bohip, m, "EI", p, Xs[lo:hi], Theta)
        assert part["rc"] == 0
        np.testing.assert_array_equal(part["grad"], full["grad"][lo:hi])
        np.testing.assert_array_equal(part["each_grad"], full["each_grad"][:, lo:hi])
        np.testing.assert_array_equal(part["scores"], full["scores"][lo:hi])
    sub = np.r_[0:8, 16376:16400, R - 16:R]
    ref = eg.score_ens_grad(kern, X, y, Theta, "EI", p, Xs[sub])
    tol = grad_tols(ref["each_grad"])
    for h in range(3):
        close(full["each_grad"][h][sub], ref["each_grad"][h], tol[h], f"two chunks each_grad[{h}]")
    close(full["grad"][sub], ref["grad"], tol.sum(axis=0) / 3.0, "two chunks grad")
    monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")
    capped = raw_grad(bohip, m, "EI", p, Xs, Theta)
    assert capped["rc"] == 0
    assert launches(m, "ens_factor") == 6 and launches(m, "ens_alpha") == 6 and launches(m, "ens_grad") == 6   # three settings, one at a time, per chunk
    for name in ("scores", "grad", "each", "each_grad", "mu", "var", "pivot"):
        np.testing.assert_array_equal(capped[name], full[name])
    assert capped["best"] == full["best"]
    m.close()


@pytest.mark.parametrize("kern", ["SEArd", "Mat32Ard"])
def test_the_lds_plan_at_its_largest(bohip, kern):
    """N = 512 and d = 64 together: the 156 800 bytes of LDS the plan tops out at (both family instantiations of the widest bucket)."""
    N, d, R = 512, 64, 17
    X, y, Xs, Theta, refs = twin_case(kern, N, d, R)
    m = model_of(bohip, kern, X, y)
    for acq, p in (("UCB", [2.5]), ("EI", None)):
        p = params(p, y)
        res, grad, each_grad = m.score_ensemble_grad(acq, p, Xs.T, Theta, want_each=True)
        assert np.all(res.pivot == 0)
        each_r, g_r = twin_grads(kern, N, d, R, acq, tuple(p))
        tol = grad_tols(g_r)
        for h in range(3):
            close(each_grad[h].T, g_r[h], tol[h], f"{kern} N=512 d=64 {acq} each_grad[{h}]")
        close(grad.T, avg(g_r, None), tol.sum(axis=0) / 3.0, f"{kern} N=512 d=64 {acq} grad")
        val = m.score_ensemble(acq, p, Xs.T, Theta, want_each=True)
        np.testing.assert_array_equal(res.scores, val.scores)
        np.testing.assert_array_equal(res.each, val.each)
    m.close()


# ---- 3. position independence, bitwise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d", [("Mat52Ard", 200, 17), ("SEArd", 65, 8), ("Mat12Iso", 17, 3)])
def test_a_gradient_depends_on_its_setting_and_its_candidate_only(bohip, kern, N, d, monkeypatch):
    X, y, Xs, _, _ = twin_case(kern, N, d, 40)
    Theta = settings(kern, d, 5, seed=77)
    p = [float(np.median(y))]
    m = model_of(bohip, kern, X, y)
    m.enable_timing(True)
    full, g_full, eg_full = m.score_ensemble_grad("EI", p, Xs.T, Theta, want_each=True)
    assert launches(m, "ens_factor") == 1 and launches(m, "ens_alpha") == 1 and launches(m, "ens_grad") == 1
    for j in (0, 15, 16, 39):                                       # a candidate alone; slots 0 and 15 of a tile; a later tile
        one, g1, eg1 = m.score_ensemble_grad("EI", p, Xs[j:j + 1].T, Theta, want_each=True)
        np.testing.assert_array_equal(eg1[:, :, 0], eg_full[:, :, j])
        np.testing.assert_array_equal(g1[:, 0], g_full[:, j])
        assert one.scores[0] == full.scores[j]
    moved = np.roll(Xs, 5, axis=0)                                  # every candidate at another slot (row j + 5 holds candidate j)
    _, g_mv, eg_mv = m.score_ensemble_grad("EI", p, moved.T, Theta, want_each=True)
    np.testing.assert_array_equal(np.roll(eg_mv, -5, axis=2), eg_full)
    np.testing.assert_array_equal(np.roll(g_mv, -5, axis=1), g_full)
    for h in (0, 3):                                                # the same setting alone ...
        _, _, eg_one = m.score_ensemble_grad("EI", p, Xs.T, Theta[h:h + 1], want_each=True)
        np.testing.assert_array_equal(eg_one[0], eg_full[h])
    perm = np.array([3, 4, 0, 2, 1])                                # ... and at another position, next to a failed row
    bad = Theta[perm].copy()
    bad[3, 0] = np.nan
    other, g_o, eg_o = m.score_ensemble_grad("EI", p, Xs.T, bad, want_each=True)
    assert other.pivot.tolist() == [0, 0, 0, 1, 0]
    assert np.all(np.isnan(eg_o[3])) and np.all(np.isnan(other.each[3]))
    for k in (0, 1, 2, 4):
        np.testing.assert_array_equal(eg_o[k], eg_full[perm[k]])
    ref = eg.score_ens_grad(kern, X, y, bad, "EI", p, Xs)           # the average over the survivors, against the twin
    assert ref["pivot"].tolist() == [0, 0, 0, 1, 0]
    alive = [0, 1, 2, 4]
    tol = grad_tols(ref["each_grad"][alive])
    close(g_o.T, ref["grad"], tol.sum(axis=0) / 4.0, "average over the four survivors")
    M = -(-N // 16) * 16
    slab_mb = (2 * M + 1) * (M + 8) * 8 / 2 ** 20
    monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")                  # read at every call
    assert 2 * slab_mb > 1.0 or N < 100                             # (at N = 200 one setting fits, two do not: 5 launches)
    capped, g_c, eg_c = m.score_ensemble_grad("EI", p, Xs.T, Theta, want_each=True)
    if N >= 100:
        assert launches(m, "ens_factor") == 5 and launches(m, "ens_alpha") == 5 and launches(m, "ens_grad") == 5
    np.testing.assert_array_equal(eg_c, eg_full)
    np.testing.assert_array_equal(g_c, g_full)
    for name in ("scores", "each", "pivot"):
        np.testing.assert_array_equal(getattr(capped, name), getattr(full, name))
    assert (capped.best_val, capped.best_idx) == (full.best_val, full.best_idx)
    m.close()


# ---- 4. factor reuse --------------------------------------------------------------------------------------------------------------------
def test_factor_reuse(bohip):
    kern, N, d, R = "Mat52Ard", 65, 8, 17
    X, y, Xs, Theta, refs = twin_case(kern, N, d, R)
    Theta = Theta.copy()
    p = [float(np.median(y))]
    m = model_of(bohip, kern, X, y, capacity=128)
    m.enable_timing(True)

    def call(T=None, xs=Xs):
        res, g, e = m.score_ensemble_grad("EI", p, xs.T, Theta if T is None else T, want_each=True)
        names = [n for n, _ in m.timing()]
        return res, g, e, names.count("ens_factor"), names

    def against_twin(g, e, Xo, yo, T, what):
        ref = eg.score_ens_grad(kern, Xo, yo, T, "EI", p, Xs)
        tol = grad_tols(ref["each_grad"])
        for h in range(3):
            close(e[h].T, ref["each_grad"][h], tol[h], f"{what} each_grad[{h}]")
        close(g.T, ref["grad"], tol.sum(axis=0) / 3.0, f"{what} grad")

    r1, g1, e1, nf, names = call()
    assert nf == 1 and names.count("ens_alpha") == 1 and "ens_grad" in names and "ens_reduce" in names
    against_twin(g1, e1, X, y, Theta, "cold")
    r2, g2, e2, nf, names = call()                                  # the same Theta: no factor stage, identical bytes
    assert nf == 0 and "ens_alpha" not in names and "ens_grad" in names
    for a, b in ((g1, g2), (e1, e2), (r1.scores, r2.scores), (r1.each, r2.each)):
        np.testing.assert_array_equal(a, b)
    _, g3, e3, nf, _ = call(xs=Xs[::-1])                            # other candidates, the same Theta: still reused
    assert nf == 0
    np.testing.assert_array_equal(e3[:, :, ::-1], e1)
    T2 = Theta.copy()                                               # one entry of theta changed
    T2[1, 3] += 1e-3
    _, g, e, nf, _ = call(T2)
    assert nf == 1
    against_twin(g, e, X, y, T2, "theta changed")
    assert call(T2)[3] == 0
    m.mll_grad_batch(Theta)                                         # the fit's batch writes the slabs
    _, g, e, nf, _ = call(T2)
    assert nf == 1
    against_twin(g, e, X, y, T2, "after mll_grad_batch")
    assert call(T2)[3] == 0
    m.score_ensemble("EI", p, Xs.T, T2)                             # so does score_ensemble
    _, g, e, nf, _ = call(T2)
    assert nf == 1
    against_twin(g, e, X, y, T2, "after score_ensemble")
    assert call(T2)[3] == 0
    xn, yn = np.full(d, 0.37), 0.25                                 # one more observation
    m.append_(xn[:, None], [yn])
    _, g, e, nf, _ = call(T2)
    assert nf == 1
    against_twin(g, e, np.vstack([X, xn]), np.append(y, yn), T2, "after append_")
    m.close()


# ---- 5. Matérn 1/2 on an observation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["Mat12Ard", "Mat12Iso"])
def test_mat12_gradient_on_an_observation(bohip, kern):
    N, d, R = 65, 3, 17
    X, y, Xs, Theta, refs = twin_case(kern, N, d, R)
    Xs = Xs.copy()
    Xs[1], Xs[16] = X[17], X[64]
    m = model_of(bohip, kern, X, y)
    for acq, p in (("UCB", [2.5]), ("EI", [float(np.median(y))])):
        _, g, e = m.score_ensemble_grad(acq, p, Xs.T, Theta, want_each=True)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(e))
        ref = eg.score_ens_grad(kern, X, y, Theta, acq, p, Xs)
        tol = grad_tols(ref["each_grad"])
        for h in range(3):
            close(e[h].T, ref["each_grad"][h], tol[h], f"{kern} {acq} on an observation each_grad[{h}]")
        close(g.T, ref["grad"], tol.sum(axis=0) / 3.0, f"{kern} {acq} on an observation grad")
    m.close()


# ---- 6. sigma^2 = 0, and LogEI where EI is dead ------------------------------------------------------------------------------------------
def test_clamped_variance_drops_the_variance_term_for_that_setting_only(bohip):
    """Setting 1 is all but noiseless (noise = e^-40 + eps) and the first candidates ARE observations: there its sigma^2 = s_f^2 - |V|^2
    rounds to 0 or below and is clamped.  Where the device's own variance is exactly 0 the setting's gradient is da/dmu grad mu alone
    (UCB: grad mu); the other settings keep both terms."""
    kern, N, d, R = "Mat12Ard", 40, 2, 17                           # (exp(-rho): well conditioned without noise, nothing fails)
    X, y, Xs, Theta, _ = twin_case(kern, N, d, R)
    Xs, Theta = Xs.copy(), Theta.copy()
    Xs[:8] = X[:8]
    Theta[1, 0] = -20.0
    m = model_of(bohip, kern, X, y)
    o = raw_grad(bohip, m, "UCB", [2.5], Xs, Theta)
    mm = raw_grad(bohip, m, "MaxMean", [], Xs, Theta)               # da/dmu = 1, no variance term: grad mu itself
    assert o["rc"] == 0 and mm["rc"] == 0 and np.all(o["pivot"] == 0)
    zero = o["var"][1] == 0.0
    print("clamped at", np.flatnonzero(zero))
    assert zero[:8].any()                                           # the construction holds on the device
    np.testing.assert_array_equal(o["each_grad"][1][zero], mm["each_grad"][1][zero])
    pos = ~zero
    assert np.all(o["var"][0] > 0) and np.all(o["var"][2] > 0)
    assert np.all(np.any(o["each_grad"][0] != mm["each_grad"][0], axis=1))   # the other settings: the variance term is there
    assert np.all(np.any(o["each_grad"][1][pos] != mm["each_grad"][1][pos], axis=1))
    assert np.all(np.isfinite(o["grad"]))
    m.close()


def test_logei_gradient_where_ei_is_dead(bohip):
    from test_logei_gpu import dead_ei_problem

    X, y, starts = dead_ei_problem(40)
    c = np.array([-3.0, 0.0, math.log(0.3), math.log(0.3), math.log(0.1)])
    Theta = c + np.random.default_rng(3).uniform(-0.1, 0.1, (3, c.size))
    m = model_of(bohip, "SEArd", X, y, theta=c)
    p = [float(y.max())]
    Xs = np.ascontiguousarray(starts.T)
    ei, g_ei, _ = m.score_ensemble_grad("EI", p, starts, Theta, want_each=True)
    le, g_le, e_le = m.score_ensemble_grad("LogEI", p, starts, Theta, want_each=True)
    assert np.all(ei.scores == 0.0) and np.all(g_ei == 0.0)         # EI is dead here: nothing to climb
    assert np.all(np.isfinite(le.scores)) and np.all(np.isfinite(g_le)) and np.all(np.abs(g_le).max(axis=0) > 0)
    ref = eg.score_ens_grad("SEArd", X, y, Theta, "LogEI", p, Xs)
    tol = grad_tols(ref["each_grad"])
    for h in range(3):
        close(e_le[h].T, ref["each_grad"][h], tol[h], f"LogEI where EI is dead each_grad[{h}]")
    close(g_le.T, ref["grad"], tol.sum(axis=0) / 3.0, "LogEI where EI is dead grad")
    m.close()


# ---- 7. the ascent -----------------------------------------------------------------------------------------------------------------------
# Seeds: chosen on the CPU with the HOST route on the twin (tests/test_ens_grad_host.py's DuckGradModel with bohip.model's
# score_ensemble / score_ensemble_grad, no device): seed 0 gives, for refine = 0 -> refine = 4,
#   d = 2:  2.14349862 -> 2.16031796  (rise 1.7e-2, the two score tolerances 2.1e-6 and 2.2e-6), maximiser (0.5208, 0.5896)
#   d = 8:  8.60888278 -> 9.67079717  (rise 1.06, tolerances 8.6e-6 and 9.7e-6), an interior maximiser
# so the strict rise is there without a device and the device test cannot pass by equality.  (Seeds 1-3 rise as well.)
ASCENT = {2: 0, 8: 0}


def ascent_problem(d):
    N, H = 40, 4
    X, y, _ = synth(N, d, 1, seed=50 + d)
    kern = "Mat52Ard"
    Theta = settings(kern, d, H, seed=60 + d)
    return kern, X, y, Theta


@pytest.mark.parametrize("d", [2, 8])
def test_refine_climbs_above_the_candidate_maximum(bohip, d):
    from bohip.acquisition import Marginalised, UpperConfidenceBound, NoBetaScaling, acquire_max

    kern, X, y, Theta = ascent_problem(d)
    w = np.full(4, 0.25)
    m = model_of(bohip, kern, X, y)
    m.hyper_samples = (Theta, w)
    m.enable_timing(True)
    a = Marginalised(UpperConfidenceBound(NoBetaScaling(), 2.0))
    lb, ub = np.zeros(d), np.ones(d)
    opts = dict(restarts=1, maxeval=256)
    f0, x0 = acquire_max(a, m, lb, ub, opts, np.random.default_rng(ASCENT[d]), setparams=False)
    factors, real_v, real_g = [], m.score_ensemble, m.score_ensemble_grad

    def spy_v(*args, **kw):
        res = real_v(*args, **kw)
        factors.append(launches(m, "ens_factor"))
        return res

    def spy_g(*args, **kw):
        res = real_g(*args, **kw)
        factors.append(launches(m, "ens_factor"))
        return res

    m.score_ensemble, m.score_ensemble_grad = spy_v, spy_g
    f4, x4 = acquire_max(a, m, lb, ub, {**opts, "refine": 4}, np.random.default_rng(ASCENT[d]), setparams=False)
    m.score_ensemble, m.score_ensemble_grad = real_v, real_g
    assert len(factors) > 2 and sum(factors) == 2 and factors[:2] == [1, 1]     # the candidate stage, and the first gradient call
    assert np.all(x4 >= lb) and np.all(x4 <= ub)
    p = a.params()

    def twin_at(x):
        ref = er.score_ens(kern, X, y, Theta, "UCB", p, x[None, :], w)
        tol = score_tols(ref["models"], ref["each"])
        return ref["scores"][0], float((w[:, None] * tol).sum(axis=0)[0])

    s4, t4 = twin_at(x4)
    s0, t0 = twin_at(x0)
    print(f"d={d}: refine=0 f {f0:.12g}, refine=4 f {f4:.12g}, rise {f4 - f0:.3g}, tolerances {t0:.3g} {t4:.3g}")
    assert abs(f4 - s4) <= t4 and abs(f0 - s0) <= t0
    assert f4 >= f0
    assert f4 - f0 > t0 + t4
    m.close()


# ---- 8. through the loop -------------------------------------------------------------------------------------------------------------------
def test_bopt_loop_with_refine(bohip):
    from test_bo_loop_gpu import branin

    lb, ub = [-5.0, 0.0], [10.0, 15.0]
    nb, mb, kb = [-4.0, 3.0], [[-20.0], [0.0]], [[-1.0, -1.0, 0.0], [4.0, 4.0, 10.0]]
    model = bohip.ElasticGPE(2, mean=bohip.MeanConst(-10.0), kernel=bohip.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=64)
    mo = bohip.MarginalGPOptimizer(every=5, samples=8, burn=5, seed=1, noisebounds=nb, meanbounds=mb, kernbounds=kb)
    opt = bohip.BOpt(lambda x: branin(x), model, bohip.Marginalised(bohip.ExpectedImprovement()), mo, lb, ub, sense=bohip.Min,
                     verbosity=bohip.Silent, rng=np.random.default_rng(5), maxiterations=15, initializer_iterations=10,
                     acquisitionoptions=dict(restarts=1, maxeval=200, refine=4))
    calls, real = [], model.score_ensemble_grad

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((np.asarray(a[2]).shape, out[0].route))
        return out

    model.score_ensemble_grad = spy
    bohip.boptimize_(opt)
    assert len(model.y) == 15 and len(calls) >= 5                   # five proposals, every one with an ascent
    assert all(c == ((2, 4), "device") for c in calls), calls[0]
    new = model.x[:, 10:]
    assert np.all(new >= np.array(lb)[:, None]) and np.all(new <= np.array(ub)[:, None]) and np.all(np.isfinite(model.y))
    model.close()
