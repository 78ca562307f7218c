"""The leave-one-out objective at H settings in one launch (include/bohip_loo_batch.h) against the NumPy twin of the
resident path (tests/loo_reference.py), which is computed once per (shape, kernel) and shared.

Shapes (N, d) are the smallest at which the one-workgroup kernel takes another path: (1, 1) and (2, 2) live inside one block with
padding; (16, 2) is one full block with none; (17, 3) has fifteen padding rows and a second panel; (65, 8) leaves the 64-column
mapping (CW = 128); (129, 8) has CW = 256; (257, 17) has CW = 512 and the 32-wide dimension bucket; 512 is the cap.
Bounds are tests/test_loo_gpu.py's check_grad: total 1e-9 relative, gradient rtol 1e-6 with the floor 1e-8 max|g_ref|; logp 1e-9 of
its largest magnitude."""
import ctypes as C
import math

import numpy as np
import pytest

import loo_reference as lr
from conftest import synth
from matern_reference import KERNELS
from test_loo_gpu import BETA, BOUNDS, STRESS, check_grad, fit_problem, model_of, params_of, theta
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ALL = list(KERNELS)
H = 5
SHAPES = {(1, 1): ["SEArd", "Mat12Iso"], (2, 2): ["SEIso", "Mat32Ard"], (16, 2): ["Mat52Ard", "Mat12Ard"],
          (17, 3): ["Mat52Ard", "Mat32Iso"], (65, 8): ALL, (129, 8): ["SEArd", "Mat52Iso"], (257, 17): ["Mat52Ard", "Mat12Iso"]}
CASES = [(k, N, d) for (N, d), ks in SHAPES.items() for k in ks]
MEAN_ZERO = ("Mat32Iso", 17, 3)


def settings(kern, d, n, seed, centre=None, beta=BETA):
    """n settings spread around a centre (the first is the centre itself)."""
    c = theta(kern, d, beta=beta) if centre is None else centre
    rng = np.random.default_rng(seed)
    T = c + 0.3 * rng.uniform(-1.0, 1.0, (n, c.size))
    T[0] = c
    return T


def check_rows(res, kern, X, y, Theta, what):
    total, G, piv, logp = res
    assert np.all(piv == 0), (what, piv)
    for h, t in enumerate(Theta):
        ref = lr.grad_vec(kern, X, y, t)
        check_grad((total[h], G[h, 0], G[h, 1], G[h, 2:]), ref, f"{what} row {h}")
        lp = lr.loo_fast(kern, X, y, t[2:-1], t[-1], t[0], t[1])[2]
        err = np.abs(logp[h] - lp).max()
        print(f"{what} row {h}: logp max err {err:.3e} / {np.abs(lp).max():.3e}")
        assert err <= 1e-9 * np.abs(lp).max(), what


# ---- 1. parity over shapes, kernels, means ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d", CASES)
def test_rows_match_the_twin(bohip, kern, N, d):
    X, y, _ = synth(N, d, 1, seed=500 + N)
    mean_const = (kern, N, d) != MEAN_ZERO
    Theta = settings(kern, d, H, seed=N + d, beta=BETA if mean_const else 0.0)
    if not mean_const:
        Theta[:, 1] = 0.0                                          # a MeanZero model passes mean = 0; its slot is still filled
    m = model_of(bohip, kern, X, y, Theta[0], mean_const)
    check_rows(m.loo_grad_batch(Theta, want_logp=True), kern, X, y, Theta, f"{kern} N={N} d={d}")
    m.close()


def test_the_size_cap(bohip):
    from bohip import _lib

    X, y, _ = synth(513, 4, 1, seed=12)
    Theta = settings("Mat52Ard", 4, 2, seed=3)
    m = model_of(bohip, "Mat52Ard", X[:512], y[:512], Theta[0], capacity=513)
    check_rows(m.loo_grad_batch(Theta, want_logp=True), "Mat52Ard", X[:512], y[:512], Theta, "Mat52Ard N=512 d=4")
    m.append_(X[512:].T, y[512:])
    with pytest.raises(bohip.BohipError) as e:
        m.loo_grad_batch(Theta)
    assert e.value.code == _lib.E_UNSUPPORTED and "512" in str(e.value) and "bohip_gp_loo_grad" in str(e.value)
    m.close()


@pytest.mark.parametrize("kern,N,d", [("SEArd", 17, 3), ("Mat12Ard", 65, 8), ("Mat52Iso", 129, 8), ("Mat32Ard", 257, 17)])
def test_rows_match_the_resident_path(bohip, kern, N, d):
    X, y, _ = synth(N, d, 1, seed=700 + N)
    Theta = settings(kern, d, 3, seed=N)
    m = model_of(bohip, kern, X, y, Theta[0])
    total, G, piv, logp = m.loo_grad_batch(Theta, want_logp=True)
    for h, t in enumerate(Theta):
        m.set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
        res, g = m.loo(), m.loo_grad()
        check_grad((total[h], G[h, 0], G[h, 1], G[h, 2:]), (g[0], np.concatenate([[g[1], g[2]], g[3]])), f"{kern} N={N} resident row {h}")
        assert abs(total[h] - res.total) <= 1e-9 * abs(res.total)
        assert np.abs(logp[h] - res.logp).max() <= 1e-9 * np.abs(res.logp).max()
    m.close()


@pytest.mark.parametrize("kern", ["SEArd", "Mat52Ard"])
def test_stress_setting(bohip, kern):
    """DESIGN.md 6r's stress setting (lsigma = 5, logNoise = 0) at (129, 2), with the bounds tests/test_loo_gpu.py's
    test_stress_setting holds the resident path to."""
    X, y, _ = synth(129, 2, 1, seed=11)
    t = theta(kern, 2, STRESS)
    Theta = np.vstack([t, t + 0.05])
    m = model_of(bohip, kern, X, y, t)
    check_rows(m.loo_grad_batch(Theta, want_logp=True), kern, X, y, Theta, f"{kern} stress (129, 2)")
    m.close()


# ---- 2. a row is a function of (model, theta_h) ---------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_the_batch(bohip, monkeypatch):
    X, y, _ = synth(65, 3, 1, seed=2)
    others = settings("Mat52Ard", 3, 300, seed=6)
    t = settings("Mat52Ard", 3, 2, seed=1)[1]
    m = model_of(bohip, "Mat52Ard", X, y, others[0])
    alone = m.loo_grad_batch(t[None], want_logp=True)
    first = m.loo_grad_batch(np.vstack([t, others[:2]]), want_logp=True)
    big = np.vstack([others[:299], t])
    last = m.loo_grad_batch(big, want_logp=True)                  # more workgroups than compute units
    monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")                # 9 settings per launch: 34 consecutive launches inside the call
    chunked = m.loo_grad_batch(big, want_logp=True)
    monkeypatch.delenv("BOHIP_FIT_WS_MAX_MB")
    for res, row in ((first, 0), (last, 299), (chunked, 299)):
        for k in (0, 1, 3):
            assert res[k][row].tobytes() == alone[k][0].tobytes(), (row, k)
    for k in (0, 1, 2, 3):
        assert chunked[k].tobytes() == last[k].tobytes()
    # value only: the same total and logp, no gradient
    value = m.loo_grad_batch(big[290:], want_grad=False, want_logp=True)
    assert value[1] is None
    assert value[0].tobytes() == last[0][290:].tobytes() and value[3].tobytes() == last[3][290:].tobytes()
    only_total = m.loo_grad_batch(big[290:], want_grad=False)
    assert len(only_total) == 3 and only_total[0].tobytes() == value[0].tobytes()
    m.close()


# ---- 3. failed rows -----------------------------------------------------------------------------------------------------------------
def test_failed_rows_stay_alone(bohip):
    # forty observations at one point: with lsigma = 10 and logNoise = -40 every entry of cK is the same number and no pivot after
    # the first can stay a positive number for long (each is the rounding residue of the one before)
    Xd, yd = np.zeros((40, 2)), np.arange(40.0) / 10.0
    good = settings("SEArd", 2, 3, seed=5)
    m = model_of(bohip, "SEArd", Xd, yd, good[0])
    nan_row, notpd = good[1].copy(), good[1].copy()
    nan_row[2] = math.nan
    notpd[0], notpd[-1] = -40.0, 10.0
    total, G, piv, logp = m.loo_grad_batch(np.vstack([good[0], nan_row, good[1], notpd, good[2]]), want_logp=True)
    print("pivots", piv, "totals", total)
    assert piv[1] == 1 and 2 <= piv[3] <= 40 and not piv[[0, 2, 4]].any()
    assert np.all(total[[1, 3]] == -np.inf) and not G[[1, 3]].any() and np.isnan(logp[[1, 3]]).all()
    assert np.isfinite(total[[0, 2, 4]]).all() and np.isfinite(logp[[0, 2, 4]]).all()
    for row, t in ((0, good[0]), (2, good[1]), (4, good[2])):
        alone = m.loo_grad_batch(t[None], want_logp=True)
        for k in (0, 1, 3):
            assert [total, G, piv, logp][k][row].tobytes() == alone[k][0].tobytes(), (row, k)
    # value only: the same report
    total_v, _, piv_v, logp_v = m.loo_grad_batch(np.vstack([good[0], nan_row, good[1], notpd, good[2]]), want_grad=False, want_logp=True)
    assert piv_v.tobytes() == piv.tobytes() and total_v.tobytes() == total.tobytes() and logp_v.tobytes() == logp.tobytes()
    m.close()


def test_errors(bohip):
    from bohip import _lib

    X, y, _ = synth(5, 2, 1, seed=1)
    t = theta("SEArd", 2)
    m = model_of(bohip, "SEArd", X, y, t)
    dp = C.POINTER(C.c_double)
    out = np.zeros(1)
    assert m._lib.bohip_gp_loo_grad_batch(m._h, 0, t.ctypes.data_as(dp), out.ctypes.data_as(dp), None, None, None) == _lib.E_ARG
    assert m._lib.bohip_gp_loo_grad_batch(m._h, 1, t.ctypes.data_as(dp), out.ctypes.data_as(dp), None, None, None) == _lib.OK
    assert out[0] == m.loo_grad_batch(t[None])[0][0]
    with pytest.raises(ValueError, match="columns"):
        m.loo_grad_batch(np.zeros((2, 3)))
    empty = bohip.ElasticGPE(2)
    with pytest.raises(bohip.BohipError) as e:
        empty.loo_grad_batch(t[None])
    assert e.value.code == _lib.E_STATE
    m.close()


# ---- 4. the model and its caches ------------------------------------------------------------------------------------------------------
def test_the_model_is_untouched(bohip):
    X, y, Xs = synth(140, 5, 64, seed=13)
    t = theta("Mat32Ard", 5)
    m = model_of(bohip, "Mat32Ard", X[:120], y[:120], t, capacity=256)
    Theta = settings("Mat32Ard", 5, 4, seed=3)

    def state():
        mu, var = m.predict_f(Xs.T)
        sc, bv, bi = m.score("EI", [float(y.max())], Xs.T)
        lo, lg = m.loo(), m.loo_grad()
        mb = m.mll_grad_batch(Theta[:2])
        return (mu.tobytes(), var.tobytes(), sc.tobytes(), bv, bi, lo.total, lo.logp.tobytes(), lg[:3], lg[3].tobytes(), mb[0].tobytes(),
                mb[1].tobytes(), np.float64(m.mll()).tobytes(), m.alpha().tobytes(), m.factor().tobytes(), m.info(2))

    before = state()
    res = m.loo_grad_batch(Theta, want_logp=True)
    assert np.all(res[2] == 0) and state() == before
    m.loo_grad_batch(Theta[:1], want_grad=False)
    assert state() == before
    m.append_(X[120:].T, y[120:])                                 # an incremental extension, no refit after it
    before = state()
    res = m.loo_grad_batch(Theta, want_logp=True)
    assert state() == before
    check_rows(res, "Mat32Ard", X, y, Theta, "after append")       # ... and the call saw the appended rows
    m.close()


def test_the_ensemble_factor_cache_is_dropped(bohip):
    X, y, Xs = synth(65, 3, 32, seed=23)
    Theta, Theta2 = settings("SEArd", 3, 3, seed=1), settings("SEArd", 3, 3, seed=2) + 0.2
    m = model_of(bohip, "SEArd", X, y, Theta[0])
    xs = np.asfortranarray(Xs.T)
    first, g1 = m.score_ensemble_grad("EI", [float(y.max())], xs, Theta)[:2]
    m.loo_grad_batch(Theta2)                                      # writes the slabs the ensemble's factors sit in
    again, g2 = m.score_ensemble_grad("EI", [float(y.max())], xs, Theta)[:2]
    assert first.route == "device"
    assert again.scores.tobytes() == first.scores.tobytes() and g2.tobytes() == g1.tobytes()
    assert (again.best_val, again.best_idx) == (first.best_val, first.best_idx)
    m.close()


# ---- 5. the fit -------------------------------------------------------------------------------------------------------------------------
def spy_on(monkeypatch, cls, name, seen):
    real = getattr(cls, name)

    def spy(self, *a, **kw):
        seen[name] = seen.get(name, 0) + 1
        return real(self, *a, **kw)

    monkeypatch.setattr(cls, name, spy)


def test_multistart_fit_evaluates_through_the_batched_call(bohip, monkeypatch):
    from bohip import bopt
    from bohip.bopt import MAPGPOptimizer, optimizemodel_

    X, y = fit_problem()
    m = model_of(bohip, "Mat52Ard", X, y, theta("Mat52Ard", 2, beta=0.0))
    start = m.loo().total
    seen, out = {}, {}
    spy_on(monkeypatch, bohip.ElasticGPE, "loo_grad_batch", seen)
    spy_on(monkeypatch, bohip.ElasticGPE, "loo_grad", seen)
    real = bopt._multistart_map
    monkeypatch.setattr(bopt, "_multistart_map", lambda *a, **kw: out.setdefault("r", real(*a, **kw)))
    optimizemodel_(MAPGPOptimizer(every=1, objective="loo", restarts=4, seed=1, maxeval=40, **BOUNDS), m)
    val, best, per = out["r"]
    print("calls", seen, "four starts end at", per)
    assert seen.get("loo_grad_batch", 0) > 0 and "loo_grad" not in seen
    assert per.shape == (4,) and val == per.max() and val >= start
    np.testing.assert_array_equal(params_of(m), best)
    assert m.loo().total == pytest.approx(val, rel=1e-9)
    m.close()


def test_multistart_fit_beyond_the_size_cap_loops(bohip, monkeypatch):
    from bohip.bopt import MAPGPOptimizer, optimizemodel_

    X, y, _ = synth(513, 2, 1, seed=3)
    m = model_of(bohip, "SEArd", X, y, theta("SEArd", 2))
    start = m.loo().total
    seen = {}
    spy_on(monkeypatch, bohip.ElasticGPE, "loo_grad_batch", seen)
    spy_on(monkeypatch, bohip.ElasticGPE, "loo_grad", seen)
    optimizemodel_(MAPGPOptimizer(every=1, objective="loo", restarts=2, seed=0, maxeval=2, **BOUNDS), m)
    assert "loo_grad_batch" not in seen and seen.get("loo_grad", 0) >= 2
    assert math.isfinite(m.loo().total) and m.loo().total >= start
    m.close()


# ---- 6. a device list of one ------------------------------------------------------------------------------------------------------------
def test_multigpe_gives_the_single_device_bits(bohip):
    X, y, _ = synth(129, 3, 1, seed=6)
    Theta = settings("Mat12Ard", 3, 3, seed=4)
    t = Theta[0]
    m = model_of(bohip, "Mat12Ard", X, y, t)
    mg = bohip.MultiGPE(3, devices=[0], mean=bohip.MeanConst(t[1]), kernel=bohip.Mat12Ard(t[2:-1], t[-1]), logNoise=t[0], capacity=129)
    mg.append_(X.T, y)
    a, b = m.loo_grad_batch(Theta, want_logp=True), mg.loo_grad_batch(Theta, want_logp=True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    assert mg.loo_grad_batch(Theta, want_grad=False)[0].tobytes() == a[0].tobytes()
    m.close()
    mg.close()
