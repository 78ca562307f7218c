"""Leave-one-out cross-validation on the device (include/bohip_loo.h) against the NumPy twin (tests/loo_reference.py).

Shapes (N, d): (1, 1), (2, 2), (17, 3), (129, 8), (257, 17) -- across a 128-tile edge and the 256-column block of the parts kernel,
dimension buckets 2, 4, 8 and 32 -- every kernel id and every shape at least twice, both means; the stress setting (lsigma = 5,
logNoise = 0) at (129, 2); N = 1100 for nine row tiles and several GEMM tiles.
Tolerances are the project's for these quantities (test_mll_gradient_vs_oracle): values, total and per point, 1e-9 of the largest
magnitude; gradient rtol 1e-6 with the floor 1e-8 max|g_ref|.  mu_-i = y_i - alpha_i / kappa_i is a difference formed at the size
of y, so its largest magnitude is taken over mu and y together (one observation under MeanZero has mu = 0 exactly)."""
import ctypes as C
import math

import numpy as np
import pytest

import loo_reference as lr
from conftest import synth
from matern_reference import KERNELS
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ALL = list(KERNELS)
SHAPES = {(1, 1): ["SEArd", "Mat12Iso", "Mat52Iso"], (2, 2): ["SEIso", "Mat32Ard", "Mat12Ard"],
          (17, 3): ["Mat52Ard", "Mat12Ard", "Mat32Iso", "SEIso"], (129, 8): ALL,
          (257, 17): ["SEArd", "Mat52Ard", "Mat32Ard", "Mat12Iso", "Mat52Iso", "Mat32Iso"]}
CASES = [(k, N, d) for (N, d), ks in SHAPES.items() for k in ks]
BASELINE = (math.log(0.5), 0.0, -2.0)     # ll, lsigma, logNoise
STRESS = (math.log(0.5), 5.0, 0.0)
BETA = 0.3


def theta(kern, d, setting=BASELINE, beta=BETA):
    return lr.theta_of(kern, d, setting[0], setting[1], setting[2], beta)


def model_of(bohip, kern, X, y, t, mean_const=True, capacity=None):
    mean = bohip.MeanConst(t[1]) if mean_const else bohip.MeanZero()
    m = bohip.ElasticGPE(X.shape[1], mean=mean, kernel=getattr(bohip, kern)(t[2:-1], t[-1]), logNoise=t[0], capacity=capacity or max(len(y), 1))
    m.append_(X.T, y)
    return m


def check_values(res, ref, y, what):
    mu, var, logp, total = ref
    for got, want, name, scale in ((res.mu, mu, "mu", max(np.abs(mu).max(), np.abs(y).max())), (res.var, var, "var", np.abs(var).max()),
                                   (res.logp, logp, "logp", np.abs(logp).max())):
        err = np.abs(got - want).max()
        print(f"{what}: {name} max err {err:.3e} / scale {scale:.3e} = {err / scale:.2e}")
        assert err <= 1e-9 * scale, (what, name)
    print(f"{what}: total {res.total:.12g} (ref {total:.12g}, rel {abs(res.total - total) / abs(total):.2e})")
    assert abs(res.total - total) <= 1e-9 * abs(total), what
    np.testing.assert_array_equal(res.z, (y - res.mu) / np.sqrt(res.var))


def check_grad(got, ref, what):
    tot, dn, dm, dk = got
    g = np.concatenate([[dn, dm], dk])
    tot_ref, g_ref = ref
    print(f"{what}: total rel {abs(tot - tot_ref) / abs(tot_ref):.2e}, max |dg| / max|g_ref| {np.abs(g - g_ref).max() / np.abs(g_ref).max():.2e}")
    assert abs(tot - tot_ref) <= 1e-9 * abs(tot_ref), what
    np.testing.assert_allclose(g, g_ref, rtol=1e-6, atol=1e-8 * np.abs(g_ref).max(), err_msg=what)


def check_model(m, kern, X, y, t, what):
    check_values(m.loo(), lr.loo_fast(kern, X, y, t[2:-1], t[-1], t[0], t[1]), y, what)
    check_grad(m.loo_grad(), lr.grad_vec(kern, X, y, t), what)


# ---- 1. parity over shapes, kernels, means --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d", CASES)
def test_values_and_gradient_match_the_twin(bohip, kern, N, d):
    X, y, _ = synth(N, d, 1, seed=300 + N)
    for mean_const in (True, False):
        t = theta(kern, d, beta=BETA if mean_const else 0.0)
        m = model_of(bohip, kern, X, y, t, mean_const)
        check_model(m, kern, X, y, t, f"{kern} N={N} d={d} {'MeanConst' if mean_const else 'MeanZero'}")
        m.close()


@pytest.mark.parametrize("kern", ["SEArd", "Mat52Ard"])
def test_stress_setting(bohip, kern):
    X, y, _ = synth(129, 2, 1, seed=11)
    t = theta(kern, 2, STRESS)
    check_model(model_of(bohip, kern, X, y, t), kern, X, y, t, f"{kern} stress (129, 2)")


def test_values_against_the_brute_force(bohip):
    X, y, _ = synth(17, 3, 1, seed=5)
    t = theta("Mat52Ard", 3)
    check_values(model_of(bohip, "Mat52Ard", X, y, t).loo(), lr.loo_brute("Mat52Ard", X, y, t[2:-1], t[-1], t[0], t[1]), y, "brute force (17, 3)")


def test_nine_row_tiles(bohip):
    X, y, _ = synth(1100, 8, 1, seed=21)
    t = theta("Mat52Ard", 8)
    check_model(model_of(bohip, "Mat52Ard", X, y, t), "Mat52Ard", X, y, t, "Mat52Ard N=1100 d=8")


# ---- 2. one total, the same bits ------------------------------------------------------------------------------------------------
def test_total_is_one_number_bit_for_bit(bohip):
    X, y, _ = synth(257, 3, 1, seed=2)
    m = model_of(bohip, "Mat32Ard", X, y, theta("Mat32Ard", 3))
    a, ga = m.loo(), m.loo_grad()
    b, gb = m.loo(), m.loo_grad()
    assert np.float64(a.total).tobytes() == np.float64(ga[0]).tobytes() == np.float64(b.total).tobytes() == np.float64(gb[0]).tobytes()
    for u, v in ((a.mu, b.mu), (a.var, b.var), (a.logp, b.logp), (ga[3], gb[3])):
        assert u.tobytes() == v.tobytes()
    assert ga[1:3] == gb[1:3]


# ---- 3. handles that have lived -------------------------------------------------------------------------------------------------
def test_a_grown_handle_agrees_with_a_fresh_one(bohip):
    X, y, _ = synth(131, 8, 1, seed=9)
    t = theta("SEArd", 8)
    grown = model_of(bohip, "SEArd", X[:126], y[:126], t, capacity=256)
    for i in range(126, 131):
        grown.append_(X[i:i + 1].T, y[i:i + 1])                    # across the 128-tile edge, no refit
    assert grown.info(3) == 5                                      # five incremental appends
    fresh = model_of(bohip, "SEArd", X, y, t)
    a, b = grown.loo(), fresh.loo()
    check_values(a, (b.mu, b.var, b.logp, b.total), y, "grown against fresh")
    gb = fresh.loo_grad()
    check_grad(grown.loo_grad(), (gb[0], np.concatenate([[gb[1], gb[2]], gb[3]])), "grown against fresh")
    check_model(grown, "SEArd", X, y, t, "grown against the twin")


def test_a_stale_handle_answers_at_the_new_parameters(bohip):
    X, y, _ = synth(65, 3, 1, seed=4)
    m = model_of(bohip, "Mat52Iso", X, y, theta("Mat52Iso", 3))
    t = np.array([-1.2, -0.1, -0.3, 0.4])
    m.set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
    check_values(m.loo(), lr.loo_fast("Mat52Iso", X, y, t[2:-1], t[-1], t[0], t[1]), y, "stale, loo first")
    t2 = t + 0.2
    m.set_params_(ll=t2[2:-1], lsigma=t2[-1], logNoise=t2[0], beta=t2[1])
    check_grad(m.loo_grad(), lr.grad_vec("Mat52Iso", X, y, t2), "stale, loo_grad first")


def test_the_model_is_untouched(bohip):
    X, y, Xs = synth(140, 5, 64, seed=13)
    t = theta("Mat32Ard", 5)
    m = model_of(bohip, "Mat32Ard", X, y, t)
    Theta = np.vstack([t, t + 0.3])

    def state():
        mu, var = m.predict_f(Xs.T)
        sc, bv, bi = m.score("EI", [float(y.max())], Xs.T)
        g = m.mll_grad()
        mb = m.mll_grad_batch(Theta)
        return (mu.tobytes(), var.tobytes(), sc.tobytes(), bv, bi, g[:3], g[3].tobytes(), mb[0].tobytes(), mb[1].tobytes(), m.alpha().tobytes(),
                m.factor().tobytes(), m.info(2))

    before = state()
    m.loo()
    assert state() == before
    m.loo_grad()
    assert state() == before
    m.loo_grad()
    m.loo()
    assert state() == before


# ---- 4. errors and the empty model ----------------------------------------------------------------------------------------------
def test_errors_and_no_observations(bohip):
    from bohip import _lib

    dp = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    empty = bohip.ElasticGPE(2, mean=bohip.MeanZero(), kernel=bohip.SEIso(0.0, 0.0))
    arrs = [np.full(3, 7.0) for _ in range(3)]
    tot = np.full(1, 7.0)
    assert empty._lib.bohip_gp_loo(empty._h, p(arrs[0]), p(arrs[1]), p(arrs[2]), p(tot)) == _lib.OK
    assert tot[0] == 0.0 and all(np.all(a == 7.0) for a in arrs)
    r = empty.loo()
    assert r.total == 0.0 and r.mu.size == 0 and r.z.size == 0
    assert empty.loo_grad()[:3] == (0.0, 0.0, 0.0) and np.array_equal(empty.loo_grad()[3], np.zeros(2))
    X, y, _ = synth(5, 2, 1, seed=1)
    m = model_of(bohip, "SEArd", X, y, theta("SEArd", 2))
    assert m._lib.bohip_gp_loo(m._h, None, None, None, None) == _lib.E_ARG
    assert m._lib.bohip_gp_loo(m._h, None, None, None, p(tot)) == _lib.OK        # every per-point array may be left out
    assert tot[0] == m.loo().total
    only = np.empty(5)
    assert m._lib.bohip_gp_loo(m._h, None, p(only), None, p(tot)) == _lib.OK and only.tobytes() == m.loo().var.tobytes()
    g = [np.zeros(3) for _ in range(4)]
    for k in range(4):
        args = [p(a) for a in g]
        args[k] = None
        assert m._lib.bohip_gp_loo_grad(m._h, *args) == _lib.E_ARG
    # a factorisation that fails reports as it does from mll_grad, and the handle stays usable
    Xd, yd = np.zeros((40, 2)), np.arange(40.0)
    bad = model_of(bohip, "SEArd", Xd, yd, theta("SEArd", 2))
    fine = bad.loo().total
    bad.set_params_(lsigma=10.0, logNoise=-30.0)
    for call in (bad.mll_grad, bad.loo, bad.loo_grad):
        with pytest.raises(bohip.NotPositiveDefinite):
            call()
    t = theta("SEArd", 2)
    bad.set_params_(lsigma=t[-1], logNoise=t[0])
    assert bad.loo().total == pytest.approx(fine, rel=1e-12)


# ---- 5. the fit's objective -----------------------------------------------------------------------------------------------------
BOUNDS = dict(noisebounds=[-4, 2], meanbounds=[[-2], [2]], kernbounds=[[-3, -3, -3], [3, 3, 3]])


def fit_problem():
    """Forty noisy observations of a function the kernel does not describe well (a kink and a trend)."""
    rng = np.random.default_rng(8)
    X = rng.random((40, 2))
    y = np.abs(X[:, 0] - 0.4) * 3.0 + X[:, 1] ** 3 + 0.3 * rng.standard_normal(40) * X[:, 0]
    return X, y


def params_of(m):
    return np.concatenate([[m.logNoise, m.mean.beta], m.kernel.ll, [m.kernel.lsigma]])


def test_map_fit_with_the_loo_objective(bohip, monkeypatch):
    from bohip import bopt
    from bohip.bopt import MAPGPOptimizer, optimizemodel_

    X, y = fit_problem()
    t0 = theta("Mat52Ard", 2, beta=0.0)
    m = model_of(bohip, "Mat52Ard", X, y, t0)
    start = m.loo().total
    optimizemodel_(MAPGPOptimizer(every=1, objective="loo", **BOUNDS), m)
    end, t_loo = m.loo().total, params_of(m)
    print("LOO objective: start", start, "end", end, "at", t_loo)
    assert end >= start
    assert end == pytest.approx(lr.total_at("Mat52Ard", X, y, t_loo), rel=1e-9)
    ref = model_of(bohip, "Mat52Ard", X, y, t0)
    optimizemodel_(MAPGPOptimizer(every=1, **BOUNDS), ref)
    print("marginal likelihood's end point", params_of(ref), "its LOO", ref.loo().total)
    assert not np.allclose(params_of(ref), t_loo, rtol=1e-3, atol=1e-3)
    # restarts: the loop route, and the best of its ends wins
    seen = {}
    real = bopt._multistart_map

    def spy(*a, **kw):
        seen["out"] = real(*a, **kw)
        return seen["out"]

    monkeypatch.setattr(bopt, "_multistart_map", spy)
    multi = model_of(bohip, "Mat52Ard", X, y, t0)
    optimizemodel_(MAPGPOptimizer(every=1, objective="loo", restarts=3, seed=1, maxeval=40, **BOUNDS), multi)
    val, best, per = seen["out"]
    print("three starts end at", per)
    assert per.shape == (3,) and val == per.max() and val >= start
    np.testing.assert_array_equal(params_of(multi), best)
    assert multi.loo().total == pytest.approx(val, rel=1e-9)


# ---- 6. a device list of one ----------------------------------------------------------------------------------------------------
def test_multigpe_gives_the_single_device_bits(bohip):
    X, y, _ = synth(129, 3, 1, seed=6)
    t = theta("Mat12Ard", 3)
    m = model_of(bohip, "Mat12Ard", X, y, t)
    mg = bohip.MultiGPE(3, devices=[0], mean=bohip.MeanConst(t[1]), kernel=bohip.Mat12Ard(t[2:-1], t[-1]), logNoise=t[0], capacity=129)
    mg.append_(X.T, y)
    a, b = m.loo(), mg.loo()
    for u, v in ((a.mu, b.mu), (a.var, b.var), (a.logp, b.logp), (a.z, b.z)):
        assert u.tobytes() == v.tobytes()
    ga, gb = m.loo_grad(), mg.loo_grad()
    assert a.total == b.total == ga[0] == gb[0] and ga[1:3] == gb[1:3] and ga[3].tobytes() == gb[3].tobytes()
