"""Posterior sample paths on the device (bohip_paths: ElasticGPE.draw_paths, PosteriorPaths.eval / eval_grad / coef, the "pathwise"
options of acquire_max and acquire_thompson_batch).

Reference: tests/path_reference.py -- Omega, w, eps rebuilt from the documented generator keys, K and k* from
tests/matern_reference.py, LAPACK solves.  Every tolerance is a derived bound, eps = 2^-52; each check prints the worst observed
fraction of its bound:
  Omega, w         elementwise what two correct evaluations of the generator's formula may differ by (path_reference.normal_tol,
                   frequencies_tol)
  u_s              backward error: |K u - rhs| <= 64 N eps (|K||u| + |rhs|) + the bound of the device's own Phi(X) w sum + the
                   tolerance of eps_s; rhs = y - beta - Phi(X) w_s - eps_s built from the DEVICE's Omega and w
  interpolation    |f_s(X_i) + eps_si + n u_si - y_i| <= the same residual bound + the value bound at X_i (device values only)
  values           |f - twin(device Omega, w, u)| <= 2 ((N + M + 8) eps (sum |u_j k_j| + sum |w_m phi_m|) + d eps amp sum_m |omega_m . x| (|w_2m| + |w_2m+1|))
  gradients        the same bound on the gradient's sums (path_reference.grad_bound); and against central differences of eval
                   with the rounding term (bound(x + h) + bound(x - h)) / 2h and the truncation term h^2 / 6 times a bound on the
                   third derivative (fd_third_bound)
  arg-max          bit for bit the first maximum of the returned values
"""
import math
import os
import warnings

import numpy as np
import pytest

import matern_reference as mr
import path_reference as pr
from conftest import synth
from joint_reference import first_argmax_rows
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LSIG, LNOISE, BETA = 0.2, -1.0, 0.1
EPS = pr.EPS
# kernel -> (N, d, log length-scales, M, [(S, R), ...]); every N in {5, 129, 600}, R in {1, 129, 1500}, S in {1, 3, 64, 200} and
# M in {16, 2048} appears; S < 24 takes the row form, S >= 24 the MFMA form (R = 70000 has its own test)
CASES = {
    "SEArd": (600, 4, np.array([-0.4, -0.2, 0.0, -0.6]), 2048, [(1, 1), (3, 129), (64, 1500), (200, 129)]),
    "Mat52Ard": (129, 10, np.full(10, 0.3), 2048, [(3, 1500), (64, 129), (200, 1)]),
    "Mat32Ard": (5, 2, np.array([-0.4, -0.1]), 16, [(1, 129), (64, 1)]),
    "Mat12Ard": (129, 4, np.full(4, -0.4), 16, [(3, 1), (200, 1500)]),
    "SEIso": (600, 8, np.array([0.2]), 2048, [(1, 1500), (64, 129)]),
}


def build(bohip, kern, X, y, ll, lnoise=LNOISE, beta=BETA, lsig=LSIG):
    m = bohip.ElasticGPE(X.shape[1], mean=bohip.MeanConst(beta), kernel=getattr(bohip, kern)(ll, lsig), logNoise=lnoise, capacity=len(y))
    m.append_(X.T, y)
    return m


def device_twin(kern, X, y, ll, M, seed, om):
    """The twin with the DEVICE's frequencies (the twin's own are compared with them separately)."""
    tw = pr.PathTwin(kern, X, y, ll, LSIG, LNOISE, BETA, M, seed)
    tw.Om_twin = tw.Om
    tw.Om = om
    tw.PhiX = pr.features(om, X, tw.s2f)
    return tw


def feature_sum_bound(tw, xs, w):
    """the part of value_bound that belongs to the feature sum alone"""
    return tw.value_bound(xs, np.zeros(tw.N), w)


def fd_third_bound(tw, xs, u, w):
    """R x d bound on |d^3 f / dx_k^3| along every axis.  Features: amp (|w_2m| + |w_2m+1|) |omega_mk|^3.  Kernel term g(rho(x)):
    |d^3/dx_k^3| <= il2_k^(3/2) (|g'''| + 3 |g''| / rho + 3 |g'| / rho^2), and |g'|, |g''|, |g'''| <= 12 s2f for all four families
    (a^3 <= 5 sqrt 5 < 12 for the exponent's rate a)."""
    il2 = mr.il2_of(tw.kern, tw.ll, tw.d)
    diff = xs[:, None, :] - tw.X[None, :, :]
    rho = np.sqrt(np.einsum("rnk,k->rn", diff * diff, il2))
    g3 = 12.0 * tw.s2f * (1.0 + 3.0 / rho + 3.0 / rho ** 2)
    amp = math.sqrt(tw.s2f / (tw.M // 2))
    wpair = np.abs(w[0::2]) + np.abs(w[1::2])
    return (g3 @ np.abs(u))[:, None] * il2[None, :] ** 1.5 + amp * (wpair @ np.abs(tw.Om) ** 3)[None, :]


@pytest.mark.parametrize("kern", list(CASES))
def test_coefficients_values_gradients_argmax(bohip, kern):
    N, d, ll, M, shapes = CASES[kern]
    X, y, _ = synth(N, d, 1, seed=17)
    seed = 12345
    m = build(bohip, kern, X, y, ll)
    rng = np.random.default_rng(3)
    worst = {}

    def note(name, frac):
        worst[name] = max(worst.get(name, 0.0), float(np.max(frac)))

    tw = None
    om0 = None
    for S, R in shapes:
        xs = rng.random((R, d))
        with m.draw_paths(S, M, seed) as p:
            assert (p.S, p.M, p.N, p.dim) == (S, M, N, d)
            vals, bv, bi = p.eval(xs.T)
            assert vals.shape == (S, R)
            # arg-max records: the first maximum of the returned values, and the same without values
            rv, ri = first_argmax_rows(vals)
            np.testing.assert_array_equal(bi, ri)
            np.testing.assert_array_equal(bv, rv)
            none, bv2, bi2 = p.eval(xs.T, want_values=False)
            assert none is None
            np.testing.assert_array_equal(bi2, bi)
            np.testing.assert_array_equal(bv2, bv)
            for s in sorted({0, S - 1, S // 2}):
                om, w, u = p.coef(s)
                if om0 is None:
                    om0 = om
                    tw = device_twin(kern, X, y, ll, M, seed, om)
                    tol = pr.frequencies_tol(kern, ll, d, M // 2, seed)
                    note("omega", np.abs(om - tw.Om_twin) / tol)
                np.testing.assert_array_equal(om, om0)                       # the basis is the same for any S and any path
                wt = tw.w(s)
                note("w", np.abs(w - wt) / pr.normal_tol(wt))
                # backward error of K u = rhs
                ze = pr.noise_normals(seed, s, M, N)
                rhs = (y - BETA) - tw.PhiX @ w - math.sqrt(tw.diag) * ze
                solve_b = (64 * N * EPS * (np.abs(tw.K) @ np.abs(u) + np.abs(rhs)) + feature_sum_bound(tw, X, w)
                           + math.sqrt(tw.diag) * pr.normal_tol(ze))
                note("K u = rhs", np.abs(tw.K @ u - rhs) / solve_b)
                # values against the twin with the device's coefficients
                note("values", np.abs(vals[s] - tw.value(xs, u, w)) / tw.value_bound(xs, u, w))
                # interpolation identity, device values only
                fX = p.eval(X.T)[0][s]
                note("interpolation", np.abs(fX + math.sqrt(tw.diag) * ze + tw.diag * u - y) / (solve_b + tw.value_bound(X, u, w)))
                # gradients: at most 40 points, on path s
                pts = xs[:40]
                f, g = p.eval_grad(pts.T, np.full(len(pts), s))
                note("grad values", np.abs(f - tw.value(pts, u, w)) / tw.value_bound(pts, u, w))
                note("gradients", np.abs(g.T - tw.grad(pts, u, w)) / tw.grad_bound(pts, u, w))
                h = 1e-5
                t3 = fd_third_bound(tw, pts, u, w)
                for k in range(d):
                    e = np.zeros(d); e[k] = h
                    fp, fm = p.eval((pts + e).T)[0][s], p.eval((pts - e).T)[0][s]
                    fd_b = (tw.value_bound(pts + e, u, w) + tw.value_bound(pts - e, u, w)) / (2 * h) + h * h / 6.0 * t3[:, k] \
                        + 4 * EPS * np.abs(g[k])
                    note("central differences", np.abs(g[k] - (fp - fm) / (2 * h)) / fd_b)
            # path_of: every point on its own path equals the rows of eval_grad taken path by path
            po = np.arange(min(R, 40)) % S
            f, g = p.eval_grad(xs[:len(po)].T, po)
            for s in set(po.tolist()):
                f1, g1 = p.eval_grad(xs[:len(po)].T, np.full(len(po), s))
                np.testing.assert_array_equal(f[po == s], f1[po == s])
                np.testing.assert_array_equal(g[:, po == s], g1[:, po == s])
            if S > 0:
                f0, g0 = p.eval_grad(xs[:len(po)].T)                          # None = path 0
                f1, g1 = p.eval_grad(xs[:len(po)].T, np.zeros(len(po), dtype=np.int64))
                np.testing.assert_array_equal(f0, f1)
                np.testing.assert_array_equal(g0, g1)
    print(f"{kern} N={N} d={d} M={M}: worst fraction of each bound: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
    m.close()


@pytest.mark.parametrize("S", [3, 64])
def test_seventy_thousand_candidates(bohip, S):
    """R = 70000 is beyond the joint draw's chunk and beyond one launch of the evaluation; records without values equal the records
    with values, and two calls of half the set agree with one call after the index offset.  S = 3: row form, S = 64: MFMA form."""
    N, d, R = 129, 4, 70000
    X, y, _ = synth(N, d, 1, seed=5)
    m = build(bohip, "Mat52Ard", X, y, np.full(d, -0.4))
    xs = np.random.default_rng(9).random((d, R))
    with m.draw_paths(S, 2048, 77) as p:
        none, bv, bi = p.eval(xs, want_values=False)
        assert none is None
        vals, bv1, bi1 = p.eval(xs)
        np.testing.assert_array_equal(bi, bi1)
        np.testing.assert_array_equal(bv, bv1)
        rv, ri = first_argmax_rows(vals)
        np.testing.assert_array_equal(bi, ri)
        np.testing.assert_array_equal(bv, rv)
        h = R // 2
        _, va, ia = p.eval(xs[:, :h], want_values=False)
        _, vb, ib = p.eval(xs[:, h:], want_values=False)
        take_b = (vb > va)                                                   # strict: on a tie the first half (smaller index) wins
        np.testing.assert_array_equal(np.where(take_b, ib + h, ia), bi)
        np.testing.assert_array_equal(np.where(take_b, vb, va), bv)
        # a value does not depend on what else was in the call
        sub = p.eval(xs[:, 1000:1129])[0]
        np.testing.assert_array_equal(sub, vals[:, 1000:1129])
    m.close()


def test_keying(bohip, monkeypatch):
    """Fewer paths are the leading paths of more, bit for bit (coefficients always; values within one form, selected through
    BOHIP_PATH_MFMA_MIN, which is read at every draw); another seed changes every path; the basis does not depend on S."""
    N, d = 129, 3
    X, y, Xs = synth(N, d, 300, seed=2)
    m = build(bohip, "Mat32Ard", X, y, np.full(d, -0.3))
    for form_min in ("1", "100000"):                                         # everything MFMA, everything row form
        monkeypatch.setenv("BOHIP_PATH_MFMA_MIN", form_min)
        with m.draw_paths(3, 64, 5) as a, m.draw_paths(64, 64, 5) as b, m.draw_paths(64, 64, 6) as c:
            va, vb, vc = a.eval(Xs.T)[0], b.eval(Xs.T)[0], c.eval(Xs.T)[0]
            np.testing.assert_array_equal(va, vb[:3])
            for s in range(3):
                for x, z in zip(a.coef(s), b.coef(s)):
                    np.testing.assert_array_equal(x, z)
            assert np.all(np.any(vb != vc, axis=1))                          # every path moved with the seed
            assert np.all(a.coef(0)[0] != c.coef(0)[0])
            ga, gb = a.eval_grad(Xs[:20].T, np.arange(20) % 3), b.eval_grad(Xs[:20].T, np.arange(20) % 3)
            np.testing.assert_array_equal(ga[0], gb[0])
            np.testing.assert_array_equal(ga[1], gb[1])
    monkeypatch.delenv("BOHIP_PATH_MFMA_MIN")
    # the two forms agree to rounding (value bound), not bit for bit
    monkeypatch.setenv("BOHIP_PATH_MFMA_MIN", "1")
    with m.draw_paths(3, 64, 5) as a:
        v_mfma = a.eval(Xs.T)[0]
        coefs = [a.coef(s) for s in range(3)]
    monkeypatch.setenv("BOHIP_PATH_MFMA_MIN", "100000")
    with m.draw_paths(3, 64, 5) as a:
        v_rows = a.eval(Xs.T)[0]
        for s in range(3):
            for x, z in zip(a.coef(s), coefs[s]):
                np.testing.assert_array_equal(x, z)                          # the coefficients never depend on the form
    tw = device_twin("Mat32Ard", X, y, np.full(d, -0.3), 64, 5, coefs[0][0])
    for s in range(3):
        assert np.all(np.abs(v_mfma[s] - v_rows[s]) <= tw.value_bound(Xs, coefs[s][2], coefs[s][1]))
    m.close()


def test_self_contained_and_model_untouched(bohip):
    from bohip import _lib

    N, d = 300, 4
    X, y, Xs = synth(N, d, 400, seed=2)
    ll = np.full(d, -0.4)
    m = build(bohip, "SEArd", X, y, ll)
    m.fit_()

    def state():
        return m.factor(), m.alpha(), m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS), m.info(_lib.INFO_CHOL_FORM), m.score("EI", [float(y.max())], Xs.T)

    before = state()
    p = m.draw_paths(5, 256, 3)
    q = m.draw_paths(70, 256, 4)
    after = state()
    for a, b in zip(before[:2], after[:2]):
        np.testing.assert_array_equal(a, b)
    assert before[2:5] == after[2:5]
    np.testing.assert_array_equal(before[5][0], after[5][0])
    assert before[5][1:] == after[5][1:]
    v0, g0, w0 = p.eval(Xs.T), p.eval_grad(Xs[:30].T, np.arange(30) % 5), q.eval(Xs.T)
    X2, y2, _ = synth(40, d, 1, seed=8)
    m.append_(X2.T, y2)
    m.set_params_(ll=np.full(d, 0.1), lsigma=0.5, logNoise=-2.0, beta=1.0)
    m.fit_()
    v1, g1, w1 = p.eval(Xs.T), p.eval_grad(Xs[:30].T, np.arange(30) % 5), q.eval(Xs.T)
    for a, b in zip(v0 + g0 + w0, v1 + g1 + w1):
        np.testing.assert_array_equal(a, b)
    assert (p.N, q.N) == (N, N)
    with m.draw_paths(1, 256, 3) as r:                                        # a new draw sees the new model
        assert r.N == N + 40
    p.close(); q.close(); m.close()


def test_moments(bohip):
    """ONE draw of S = 4000 paths at 8 points.  Given the device's Omega the paths are exactly Gaussian with mean mu and covariance
    G G' + n A'A (path_reference.conditional_moments), so no random-feature slack enters; limits of test_moments_of_one_call:
    5 standard errors, 0.15 relative."""
    X, y, Xs = synth(120, 2, 8, seed=4)
    ll = np.array([-0.5, -0.5])
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(BETA), kernel=bohip.SEArd(ll, LSIG), logNoise=LNOISE, capacity=120)
    m.append_(X.T, y)
    S, M = 4000, 2048
    with m.draw_paths(S, M, 0) as p:
        draws = p.eval(Xs.T)[0]
        om = p.coef(0)[0]
    tw = device_twin("SEArd", X, y, ll, M, 0, om)
    mu, cov = pr.conditional_moments(tw, Xs)
    sd = np.sqrt(np.diag(cov))
    dm = np.abs(draws.mean(0) - mu) / (sd / math.sqrt(S))
    dc = np.abs(np.cov(draws.T) - cov) / np.outer(sd, sd)
    print(f"moments: worst mean deviation {dm.max():.2f} standard errors (limit 5), worst covariance deviation {dc.max():.4f} (limit 0.15)")
    assert np.all(np.abs(draws.mean(0) - mu) <= 5 * sd / math.sqrt(S))
    assert np.all(np.abs(np.cov(draws.T) - cov) <= 0.15 * np.outer(sd, sd) + 1e-12)
    m.close()


def test_errors(bohip):
    from bohip import _lib

    N, d = 50, 3
    X, y, Xs = synth(N, d, 20, seed=1)
    m = build(bohip, "SEArd", X, y, np.full(d, -0.4))
    for S, M in ((0, 16), (-1, 16), (1, 0), (1, 1), (1, 2), (1, 17), (1, 24), (1, -16)):
        with pytest.raises(_lib.BohipError) as e:
            m.draw_paths(S, M, 0)
        assert e.value.code == _lib.E_ARG, (S, M)
    with pytest.raises(_lib.BohipError, match=str(_lib.PATHS_S_MAX)) as e:
        m.draw_paths(_lib.PATHS_S_MAX + 1, 16, 0)
    assert e.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.BohipError, match=str(_lib.PATHS_M_MAX)) as e:
        m.draw_paths(1, _lib.PATHS_M_MAX + 16, 0)
    assert e.value.code == _lib.E_UNSUPPORTED
    empty = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, -0.4), 0.0), logNoise=-1.0, capacity=8)
    with pytest.raises(_lib.BohipError) as e:
        empty.draw_paths(1, 16, 0)
    assert e.value.code == _lib.E_STATE
    lib = _lib.load()
    import ctypes as C
    out = C.c_void_p(1)
    assert lib.bohip_gp_paths_draw(None, 1, 16, 0, C.byref(out)) == _lib.E_ARG and not out.value    # null handles never crash
    assert lib.bohip_gp_paths_draw(None, 1, 16, 0, None) == _lib.E_ARG
    lib.bohip_paths_destroy(None)
    assert lib.bohip_paths_dims(None, None, None, None, None) == _lib.E_ARG
    assert lib.bohip_paths_eval(None, None, 1, None, None) == _lib.E_ARG
    assert lib.bohip_paths_eval_grad(None, None, 1, None, None, None) == _lib.E_ARG
    assert lib.bohip_paths_coef(None, 0, None, None, None) == _lib.E_ARG
    p = m.draw_paths(2, 16, 0)
    with pytest.raises(_lib.BohipError) as e:
        p.eval(np.zeros((d, 0), order="F"))
    assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.BohipError) as e:
        p.eval_grad(np.zeros((d, 0), order="F"))
    assert e.value.code == _lib.E_ARG
    for bad in ([2, 0], [0, -1]):
        with pytest.raises(_lib.BohipError) as e:
            p.eval_grad(Xs[:2].T, bad)
        assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.BohipError) as e:
        p.coef(2)
    assert e.value.code == _lib.E_ARG
    assert p.eval(Xs.T)[0].shape == (2, 20)                                   # the object works on
    p.close(); p.close()                                                      # idempotent
    for call in (lambda: p.eval(Xs.T), lambda: p.eval_grad(Xs.T), lambda: p.coef(0)):
        with pytest.raises(_lib.BohipError) as e:
            call()
        assert e.value.code == _lib.E_STATE
    # the largest sizes the issue names, at a small N: S = 1024 paths and M = 8192 features
    with m.draw_paths(1024, 8192, 1) as big:
        v, bv, bi = big.eval(Xs.T)
        assert v.shape == (1024, 20) and np.all(np.isfinite(v)) and np.all(bi >= 0)
    m.close(); empty.close()


def test_multigpe_draws_on_the_first_replica(bohip):
    X, y, Xs = synth(200, 3, 140, seed=8)
    ll = np.full(3, -0.4)
    one = build(bohip, "SEArd", X, y, ll)
    mg = bohip.MultiGPE(3, mean=bohip.MeanConst(BETA), kernel=bohip.SEArd(ll, LSIG), logNoise=LNOISE, capacity=200, devices=[0])
    mg.append_(X.T, y)
    with one.draw_paths(5, 64, 4) as a, mg.draw_paths(5, 64, 4) as b:
        np.testing.assert_array_equal(a.eval(Xs.T)[0], b.eval(Xs.T)[0])
    one.close(); mg.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_acquire_max_pathwise_direct_beats_a_latin_hypercube(bohip):
    """acquire_max(ThompsonSamplingSimple, GN_DIRECT_L, pathwise) searches ONE path; the value it returns is that path's value at
    the returned point and is at least the best of 2000 Latin-hypercube points on the same path."""
    from bohip.utils import latin_hypercube_sampling

    X, y, _ = synth(150, 2, 1, seed=3)
    m = build(bohip, "Mat52Ard", X, y, np.full(2, -0.4))
    lb, ub = np.zeros(2), np.ones(2)
    opts = {"method": "GN_DIRECT_L", "restarts": 1, "maxeval": 2000, "pathwise": True, "features": 1024}
    f, x = bohip.acquire_max(bohip.ThompsonSamplingSimple(), m, lb, ub, opts, rng=np.random.default_rng(11))
    seed = int(np.random.default_rng(11).integers(0, 2 ** 63 - 1))           # replay: the call's first number from rng is the seed
    with m.draw_paths(1, 1024, seed) as p:
        assert p.eval(x.reshape(-1, 1))[0][0, 0] == f
        lhs = latin_hypercube_sampling(lb, ub, 2000, np.random.default_rng(5))
        best = p.eval(lhs, want_values=False)[1][0]
    print(f"pathwise DIRECT-L: {f:.6f} at {x}, best of 2000 Latin-hypercube points on the same path {best:.6f}")
    assert f >= best and np.all((x >= lb) & (x <= ub))
    # LD_LBFGS: candidates, then the ascent on the path's gradient
    opts = {"method": "LD_LBFGS", "restarts": 3, "maxeval": 200, "pathwise": True, "features": 1024}
    f2, x2 = bohip.acquire_max(bohip.ThompsonSamplingSimple(), m, lb, ub, opts, rng=np.random.default_rng(12))
    assert np.isfinite(f2) and np.all((x2 >= lb) & (x2 <= ub))
    m.close()


def test_thompson_batch_pathwise(bohip):
    N, d, q = 300, 4, 6
    X, y, _ = synth(N, d, 1, seed=31)
    m = build(bohip, "Mat52Ard", X, y, np.full(d, -0.4))
    lb, ub = np.zeros(d), np.ones(d)
    xs = np.asfortranarray(np.random.default_rng(2).random((d, 70000)))       # more candidates than one joint-draw chunk
    v0, X0 = bohip.acquire_thompson_batch(m, lb, ub, q, {"xs": xs, "pathwise": True, "refine": False}, rng=np.random.default_rng(1))
    v1, X1 = bohip.acquire_thompson_batch(m, lb, ub, q, {"xs": xs, "pathwise": True}, rng=np.random.default_rng(1))
    assert X0.shape == (d, q) and X1.shape == (d, q)
    cols = [int(np.flatnonzero(np.all(xs == X0[:, [j]], axis=0))[0]) for j in range(q)]
    assert len(set(cols)) == q                                                # distinct candidates
    assert len({tuple(c) for c in X1.T}) == q and np.all((X1 >= lb[:, None]) & (X1 <= ub[:, None]))
    print("refined - pick:", (v1 - v0).tolist())
    assert np.all(v1 >= v0)
    seed = int(np.random.default_rng(1).integers(0, 2 ** 63 - 1))
    with m.draw_paths(q, 2048, seed) as p:                                    # the values are the paths' own values at the points
        f, _ = p.eval_grad(X1, np.arange(q))
        up = v1 > v0
        np.testing.assert_array_equal(f[up], v1[up])                          # a refined point carries the ascent's own value ...
        np.testing.assert_array_equal(X1[:, ~up], X0[:, ~up])                 # ... and a pick that was not improved stays
        np.testing.assert_array_equal(v1[~up], v0[~up])
    m.close()


def test_branin_thompson_batches_pathwise(bohip):
    """test_branin_thompson_batches with the pathwise option: every iteration appends 4 distinct points."""
    from test_bo_loop_gpu import make_opt

    bo = bohip
    model = bo.ElasticGPE(2, mean=bo.MeanConst(-10.0), kernel=bo.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=200)
    batches = 5
    opt = make_opt(bo, model, bo.ThompsonSamplingSimple(), maxiterations=10 + batches, batchsize=4,
                   batchoptions={"candidates": 512, "pathwise": True})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bo.boptimize_(opt)
    assert len(model.y) == 10 + 4 * batches
    for b in range(batches):
        cols = model.x[:, 10 + 4 * b: 14 + 4 * b]
        assert len({tuple(c) for c in cols.T}) == 4
    model.close()
