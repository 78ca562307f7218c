"""Constrained optimisation on the device (include/bohip_con.h) against tests/con_reference.py.

Bounds.  predict_grad: mu 1e-6 |ref| + mu_floor, sigma^2 var_tol, the Jacobians test_matern_gpu's bound on a gradient (rtol 1e-6, atol
1e-9 max|g_ref| + 1e-12).  con_values: 16 x con_reference.WORST relative to max(1, |ref|) against the 50-digit evaluator (WORST is the
twin's own measured error; the device's libm differs from NumPy's in the last bits).  score_con: the first-order propagation of the
members' bounds through the twin's partials (con_reference.propagate)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import con_reference as cr
from conftest import synth
from matern_reference import KERNELS, MaternGP
from test_fit_gpu import centre, model_of
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ALL = list(KERNELS)
SHAPES = {(1, 1): ["SEArd", "Mat12Iso"], (2, 2): ["SEIso", "Mat32Ard"], (17, 3): ["Mat52Ard", "Mat12Ard", "Mat32Iso"], (65, 8): ALL,
          (200, 17): ["Mat52Iso", "Mat12Ard", "SEIso"], (64, 33): ["Mat32Ard", "Mat52Ard", "Mat12Iso"], (130, 64): ["SEArd", "Mat32Iso"]}
CASES = [(k, N, d) for (N, d), ks in SHAPES.items() for k in ks]


def twin_of(kern, X, y, t=None):
    t = centre(kern, X.shape[1]) if t is None else t
    return MaternGP(kern, X, y, t[2:-1], t[-1], t[0], t[1])


def check_predict_grad(res, ref, tw, what):
    """res = (mu, var, dmu[d, R], dvar[d, R]) of the device, tw = posterior_jac of the twin; prints the worst share of each bound."""
    mu, var, jm, jv = tw
    bm, bv = cr.moment_bounds(ref, mu, var)
    shares = [np.max(np.abs(res[0] - mu) / bm), np.max(np.abs(res[1] - var) / bv),
              np.max(np.abs(res[2].T - jm) / cr.jac_bound(jm)), np.max(np.abs(res[3].T - jv) / cr.jac_bound(jv))]
    print(f"{what}: worst share of the bound: mu {shares[0]:.3g}, var {shares[1]:.3g}, dmu {shares[2]:.3g}, dvar {shares[3]:.3g}")
    assert all(np.isfinite(s) and s <= 1.0 for s in shares), (what, shares)


# ---- 1. predict_grad ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d", CASES)
def test_predict_grad_against_the_twin(bohip, kern, N, d):
    X, y, Xs = synth(N, d, 300, seed=2000 + 7 * N + 3 * d)
    ref = twin_of(kern, X, y)
    m = model_of(bohip, kern, X, y)
    full = None
    for R in (1, 17, 300):
        res = m.predict_grad(Xs[:R].T)
        assert res[2].shape == (d, R) and res[3].shape == (d, R)
        check_predict_grad(res, ref, cr.posterior_jac(ref, Xs[:R]), f"{kern} N={N} d={d} R={R}")
        full = res
    mu, var = m.predict_f(Xs.T)                                                # bohip_gp_predict at R = 300 takes the same route (K*' chunks,
    assert full[0].tobytes() == mu.tobytes() and full[1].tobytes() == var.tobytes()   # the fused finish adds q in k_score's order): the same bits
    m.close()


@pytest.mark.parametrize("kern,N,d,R,what", [("Mat52Ard", 1000, 4, 40, "split-K"), ("SEArd", 1500, 5, 3, "split-K, few candidates"),
                                               ("Mat32Ard", 1600, 5, 3, "two observation splits")])
def test_predict_grad_on_the_other_routes(bohip, kern, N, d, R, what):
    """N = 1000, R = 40: eight row tiles and few candidate tiles take the split-K posterior.  N = 1500, R = 3: the same with k_post_grad_finish
    on a handful of candidates; k_grad_finish's rule splits the observations over min(16, N / 768) workgroups, which is ONE at
    1500, so N = 1600 is here as well: two splits and the last-arriver combine.  A second call sees the arrival counters back at zero."""
    X, y, Xs = synth(N, d, R, seed=77 + N)
    ref = twin_of(kern, X, y)
    m = model_of(bohip, kern, X, y)
    res = m.predict_grad(Xs.T)
    check_predict_grad(res, ref, cr.posterior_jac(ref, Xs), f"{what}: {kern} N={N} R={R}")
    again = m.predict_grad(Xs.T)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res, again))
    m.close()


def test_predict_grad_over_two_candidate_chunks(bohip):
    """R = 70001 at N = 200 is two K*' chunks inside the call (test_parity_gpu.test_candidate_chunking_is_invisible's shape): 400
    candidates across the boundary against the twin, and a call on that slice alone gives the slice's bytes."""
    from bohip import _lib

    X, y, Xs = synth(200, 3, 70001, seed=17)
    ref = twin_of("Mat52Ard", X, y)
    m = model_of(bohip, "Mat52Ard", X, y)
    res = m.predict_grad(Xs.T)
    ch = m.info(_lib.INFO_SCORE_CHUNK)
    assert 0 < ch < 70001
    lo, hi = ch - 192, ch + 208
    sub = tuple(a[..., lo:hi] for a in res)
    check_predict_grad(sub, ref, cr.posterior_jac(ref, Xs[lo:hi]), "two chunks, across the boundary")
    check_predict_grad(tuple(a[..., -300:] for a in res), ref, cr.posterior_jac(ref, Xs[-300:]), "two chunks, the tail")
    alone = m.predict_grad(Xs[lo:hi].T)
    assert all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(sub, alone))
    m.close()


# ---- 2. con_values on crafted moments ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted_ref(acq, C_, R):
    thr, s, mu, var = cr.crafted(C_, R, seed=7 * C_ + R)
    out = (thr, s, mu, var) + cr.mp_table(acq, [0.3], thr, s, mu, var)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def anchor(bohip):
    m = bohip.ElasticGPE(2)                                                     # no observations: the device and the stream only
    yield m
    m.close()


@pytest.mark.parametrize("R", [1, 257, 1000])
@pytest.mark.parametrize("C_", [0, 1, 5])
@pytest.mark.parametrize("acq", cr.FORMS)
def test_con_values_against_mpmath(bohip, anchor, acq, C_, R):
    thr, s, mu, var, fr, Lr, pmr, pvr = crafted_ref(acq, C_, R)
    f, L, pm, pv, bv, bi = anchor.con_values(acq, [0.3], thr, s, mu, var, want_grad=True)
    f2, L2, none_m, none_v, bv2, bi2 = anchor.con_values(acq, [0.3], thr, s, mu, var)
    assert none_m is None and none_v is None and f2.tobytes() == f.tobytes() and L2.tobytes() == L.tobytes() and (bv2, bi2) == (bv, bi)
    shares = {"value": cr.worst_share(f, fr, 16 * cr.WORST["value"]), "dmu": cr.worst_share(pm, pmr, 16 * cr.WORST["dmu"]),
              "dvar": cr.worst_share(pv, pvr, 16 * cr.WORST["dvar"])}
    ok = np.isfinite(Lr)
    shares["logfeas"] = cr.worst_share(L[ok], Lr[ok], 16 * cr.WORST["value"])
    print(f"{acq} C={C_} R={R}: worst share of 16 x WORST {shares}")
    assert max(shares.values()) <= 1.0, shares
    assert not np.any(np.isnan(pm[:, np.isfinite(f)])) and not np.any(np.isnan(pv[:, np.isfinite(f)]))
    assert (bv, bi) == cr.record(f)                                             # the record of the device's own values: first maximum,
    if bi >= 0:                                                                 # NaN never wins
        assert f[bi] == bv and not np.isnan(bv)
    tv, ti = cr.record(fr)                                                     # ... and the 50-digit winner, or its equal within the bound
    assert ti == bi or abs(f[ti] - f[bi]) <= 32 * cr.WORST["value"] * max(1.0, abs(tv))


def test_con_values_beyond_one_grid_stride(bohip, anchor):
    """R = 262144 + 257: more candidates than k_con_combine's grid holds threads, so every thread of the first 257 takes a second
    one.  Against the twin, within the device's bound plus the twin's own (17 x WORST); the record is that of the values."""
    R = 262144 + 257
    thr, s, mu, var = cr.crafted(2, R, seed=5)
    f, L, pm, pv, bv, bi = anchor.con_values("LogEI", [0.3], thr, s, mu, var, want_grad=True)
    fr, Lr, pmr, pvr = cr.combine("LogEI", [0.3], thr, s, mu, var)
    assert cr.worst_share(f, fr, 17 * cr.WORST["value"]) <= 1.0 and cr.worst_share(pm, pmr, 17 * cr.WORST["dmu"]) <= 1.0
    assert cr.worst_share(pv, pvr, 17 * cr.WORST["dvar"]) <= 1.0
    assert (bv, bi) == cr.record(f)
    late = f.copy()
    late[:262144] = -np.inf                                                     # a winner in the second stride
    mu2 = mu.copy()
    mu2[0, :262144] = np.nan
    f3, _, _, _, bv3, bi3 = anchor.con_values("LogEI", [0.3], thr, s, mu2, var)
    assert (bv3, bi3) == cr.record(f3) == cr.record(late) and bi3 >= 262144


# ---- 3. score_con end to end ------------------------------------------------------------------------------------------------------
D_E2E = 4
MEMBERS = (("Mat52Ard", 65), ("SEArd", 17), ("Mat12Iso", 130))                # the objective, then the two constraint models
# trials of the candidates' seed, chosen on the CPU from the twin alone so that its winner leads by > 4 x the two tolerances (lead_ok)
TRIAL = {}


@functools.lru_cache(maxsize=None)
def member_data():
    out = []
    for i, (kern, n) in enumerate(MEMBERS):
        X, y, _ = synth(n, D_E2E, 1, seed=300 + i)
        y = y - (0.0 if i == 0 else float(np.median(y)))
        out.append((kern, X, y, twin_of(kern, X, y)))
    return tuple(out)


def constraint_set(C_):
    """C constraints over the two constraint models in turn (a handle may serve several), senses alternating."""
    which = [1 + c % 2 for c in range(C_)]
    thr = [(-0.3, 0.25, 0.4, -0.5, 0.1)[c] for c in range(C_)]
    senses = [(1, -1, -1, 1, 1)[c] for c in range(C_)]
    return which, thr, senses


@functools.lru_cache(maxsize=None)
def e2e_twin(acq, C_, R):
    data = member_data()
    which, thr, senses = constraint_set(C_)
    t = TRIAL.get((acq, C_, R), 0)
    Xs = np.random.default_rng(900 + 31 * C_ + R + 10007 * t).random((R, D_E2E))
    models = [data[0][3]] + [data[w][3] for w in which]
    # tau: the median observation; PI saturates at 1 - 1e-13 over half the box there and has no clear winner, so PI takes the maximum
    tau = float(np.max(data[0][2])) if acq == "PI" else float(np.median(data[0][2]))
    tw = cr.score_con(models, acq, [tau], thr, senses, Xs)
    ts, tg = cr.propagate(models, acq, tw)
    for a in (Xs, ts, tg):
        a.setflags(write=False)
    return Xs, models, tau, tw, ts, tg


def lead_ok(tw, ts):
    """The twin's winner leads every other candidate by more than four times the sum of the two tolerances."""
    f, bi = tw["scores"], tw["best_idx"]
    if bi < 0 or f.size == 1:
        return True
    others = np.delete(np.arange(f.size), bi)
    with np.errstate(invalid="ignore"):
        gap = f[bi] - f[others]
    return bool(np.all(np.isnan(gap) | (gap > 4.0 * (ts[bi] + ts[others]))))


@pytest.fixture(scope="module")
def e2e_models(bohip):
    ms = [model_of(bohip, kern, X, y) for kern, X, y, _ in member_data()]
    yield ms
    for m in ms:
        m.close()


@pytest.mark.parametrize("R", [1, 17, 300])
@pytest.mark.parametrize("C_", [0, 1, 2, 5])
@pytest.mark.parametrize("acq", cr.FORMS)
def test_score_con_against_the_twin(bohip, e2e_models, acq, C_, R):
    Xs, models, tau, tw, ts, tg = e2e_twin(acq, C_, R)
    which, thr, senses = constraint_set(C_)
    cm = bohip.ConstrainedGPE(e2e_models[0], [e2e_models[w] for w in which], thr, senses)
    val = cm.score(acq, [tau], Xs.T)
    grd = cm.score(acq, [tau], Xs.T, want_grad=True)
    for a, b in ((val.scores, grd.scores), (val.logfeas, grd.logfeas), (val.mu, grd.mu), (val.var, grd.var)):
        assert a.tobytes() == b.tobytes()                                       # value call == gradient call, bit for bit
    assert (val.best_val, val.best_idx) == (grd.best_val, grd.best_idx) and val.grad is None and grd.grad.shape == (D_E2E, R)
    s_share = np.max(np.abs(val.scores - tw["scores"]) / ts)
    smooth = np.ones(R, dtype=bool)
    for m_, t_ in zip(range(len(models)), [tau] + list(thr)):
        if m_ == 0 and acq == "Feasibility":
            continue
        with np.errstate(all="ignore"):
            smooth &= (tw["var"][m_] > 0) & (np.abs(tw["mu"][m_] - t_) / np.sqrt(tw["var"][m_]) < 6.0)
    g_share = np.max(np.abs(grd.grad.T - tw["grad"])[smooth] / tg[smooth]) if smooth.any() else 0.0
    print(f"{acq} C={C_} R={R}: worst share of the bound: score {s_share:.3g}, gradient {g_share:.3g} on {int(smooth.sum())} smooth candidates")
    assert s_share <= 1.0 and g_share <= 1.0
    assert np.all(np.isfinite(grd.grad[:, np.isfinite(grd.scores)]))
    rows = slice(1, None) if acq == "Feasibility" else slice(None)
    for m_ in range(len(models))[rows]:
        bm, bv = cr.moment_bounds(models[m_], tw["mu"][m_], tw["var"][m_])
        assert np.all(np.abs(val.mu[m_] - tw["mu"][m_]) <= bm) and np.all(np.abs(val.var[m_] - tw["var"][m_]) <= bv)
    if acq == "Feasibility":
        assert np.all(np.isnan(val.mu[0])) and np.all(np.isnan(val.var[0]))
    # the arg-max is the twin's, with no exemption: the seed makes the twin's winner lead by more than 4 x the two tolerances
    constant = bool(np.all(tw["scores"] == tw["scores"][0]))                   # (C = 0 under "Feasibility": L = 0 everywhere, index 0 wins)
    assert constant or lead_ok(tw, ts), ("choose another trial for", acq, C_, R)
    assert val.best_idx == tw["best_idx"] and val.best_val == val.scores[val.best_idx]
    if C_ == 0 and acq != "Feasibility":                                         # C = 0 is bohip_gp_score's quantity
        sc, bv_, bi_ = e2e_models[0].score(acq, [tau], Xs.T)
        floor = cr.mu_floor(models[0].alpha, models[0].s2f)
        assert np.all(np.abs(val.scores - sc) <= 2 * (1e-6 * np.abs(sc) + floor + 1e-12)) and bi_ == val.best_idx
    if R > 1:                                                                    # two halves scored separately give the bytes of the whole
        h = R // 2
        a, b = cm.score(acq, [tau], Xs[:h].T, want_grad=True), cm.score(acq, [tau], Xs[h:].T, want_grad=True)
        assert np.concatenate([a.scores, b.scores]).tobytes() == grd.scores.tobytes()
        assert np.concatenate([a.grad, b.grad], axis=1).tobytes(order="F") == grd.grad.tobytes(order="F")


def test_feasibility_needs_no_objective_observations(bohip, e2e_models):
    empty = bohip.ElasticGPE(D_E2E)
    Xs = np.random.default_rng(1).random((D_E2E, 33))
    a = bohip.ConstrainedGPE(empty, [e2e_models[1]], [0.1], [1]).score("Feasibility", [], Xs, want_grad=True)
    b = bohip.ConstrainedGPE(e2e_models[0], [e2e_models[1]], [0.1], [1]).score("Feasibility", [], Xs, want_grad=True)
    assert a.scores.tobytes() == b.scores.tobytes() and a.grad.tobytes() == b.grad.tobytes() and a.best_idx == b.best_idx >= 0
    np.testing.assert_array_equal(a.scores, a.logfeas)
    empty.close()


# ---- 4. every error code ------------------------------------------------------------------------------------------------------------
def test_error_codes(bohip, e2e_models):
    from bohip import _lib

    lib = _lib.load()
    obj, c1 = e2e_models[0], e2e_models[1]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    R = 5
    xs = np.asfortranarray(np.random.default_rng(0).random((D_E2E, R)))
    out = np.empty(R)
    p = np.array([0.1, 0.0])
    ptr = lambda a: a.ctypes.data_as(dp)   # noqa: E731

    def call(o=obj, acq=0, par=p, cons=(c1,), thr=(0.0,), sn=(1,), Xs=xs):
        Cn = len(thr)
        h = (C.c_void_p * max(Cn, 1))(*[getattr(m, "_h", m) for m in cons]) if cons is not None else None
        t = np.array(thr, dtype=np.float64)
        s_ = np.array(sn, dtype=np.intc)
        return lib.bohip_gp_score_con(o._h if o is not None else None, acq, ptr(par) if par is not None else None, Cn, h,
                                      ptr(t) if Cn else None, s_.ctypes.data_as(ip) if Cn else None,
                                      ptr(Xs) if Xs is not None else None, R, ptr(out), None, None, None, None, None)

    assert call() == _lib.OK
    assert call(o=None) == _lib.E_ARG
    assert call(cons=tuple([c1] * 17), thr=tuple([0.0] * 17), sn=tuple([1] * 17)) == _lib.E_ARG          # C out of range
    assert lib.bohip_gp_score_con(obj._h, 0, ptr(p), -1, None, None, None, ptr(xs), R, ptr(out), None, None, None, None, None) == _lib.E_ARG
    assert call(cons=(None,)) == _lib.E_ARG                                                              # a null constraint handle
    assert call(cons=None) == _lib.E_ARG
    assert call(thr=(math.inf,)) == _lib.E_ARG and call(thr=(math.nan,)) == _lib.E_ARG
    assert call(sn=(0,)) == _lib.E_ARG and call(sn=(2,)) == _lib.E_ARG
    for bad in (_lib.ACQ["UCB"], _lib.ACQ["MI"], _lib.ACQ["MaxMean"], _lib.ACQ["ThompsonDraw"], 7, -2):
        assert call(acq=bad) == _lib.E_ARG, bad
    assert b"product form" in lib.bohip_last_error()
    assert call(par=None) == _lib.E_ARG and call(Xs=None) == _lib.E_ARG
    other = bohip.ElasticGPE(D_E2E + 1)
    assert call(cons=(other,)) == _lib.E_ARG and b"dimension" in lib.bohip_last_error()
    empty = bohip.ElasticGPE(D_E2E)
    assert call(o=empty) == _lib.E_STATE and call(cons=(empty,)) == _lib.E_STATE
    assert call(o=empty, acq=_lib.CON_FEASIBILITY, par=None) == _lib.OK                                   # the objective is not needed
    if lib.bohip_device_count() > 1:
        far = bohip.ElasticGPE(D_E2E, device=1)
        assert call(cons=(far,)) == _lib.E_ARG and b"device" in lib.bohip_last_error()
        far.close()
    # con_values and predict_grad
    mu = np.zeros((2, R))
    var = np.ones((2, R))
    t, s_ = np.array([0.0]), np.array([1], dtype=np.intc)
    cv = lambda acq=0, Cn=1, dm=None, dv=None, h=obj._h: lib.bohip_con_values(   # noqa: E731
        h, acq, ptr(p), Cn, ptr(t), s_.ctypes.data_as(ip), ptr(mu), ptr(var), R, ptr(out), None, dm, dv, None)
    assert cv() == _lib.OK and cv(h=None) == _lib.E_ARG and cv(acq=2) == _lib.E_ARG and cv(Cn=17) == _lib.E_ARG
    assert cv(dm=ptr(mu.copy())) == _lib.E_ARG                                                            # only one of dmu / dvar
    g = np.empty((D_E2E, R), order="F")
    assert lib.bohip_gp_predict_grad(empty._h, ptr(xs), R, ptr(out), ptr(out.copy()), ptr(g), ptr(g.copy())) == _lib.E_STATE
    assert lib.bohip_gp_predict_grad(obj._h, ptr(xs), R, ptr(out), ptr(out.copy()), ptr(g), None) == _lib.E_ARG
    assert lib.bohip_gp_predict_grad(None, ptr(xs), R, ptr(out), ptr(out.copy()), ptr(g), ptr(g.copy())) == _lib.E_ARG
    with pytest.raises(ValueError):
        bohip.ConstrainedGPE(obj, [c1], [0.0], [1]).score("UCB", [1.0], xs)
    other.close()
    empty.close()


# ---- 5. acquire_max and the loop ------------------------------------------------------------------------------------------------------
def test_acquire_max_with_and_without_refine(bohip, e2e_models):
    cm = bohip.ConstrainedGPE(e2e_models[0], [e2e_models[1], e2e_models[2]], [-0.3, 0.25], [1, -1])
    lb, ub = np.zeros(D_E2E), np.ones(D_E2E)
    for inner in (bohip.ExpectedImprovement(), bohip.LogExpectedImprovement()):
        a = bohip.Constrained(inner)
        assert cm.nobs == 65 and len({m.nobs for m in cm.members}) == 3
        a.a.tau = float(np.median(cm.y))                                        # (the members' observations are not aligned: no incumbent rule)
        f0, x0 = bohip.acquire_max(a, cm, lb, ub, dict(restarts=1, maxeval=512), np.random.default_rng(4), setparams=False)
        f1, x1 = bohip.acquire_max(a, cm, lb, ub, dict(restarts=1, maxeval=512, refine=4), np.random.default_rng(4), setparams=False)
        xs = bohip.latin_hypercube_sampling(lb, ub, 512, np.random.default_rng(4))
        res = cm.score(a.acq_id, a.params(), xs)
        assert f0 == res.best_val and np.array_equal(x0, xs[:, res.best_idx])   # the candidate route: one call, the device's arg-max
        assert f1 >= f0 and np.all(x1 >= lb) and np.all(x1 <= ub) and np.all(x0 >= lb) and np.all(x0 <= ub)
        again = cm.score(a.acq_id, a.params(), x1.reshape(-1, 1)).scores[0]
        assert again == pytest.approx(f1, rel=1e-9, abs=1e-12)
        print(f"{a.acq_id}: candidates {f0:.6g} -> refined {f1:.6g}")


def test_bopt_with_a_disc_constraint(bohip):
    """20 iterations on a 2-d toy: maximise -(|x - (0.7, 0.7)|^2) inside the disc |x - (0.4, 0.4)| <= 0.3 (g = 0.09 - r^2 >= 0).  Every
    proposal is in the box, the final optimum is feasible and better than the best feasible point of the initial design."""
    seen = []

    def func(x):
        y = -((x[0] - 0.7) ** 2 + (x[1] - 0.7) ** 2)
        g = 0.09 - ((x[0] - 0.4) ** 2 + (x[1] - 0.4) ** 2)
        seen.append((np.array(x), y, g))
        return y, g

    mk = lambda: bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(2, -1.0), -1.0), logNoise=-4.0,   # noqa: E731
                                  capacity=64)
    cm = bohip.ConstrainedGPE(mk(), [mk()], [0.0], [1])
    opt = bohip.MAPGPOptimizer(every=10, noisebounds=[-6, -2], kernbounds=[[-3, -3, -3], [1, 1, 1]], maxeval=20, domean=False)
    o = bohip.BOpt(func, cm, bohip.Constrained(bohip.LogExpectedImprovement()), opt, [0.0, 0.0], [1.0, 1.0], sense=bohip.Max,
                   maxiterations=20, initializer_iterations=5, verbosity=bohip.Silent, rng=np.random.default_rng(11),
                   acquisitionoptions=dict(maxeval=1024, refine=2))
    res = bohip.boptimize_(o)
    X = np.array([s[0] for s in seen])
    assert len(seen) == 20 and np.all(X >= 0.0) and np.all(X <= 1.0)
    assert cm.nobs == 20 and cm.constraints[0].nobs == 20
    feas = [s for s in seen if s[2] >= 0.0]
    assert feas
    best = max(feas, key=lambda s: s[1])
    assert res["observed_optimum"] == best[1] and np.array_equal(res["observed_optimizer"], best[0])
    xo = res["observed_optimizer"]
    assert 0.09 - ((xo[0] - 0.4) ** 2 + (xo[1] - 0.4) ** 2) >= 0.0               # the final optimum is feasible
    init_feas = [s[1] for s in seen[:5] if s[2] >= 0.0]
    print(f"initial feasible best {max(init_feas) if init_feas else None}, final {res['observed_optimum']:.6g} at {xo}, "
          f"{len(feas)} of 20 feasible; the constrained optimum is {-(math.hypot(0.3, 0.3) - 0.3) ** 2:.6g}")
    assert not init_feas or res["observed_optimum"] > max(init_feas)
    cm.close()
