"""Two-objective optimisation on the device (include/bohip_mo.h) against tests/mo_reference.py.

Bounds.  ehvi_values: 16 x mo_reference.WORST against the 50-digit evaluator, relative to the sum S the strip differences cancel
against (WORST is the twin's own measured error; the device's exp and erfc differ from libm's in the last bits).  score: the
first-order propagation of the members' moment and Jacobian bounds through the twin's partials (mo_reference.propagate)."""
import ctypes as C
import functools

import numpy as np
import pytest

import con_reference as cr
import mo_reference as mr
from conftest import synth
from matern_reference import MaternGP
from test_fit_gpu import centre, model_of
from test_mo_host import crafted_ref
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def anchor(bohip):
    m = bohip.ElasticGPE(2)                                                     # no observations: the device and the stream only
    yield m
    m.close()


# ---- 1. ehvi_values on crafted moments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 257, 1000])
@pytest.mark.parametrize("n_front", [0, 1, 15, 16, 17, 63, 65, 1024])
def test_ehvi_values_against_mpmath(bohip, anchor, n_front, R):
    """The group width's boundaries (15, 16, 17 strips a sweep more or less), one sweep against many, the largest front, a ragged last
    workgroup (R = 1000 is 62.5 workgroups of 16 candidates) and a single candidate."""
    fr, ref, mu, var, tab = crafted_ref(n_front, R)
    f, pm, pv, bv, bi = bohip.ehvi_values(anchor, fr, ref, mu, var, want_grad=True)
    f2, none_m, none_v, bv2, bi2 = bohip.ehvi_values(anchor, fr, ref, mu, var)
    assert none_m is None and none_v is None and f2.tobytes() == f.tobytes() and (bv2, bi2) == (bv, bi)
    sh = mr.shares((f, pm, pv), tab, {k: 16 * mr.WORST[k] for k in mr.KEYS})    # (asserts NaN columns for NaN / negative moments)
    tw = mr.shares(mr.ehvi(fr, ref, mu, var), tab, {k: 16 * mr.WORST[k] for k in mr.KEYS})
    print(f"n_front={n_front} R={R}: worst share of 16 x WORST {sh}; the twin's {tw}")
    assert max(sh.values()) <= 1.0, sh
    assert (bv, bi) == mr.record(f)                                             # the record of the device's own values: first maximum,
    assert bi >= 0 and f[bi] == bv and not np.isnan(bv)                         # NaN never wins
    if R >= 16:
        assert np.all(np.isnan(f[9:12])) and np.all(pv[0, [0, 1, 2, 6, 7, 8]] == 0.0) and np.all(pv[1, 3:9] == 0.0) and f[7] == 0.0


def test_ehvi_values_only_nan_candidates_and_none(bohip, anchor):
    fr, ref, mu, var = mr.crafted(5, 40, seed=1)
    f, _, _, bv, bi = bohip.ehvi_values(anchor, fr, ref, np.full((2, 40), np.nan), var)
    assert np.all(np.isnan(f)) and (bv, bi) == (-np.inf, -1)
    f, pm, pv, bv, bi = bohip.ehvi_values(anchor, fr, ref, np.zeros((2, 0)), np.zeros((2, 0)), want_grad=True)      # R = 0
    assert f.size == 0 and (bv, bi) == (-np.inf, -1)


def test_ehvi_values_beyond_one_grid_stride(bohip, anchor):
    """R = 16384 + 40: more candidates than the grid's 1024 workgroups hold groups of 16 lanes, so the first 40 groups take a second
    candidate.  What is computed for a candidate depends on its moments, the front and ref alone: the second stride scored alone
    (where it is the first) gives the same bytes, and a winner there is recorded with its index."""
    S1 = 16384
    R = S1 + 40
    fr, ref, mu, var = mr.crafted(17, R, seed=9)
    f, pm, pv, bv, bi = bohip.ehvi_values(anchor, fr, ref, mu, var, want_grad=True)
    assert (bv, bi) == mr.record(f)
    for sl in (slice(0, S1), slice(S1, R)):
        a = bohip.ehvi_values(anchor, fr, ref, mu[:, sl], var[:, sl], want_grad=True)
        assert a[0].tobytes() == f[sl].tobytes()
        assert np.ascontiguousarray(a[1]).tobytes() == np.ascontiguousarray(pm[:, sl]).tobytes()
        assert np.ascontiguousarray(a[2]).tobytes() == np.ascontiguousarray(pv[:, sl]).tobytes()
    late = mu.copy()
    late[0, :S1] = np.nan
    f3, _, _, bv3, bi3 = bohip.ehvi_values(anchor, fr, ref, late, var)
    assert np.all(np.isnan(f3[:S1])) and f3[S1:].tobytes() == f[S1:].tobytes() and (bv3, bi3) == mr.record(f3) and bi3 >= S1


def test_error_codes(bohip, anchor):
    from bohip import _lib

    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    R = 5
    mu, var, out, ref = np.zeros((2, R)), np.ones((2, R)), np.empty(R), np.array([-1.0, -1.0])
    good = np.array([[0.0, 1.0, 2.0], [2.0, 1.0, 0.0]])

    def ev(fr=good, n=None, r=ref, h=anchor._h, dm=None, dv=None, m=mu):
        return lib.bohip_mo_ehvi_values(h, ptr(fr), fr.shape[1] if n is None else n, ptr(r), ptr(m), ptr(var), R, ptr(out), dm, dv, None)

    assert ev() == _lib.OK and ev(h=None) == _lib.E_ARG and ev(r=None) == _lib.E_ARG and ev(m=None) == _lib.E_ARG
    big = np.stack([np.arange(1025.0), -np.arange(1025.0)]) + np.array([[0.0], [2000.0]])
    assert ev(fr=big) == _lib.E_UNSUPPORTED and b"1024" in lib.bohip_last_error()
    assert ev(fr=np.ascontiguousarray(big[:, :1024])) == _lib.OK
    assert ev(fr=np.array([[0.0, 2.0, 1.0], [2.0, 1.0, 0.0]])) == _lib.E_ARG                               # f1 not ascending
    assert ev(fr=np.array([[0.0, 1.0, 2.0], [2.0, 2.0, 0.0]])) == _lib.E_ARG                               # f2 not strictly descending
    assert ev(fr=np.array([[0.0, 1.0, 2.0], [2.0, 1.0, -1.0]])) == _lib.E_ARG                              # on ref, not above it
    assert ev(fr=np.array([[0.0, 1.0, np.nan], [2.0, 1.0, 0.0]])) == _lib.E_ARG
    assert ev(r=np.array([0.0, np.inf])) == _lib.E_ARG and ev(n=-1) == _lib.E_ARG
    assert ev(dm=ptr(mu.copy())) == _lib.E_ARG                                                              # only one of dmu / dvar
    X, y, Xs = synth(9, 3, R, seed=4)
    a, b_ = model_of(bohip, "SEArd", X, y), model_of(bohip, "Mat52Ard", X, -y)
    xs = np.asfortranarray(Xs.T)

    def sc(o0=a, o1=b_, fr=good, x=xs):
        return lib.bohip_gp_score_mo(getattr(o0, "_h", o0), getattr(o1, "_h", o1), ptr(fr), fr.shape[1], ptr(ref), ptr(x), R, ptr(out),
                                     None, None, None, None)

    assert sc() == _lib.OK and sc(o0=None) == _lib.E_ARG and sc(o1=None) == _lib.E_ARG and sc(x=None) == _lib.E_ARG
    assert sc(fr=big) == _lib.E_UNSUPPORTED and sc(fr=np.ascontiguousarray(good[:, ::-1])) == _lib.E_ARG
    other, empty = bohip.ElasticGPE(4), bohip.ElasticGPE(3)
    assert sc(o1=other) == _lib.E_ARG and b"dimension" in lib.bohip_last_error()
    assert sc(o1=empty) == _lib.E_STATE and sc(o0=empty) == _lib.E_STATE
    if lib.bohip_device_count() > 1:
        far = bohip.ElasticGPE(3, device=1)
        assert sc(o1=far) == _lib.E_ARG and b"device" in lib.bohip_last_error()
        far.close()
    for m in (a, b_, other, empty):
        m.close()


# ---- 2. score end to end -------------------------------------------------------------------------------------------------------------
#        kernels of the two objectives, their N, d
E2E = {"1x1": (("SEArd", "Mat12Iso"), (1, 1), 1), "17x3": (("Mat52Ard", "SEArd"), (17, 17), 3), "65x8": (("Mat32Iso", "Mat52Ard"), (65, 65), 8),
       "200x17": (("SEIso", "Mat12Ard"), (200, 200), 17), "40+65": (("Mat52Ard", "Mat32Ard"), (40, 65), 4),
       "split-K": (("Mat52Ard", "SEArd"), (1000, 1000), 4)}


def twin_of(kern, X, y):
    t = centre(kern, X.shape[1])
    return MaternGP(kern, X, y, t[2:-1], t[-1], t[0], t[1])


@functools.lru_cache(maxsize=None)
def e2e_data(case):
    """The two members' observations, their twins, and a front: the front of the observations both members share, above the default
    rule's reference point."""
    kerns, Ns, d = E2E[case]
    N = max(Ns)
    X, y0, Xs = synth(N, d, 300, seed=4000 + 7 * N + d)
    y1 = np.cos(2.0 * X).sum(1) - 0.5 * X[:, 0] + 0.1 * np.random.default_rng(N + d).standard_normal(N)
    ys = (y0[:Ns[0]], y1[:Ns[1]])
    n = min(Ns)
    Y = np.stack([y0[:n], y1[:n]])
    lo, hi = Y.min(axis=1), Y.max(axis=1)
    ref = np.where(hi - lo > 0, lo - 0.1 * (hi - lo), lo - 1.0)
    fr, _ = mr.front(Y, ref)
    twins = tuple(twin_of(k, X[:m], y) for k, m, y in zip(kerns, Ns, ys))
    for a in (X, Xs, fr, ref) + ys:
        a.setflags(write=False)
    return X, ys, Xs, fr, ref, twins


@functools.lru_cache(maxsize=None)
def e2e_twin(case, R):
    X, ys, Xs, fr, ref, twins = e2e_data(case)
    tw = mr.score_mo(twins, fr, ref, Xs[:R])
    return tw, mr.propagate(twins, tw)


@pytest.fixture(scope="module")
def e2e_models(bohip):
    made = {}

    def get(case):
        if case not in made:
            kerns, Ns, d = E2E[case]
            X, ys, *_ = e2e_data(case)
            made[case] = tuple(model_of(bohip, k, X[:m], y) for k, m, y in zip(kerns, Ns, ys))
        return made[case]

    yield get
    for ms in made.values():
        for m in ms:
            m.close()


def smooth_mask(tw, fr, ref):
    """Candidates where both members have sigma^2 > 0 and lie within 6 sigma of a corner of the front: where the score is not
    flat to rounding, so a first-order bound on its gradient means something."""
    c, b = mr.corners(fr, ref)
    ok = np.ones(tw["scores"].size, dtype=bool)
    for m, t in ((0, c[:-1]), (1, b)):
        with np.errstate(all="ignore"):
            z = np.abs(tw["mu"][m][:, None] - t[None, :]) / np.sqrt(tw["var"][m])[:, None]
            ok &= (tw["var"][m] > 0) & (z.min(axis=1) < 6.0)
    return ok


@pytest.mark.parametrize("R", [1, 17, 300])
@pytest.mark.parametrize("case", ["1x1", "17x3", "65x8", "200x17", "40+65"])
def test_score_against_the_twin(bohip, e2e_models, case, R):
    X, ys, Xs, fr, ref, twins = e2e_data(case)
    tw, (ts, tg) = e2e_twin(case, R)
    m0, m1 = e2e_models(case)
    xs = Xs[:R].T
    val = bohip.model.score_mo(m0, m1, fr, ref, xs)
    grd = bohip.model.score_mo(m0, m1, fr, ref, xs, want_grad=True)
    for a, b in ((val.scores, grd.scores), (val.mu, grd.mu), (val.var, grd.var)):
        assert a.tobytes() == b.tobytes()                                       # value call == gradient call, bit for bit
    assert (val.best_value, val.best_index) == (grd.best_value, grd.best_index) and val.grad is None and grd.grad.shape == (xs.shape[0], R)
    s_share = np.max(np.abs(val.scores - tw["scores"]) / ts)
    smooth = smooth_mask(tw, fr, ref)
    g_share = np.max(np.abs(grd.grad.T - tw["grad"])[smooth] / tg[smooth]) if smooth.any() else 0.0
    print(f"{case} R={R} n_front={fr.shape[1]}: worst share of the bound: score {s_share:.3g}, gradient {g_share:.3g} on "
          f"{int(smooth.sum())} smooth candidates")
    assert s_share <= 1.0 and g_share <= 1.0
    assert np.all(np.isfinite(grd.grad)) and np.all(np.isfinite(val.scores))
    for m_ in range(2):
        bm, bv = cr.moment_bounds(twins[m_], tw["mu"][m_], tw["var"][m_])
        assert np.all(np.abs(val.mu[m_] - tw["mu"][m_]) <= bm) and np.all(np.abs(val.var[m_] - tw["var"][m_]) <= bv)
    assert (val.best_value, val.best_index) == mr.record(val.scores)
    # the bitwise properties: the EHVI stage alone on the returned moments, a second call, and a slice scored alone
    again = bohip.ehvi_values(m0, fr, ref, val.mu, val.var)
    assert again[0].tobytes() == val.scores.tobytes() and again[3:] == (val.best_value, val.best_index)
    twice = bohip.model.score_mo(m0, m1, fr, ref, xs, want_grad=True)
    assert twice.scores.tobytes() == grd.scores.tobytes() and twice.grad.tobytes(order="F") == grd.grad.tobytes(order="F")
    if R > 1:
        h = R // 2
        a, b = (bohip.model.score_mo(m0, m1, fr, ref, part, want_grad=True) for part in (xs[:, :h], xs[:, h:]))
        assert np.concatenate([a.scores, b.scores]).tobytes() == grd.scores.tobytes()
        assert np.concatenate([a.grad, b.grad], axis=1).tobytes(order="F") == grd.grad.tobytes(order="F")


def test_score_on_the_split_k_route(bohip, e2e_models):
    """N = 1000, d = 4, R = 40: eight row tiles and few candidate tiles take the split-K posterior on both members."""
    case, R = "split-K", 40
    X, ys, Xs, fr, ref, twins = e2e_data(case)
    tw, (ts, tg) = e2e_twin(case, R)
    m0, m1 = e2e_models(case)
    val = bohip.model.score_mo(m0, m1, fr, ref, Xs[:R].T)
    grd = bohip.model.score_mo(m0, m1, fr, ref, Xs[:R].T, want_grad=True)
    assert val.scores.tobytes() == grd.scores.tobytes() and (val.best_value, val.best_index) == mr.record(val.scores)
    smooth = smooth_mask(tw, fr, ref)
    s_share = np.max(np.abs(val.scores - tw["scores"]) / ts)
    g_share = np.max(np.abs(grd.grad.T - tw["grad"])[smooth] / tg[smooth]) if smooth.any() else 0.0
    print(f"split-K n_front={fr.shape[1]}: worst share of the bound: score {s_share:.3g}, gradient {g_share:.3g} on {int(smooth.sum())}")
    assert s_share <= 1.0 and g_share <= 1.0


def test_one_handle_for_both_objectives(bohip, e2e_models):
    """obj0 is obj1: accepted; the score is the EHVI stage on the handle's moments in both rows."""
    X, ys, Xs, fr, ref, twins = e2e_data("17x3")
    m0, _ = e2e_models("17x3")
    y = np.asarray(m0.y)
    Y = np.stack([y, y])
    r = np.array([y.min() - 1.0, y.min() - 1.0])
    fr1, _ = mr.front(Y, r)                                                     # one point: the maximum, twice
    assert fr1.shape == (2, 1)
    res = bohip.model.score_mo(m0, m0, fr1, r, Xs[:33].T, want_grad=True)
    assert res.mu[0].tobytes() == res.mu[1].tobytes() and res.var[0].tobytes() == res.var[1].tobytes()
    again = bohip.ehvi_values(m0, fr1, r, res.mu, res.var)
    assert again[0].tobytes() == res.scores.tobytes() and np.all(np.isfinite(res.grad)) and np.all(res.scores >= 0.0)
    mo = bohip.MultiObjectiveGPE((m0, m0), ref=r)
    assert mo.front.tobytes() == fr1.tobytes() and mo.score(Xs[:33].T, want_grad=True).scores.tobytes() == res.scores.tobytes()


# ---- 3. the gradient against central differences of the twin's score ----------------------------------------------------------------
STEP = 1e-3                                                                     # (test_con_host's step and recipe)


def test_gradient_against_central_differences_of_the_twin(bohip, e2e_models):
    """Richardson's (4 D(h) - D(2h)) / 3 of the twin's score in x at five candidates: what is left is bounded by |D(2h) - D(h)| / 3,
    rounding by 6 noise / h (noise: the twin's score by two routes, never below 8 eps max|f|), and the device's gradient differs from
    the twin's by the propagated bound."""
    case = "17x3"
    X, ys, Xs, fr, ref, twins = e2e_data(case)
    m0, m1 = e2e_models(case)
    rng = np.random.default_rng(123)
    pts = []
    while len(pts) < 5:
        x = rng.random(3)
        if np.min(np.abs(x[None, :] - X).max(axis=1)) < 8 * STEP:
            continue
        t = mr.score_mo(twins, fr, ref, x[None, :])
        if smooth_mask(t, fr, ref)[0] and t["scores"][0] > 1e-6:
            pts.append(x)
    pts = np.array(pts)
    tw = mr.score_mo(twins, fr, ref, pts)
    _, tg = mr.propagate(twins, tw)
    dev = bohip.model.score_mo(m0, m1, fr, ref, pts.T, want_grad=True)

    def by_predict(P):
        mv = [m.predict(P) for m in twins]
        return mr.ehvi(fr, ref, np.array([a for a, _ in mv]), np.array([b for _, b in mv]))[0]

    val = by_predict(pts)
    noise = max(np.abs(tw["scores"] - val).max(), 8 * np.finfo(np.float64).eps * np.abs(val).max())
    worst = 0.0
    for i, x in enumerate(pts):
        for k in range(3):
            e = np.zeros(3)
            e[k] = STEP
            f = by_predict(np.array([x + e, x - e, x + 2 * e, x - 2 * e]))
            d1, d2 = (f[0] - f[1]) / (2 * STEP), (f[2] - f[3]) / (4 * STEP)
            rich = (4.0 * d1 - d2) / 3.0
            bound = abs(d2 - d1) / 3.0 + 6.0 * noise / STEP + tg[i, k]
            err = abs(dev.grad[k, i] - rich)
            worst = max(worst, err / bound)
            assert err <= bound, (i, k, dev.grad[k, i], rich, err / bound)
    print(f"worst share of the bound {worst:.3g}")


# ---- 4. the loop -----------------------------------------------------------------------------------------------------------------------
def test_bopt_with_two_quadratic_objectives(bohip):
    """d = 2, f1 = -|x - a|^2, f2 = -|x - b|^2, 8 initial points and 12 iterations with "refine": 4, against the fixed reference point
    (-1.5, -1.5): the hypervolume of the observations never decreases and ends above its value after the initial design.  The same
    loop was run beforehand on the CPU with the twins alone (matern_reference.MaternGP members and mo_reference's EHVI in place of the
    device call, the same seeds and hyper-parameters): the hypervolume rose from 2.13781 after the initial design to 2.18944, with
    10 of the 12 proposals improving it (they line up along the segment between a and b, the Pareto set)."""
    a_, b_ = np.array([0.2, 0.3]), np.array([0.8, 0.7])
    ref = np.array([-1.5, -1.5])
    seen, hvs = [], []

    def func(x):
        y = (-float(np.sum((x - a_) ** 2)), -float(np.sum((x - b_) ** 2)))
        seen.append((np.array(x), y))
        hvs.append(mr.front(np.array([s[1] for s in seen]).T, ref)[1])
        return y

    mk = lambda: bohip.ElasticGPE(2, mean=bohip.MeanConst(-0.4), kernel=bohip.SEArd(np.full(2, -0.3), -0.7), logNoise=-4.0,   # noqa: E731
                                  capacity=32)
    mo = bohip.MultiObjectiveGPE((mk(), mk()), ref=ref)
    o = bohip.BOpt(func, mo, bohip.ExpectedHypervolumeImprovement(), bohip.NoModelOptimizer(), [0.0, 0.0], [1.0, 1.0], sense=bohip.Max,
                   maxiterations=20, initializer_iterations=8, verbosity=bohip.Silent, rng=np.random.default_rng(11),
                   acquisitionoptions=dict(maxeval=512, refine=4))
    res = bohip.boptimize_(o)
    X = np.array([s[0] for s in seen])
    assert len(seen) == 20 and np.all(X >= 0.0) and np.all(X <= 1.0) and mo.nobs == 20
    assert all(b >= a for a, b in zip(hvs, hvs[1:])), hvs
    print(f"hypervolume after the initial design {hvs[7]:.6g}, at the end {hvs[-1]:.6g}; {sum(b > a for a, b in zip(hvs[7:], hvs[8:]))} of 12 "
          f"proposals improved it; the front has {res['observed_front']['y'].shape[1]} points")
    assert hvs[-1] > hvs[7]
    assert res["hypervolume"] == hvs[-1] == mo.hypervolume and res["observed_optimum"] is None
    tf, _ = mr.front(np.array([s[1] for s in seen]).T, ref)
    np.testing.assert_array_equal(res["observed_front"]["y"], tf)
    mo.close()


def test_map_optimizer_fits_each_member(bohip):
    """sense = Min with MAPGPOptimizer: both members are fitted (their length scales leave the initial values), both hold the flipped
    observations, and the front comes back in the caller's sense."""
    seen = []

    def func(x):
        y = (float(np.sum((x - 0.2) ** 2)), float(np.sum((x - 0.8) ** 2)))    # both minimised
        seen.append((np.array(x), y))
        return y

    mk = lambda: bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(2, -1.0), -1.0), logNoise=-4.0,   # noqa: E731
                                  capacity=32)
    mo = bohip.MultiObjectiveGPE((mk(), mk()))
    opt = bohip.MAPGPOptimizer(every=2, noisebounds=[-6, -2], kernbounds=[[-3, -3, -3], [1, 1, 1]], maxeval=20, domean=False)
    o = bohip.BOpt(func, mo, bohip.ExpectedHypervolumeImprovement(), opt, [0.0, 0.0], [1.0, 1.0], sense=bohip.Min, maxiterations=10,
                   initializer_iterations=6, verbosity=bohip.Silent, rng=np.random.default_rng(3), acquisitionoptions=dict(maxeval=256))
    res = bohip.boptimize_(o)
    Yc = np.array([s[1] for s in seen]).T
    assert len(seen) == 10 and mo.y.tobytes() == (-Yc).tobytes()
    for m in mo.members:
        assert not np.array_equal(m.kernel.ll, np.full(2, -1.0)), "a member was not fitted"
    tf, thv = mr.front(-Yc, mo.ref)
    np.testing.assert_array_equal(res["observed_front"]["y"], -tf)
    assert res["hypervolume"] == thv > 0.0 and np.all(res["observed_front"]["y"] >= 0.0)
    fx = res["observed_front"]["x"]
    assert all(func(fx[:, i]) == tuple(res["observed_front"]["y"][:, i]) for i in range(fx.shape[1]))
    mo.close()
