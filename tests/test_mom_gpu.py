"""Two to four objectives on the device (include/bohip_mom.h) against tests/mom_reference.py.

Bounds.  ehvi_values_many: 16 x mom_reference.WORST against the 50-digit evaluator, relative to the box sum S the differences cancel
against (WORST is the twin's own measured error; the device's exp and erfc differ from libm's in the last bits).  score_mom: the
first-order propagation of the members' moment and Jacobian bounds through the twin's partials (mom_reference.propagate)."""
import ctypes as C
import functools

import numpy as np
import pytest

import con_reference as cr
import mo_reference as mr
import mom_reference as qr
from conftest import synth
from test_fit_gpu import model_of
from test_mo_gpu import twin_of
from test_mom_host import crafted_ref
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def anchor(bohip):
    m = bohip.ElasticGPE(2)                                                     # no observations: the device and the stream only
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def staircase_ref(M, n, R):
    """A front of n + M - 1 boxes (mom_reference.staircase) with crafted moments and their 50-digit table."""
    rng = np.random.default_rng(7000 + 100 * M + n)
    fr, ref = qr.staircase(M, n), qr.REF4[:M].copy()
    mu, var = qr.crafted_moments(fr, ref, R, rng)
    return fr, ref, mu, var, qr.mp_table(fr, ref, mu, var)


def check_values(bohip, anchor, fr, ref, mu, var, tab, what):
    M, R = mu.shape
    f, pm, pv, bv, bi = bohip.ehvi_values_many(anchor, fr, ref, mu, var, want_grad=True)
    f2, none_m, none_v, bv2, bi2 = bohip.ehvi_values_many(anchor, fr, ref, mu, var)
    assert none_m is None and none_v is None and f2.tobytes() == f.tobytes() and (bv2, bi2) == (bv, bi)      # value form == GRAD form
    sh = qr.shares((f, pm, pv), tab, 16 * qr.WORST)                              # (asserts NaN columns for NaN / negative moments)
    tw = qr.shares(qr.ehvi(fr, ref, mu, var), tab, 16 * qr.WORST)
    print(f"{what}: worst share of 16 x WORST {max(sh.values()):.3g} ({max(sh, key=sh.get)}); the twin's {max(tw.values()):.3g}")
    assert max(sh.values()) <= 1.0, sh
    assert (bv, bi) == qr.record(f)                                             # the record of the device's own values: first maximum,
    assert bi >= 0 and f[bi] == bv and not np.isnan(bv)                         # NaN never wins
    if R >= 16:
        assert np.all(np.isnan(f[9:12])) and np.all(np.isnan(pm[:, 9:12])) and np.all(np.isnan(pv[:, 9:12]))
        assert np.all(pv[0, [0, 1, 2, 6, 7, 8]] == 0.0) and np.all(pv[M - 1, 3:9] == 0.0) and f[7] == 0.0
    return f, pm, pv


# ---- 1. ehvi_values_many on crafted moments -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", qr.GRID, ids=lambda c: "M{}-n{}-R{}".format(*c))
def test_ehvi_values_against_mpmath(bohip, anchor, case):
    """Fronts of 0, 1, 2 and 17 points at R = 257 (64 workgroups of 4 candidates and one of 1), 2336 boxes at M = 3 and 796 at
    M = 4 (37 and 13 sweeps of the 64 lanes)."""
    M, n_front, R = case
    fr, ref, mu, var, tab = crafted_ref(M, n_front, R)
    check_values(bohip, anchor, fr, ref, mu, var, tab, f"M={M} n_front={n_front} R={R} boxes={qr.boxes(fr, ref)[1].shape[1]}")


@pytest.mark.parametrize("boxes", [63, 64, 65])
@pytest.mark.parametrize("M", [3, 4])
def test_ehvi_values_around_one_sweep_of_the_lanes(bohip, anchor, M, boxes):
    """63, 64 and 65 boxes: a sweep less one lane, exactly one sweep, one sweep and one box."""
    fr, ref, mu, var, tab = staircase_ref(M, boxes - (M - 1), 40)
    assert qr.boxes(fr, ref)[1].shape[1] == boxes
    check_values(bohip, anchor, fr, ref, mu, var, tab, f"M={M} boxes={boxes}")


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_ehvi_values_on_a_few_candidates(bohip, anchor, M, R):
    fr, ref, mu, var = qr.crafted(M, 17, R, seed=40 + M + R)
    check_values(bohip, anchor, fr, ref, mu, var, qr.mp_table(fr, ref, mu, var), f"M={M} R={R}")


def test_ehvi_values_only_nan_candidates_and_none(bohip, anchor):
    fr, ref, mu, var = qr.crafted(3, 5, 40, seed=1)
    f, _, _, bv, bi = bohip.ehvi_values_many(anchor, fr, ref, np.full((3, 40), np.nan), var)
    assert np.all(np.isnan(f)) and (bv, bi) == (-np.inf, -1)
    f, pm, pv, bv, bi = bohip.ehvi_values_many(anchor, fr, ref, np.zeros((3, 0)), np.zeros((3, 0)), want_grad=True)      # R = 0
    assert f.size == 0 and (bv, bi) == (-np.inf, -1)


# ---- 2. two objectives against the strip form on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("n_front", [0, 2, 17])
def test_two_objectives_against_the_strip_kernel(bohip, anchor, n_front):
    """M = 2: k_ehvi_boxes against k_ehvi on the same inputs, within the sum of the two kernels' bounds (16 x WORST of each twin,
    each relative to the sum its own differences cancel against)."""
    fr, ref, mu, var, tab = crafted_ref(2, n_front, 257)
    fs = np.ascontiguousarray(fr[:, np.argsort(fr[0])])
    strip_tab = mr.mp_table(fs, ref, mu, var)
    a = bohip.ehvi_values_many(anchor, fr, ref, mu, var, want_grad=True)
    b = bohip.ehvi_values(anchor, fs, ref, mu, var, want_grad=True)
    ok = np.isfinite(tab["value"])
    mine = dict(zip(qr.keys(2), (a[0],) + tuple(a[1]) + tuple(a[2])))
    theirs = dict(zip(qr.keys(2), (b[0],) + tuple(b[1]) + tuple(b[2])))
    for k, ks in zip(qr.keys(2), ("value", "dmu1", "dmu2", "dvar1", "dvar2")):
        bound = 16 * qr.WORST * np.maximum(tab["S_" + k][ok], 1e-300) + 16 * mr.WORST[ks] * np.maximum(strip_tab["S_" + ks][ok], 1e-300)
        share = np.max(np.abs(mine[k][ok] - theirs[k][ok]) / bound)
        print(f"n_front={n_front} {k}: worst share of the two bounds {share:.3g}")
        assert share <= 1.0, k
        assert np.all(np.isnan(mine[k][~ok])) and np.all(np.isnan(theirs[k][~ok]))


# ---- 3. beyond one stride of the grid, 4. a permuted front -------------------------------------------------------------------------
def test_ehvi_values_beyond_one_grid_stride(bohip, anchor):
    """R = 4096 + 40: more candidates than the grid's 1024 workgroups hold wavefronts -- 4 a workgroup in the value form, 2 in the
    GRAD form, so that form runs two whole strides and a ragged third.  What is computed for a candidate depends on its moments, the
    front and ref alone: each stride scored alone (where it is the first) gives the same bytes, and a winner in the last stride is
    recorded with its index."""
    S1 = 4096
    R = S1 + 40
    fr, ref, mu, var = qr.crafted(3, 8, R, seed=9)
    f, pm, pv, bv, bi = bohip.ehvi_values_many(anchor, fr, ref, mu, var, want_grad=True)
    f0, _, _, bv0, bi0 = bohip.ehvi_values_many(anchor, fr, ref, mu, var)
    assert (bv, bi) == qr.record(f) == (bv0, bi0) and f0.tobytes() == f.tobytes()
    for sl in (slice(0, 2048), slice(2048, S1), slice(S1, R)):
        a = bohip.ehvi_values_many(anchor, fr, ref, mu[:, sl], var[:, sl], want_grad=True)
        assert a[0].tobytes() == f[sl].tobytes()
        assert a[1].tobytes() == np.ascontiguousarray(pm[:, sl]).tobytes() and a[2].tobytes() == np.ascontiguousarray(pv[:, sl]).tobytes()
        assert bohip.ehvi_values_many(anchor, fr, ref, mu[:, sl], var[:, sl])[0].tobytes() == f[sl].tobytes()
    late = mu.copy()
    late[0, :S1] = np.nan
    for grad_form in (False, True):
        f3, _, _, bv3, bi3 = bohip.ehvi_values_many(anchor, fr, ref, late, var, want_grad=grad_form)
        assert np.all(np.isnan(f3[:S1])) and f3[S1:].tobytes() == f[S1:].tobytes() and (bv3, bi3) == qr.record(f3) and bi3 >= S1


@pytest.mark.parametrize("M", [2, 3, 4])
def test_a_permuted_front_gives_the_same_bytes(bohip, anchor, M):
    fr, ref, mu, var, _ = crafted_ref(M, 17, 257)
    a = bohip.ehvi_values_many(anchor, fr, ref, mu, var, want_grad=True)
    perm = np.random.default_rng(M).permutation(17)
    b = bohip.ehvi_values_many(anchor, np.ascontiguousarray(fr[:, perm]), ref, mu, var, want_grad=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3:] == b[3:]


def test_the_resident_plan_follows_the_front(bohip, anchor):
    """The handle keeps the decomposition of the last (front, ref): the same front again reuses it, another front of the same shape,
    another ref, and a front of another M with as many numbers (M (n + 1) = 12) replace it -- every call gives the bytes of a
    fresh handle's."""
    rng = np.random.default_rng(77)
    cases = []
    for M, n in ((3, 3), (3, 3), (2, 5), (4, 2), (3, 3)):
        fr = qr.sphere_front(M, n, rng)
        mu, var = qr.crafted_moments(fr, qr.REF4[:M], 33, rng)
        cases.append((fr, qr.REF4[:M].copy(), mu, var))
    cases.append((cases[0][0], cases[0][1] - 0.5, cases[0][2], cases[0][3]))    # the first front above another ref
    fresh = []
    for fr, ref, mu, var in cases:
        h = bohip.ElasticGPE(2)
        fresh.append(bohip.ehvi_values_many(h, fr, ref, mu, var, want_grad=True))
        h.close()
    for order in ((0, 0, 1, 0, 5, 0), (2, 3, 4, 2, 3, 4, 1)):
        for i in order:
            fr, ref, mu, var = cases[i]
            got = bohip.ehvi_values_many(anchor, fr, ref, mu, var, want_grad=True)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], fresh[i][:3])) and got[3:] == fresh[i][3:], i


# ---- 5. score_mom end to end ---------------------------------------------------------------------------------------------------------
#        kernels of the objectives, their N, d
E2E = {"1x1": (("SEArd", "Mat12Iso", "Mat52Ard"), (1, 1, 1), 1), "17x3": (("Mat52Ard", "SEArd", "Mat32Iso"), (17, 17, 17), 3),
       "65x8": (("Mat32Iso", "Mat52Ard", "SEIso", "Mat12Ard"), (65, 65, 65, 65), 8),
       "17x3x4": (("SEArd", "Mat52Ard", "Mat32Ard", "SEArd"), (17, 17, 17, 17), 3),
       "40+65+17": (("Mat52Ard", "Mat32Ard", "SEArd"), (40, 65, 17), 4),
       "split-K": (("Mat52Ard", "SEArd", "Mat32Ard"), (1000, 1000, 1000), 4)}


@functools.lru_cache(maxsize=None)
def e2e_data(case):
    """The members' observations, their twins, and a front: the front of the observations every member shares, above the default
    rule's reference point."""
    kerns, Ns, d = E2E[case]
    M, N = len(kerns), max(Ns)
    X, y0, Xs = synth(N, d, 40, seed=6000 + 7 * N + d)
    rng = np.random.default_rng(N + d)
    rows = [y0, np.cos(2.0 * X).sum(1) - 0.5 * X[:, 0] + 0.1 * rng.standard_normal(N), -((X - 0.5) ** 2).sum(1) + 0.1 * rng.standard_normal(N),
            np.sin(5.0 * X[:, 0]) - X.sum(1) / d + 0.1 * rng.standard_normal(N)][:M]
    ys = tuple(r[:n] for r, n in zip(rows, Ns))
    n = min(Ns)
    Y = np.stack([r[:n] for r in rows])
    lo, hi = Y.min(axis=1), Y.max(axis=1)
    ref = np.where(hi - lo > 0, lo - 0.1 * (hi - lo), lo - 1.0)
    fr, _ = qr.front(Y, ref)
    twins = tuple(twin_of(k, X[:m], y) for k, m, y in zip(kerns, Ns, ys))
    for a in (X, Xs, fr, ref) + ys:
        a.setflags(write=False)
    return X, ys, Xs, fr, ref, twins


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
    """Candidates where every member has sigma^2 > 0 and lies within 6 sigma of a level of the front: where the score is not flat to
    rounding, so a first-order bound on its gradient means something."""
    L = qr.levels_of(fr, ref)
    ok = np.ones(tw["scores"].size, dtype=bool)
    for m in range(len(L)):
        with np.errstate(all="ignore"):
            z = np.abs(tw["mu"][m][:, None] - L[m][None, :-1]) / np.sqrt(tw["var"][m])[:, None]
            ok &= (tw["var"][m] > 0) & (z.min(axis=1) < 6.0)
    return ok


@pytest.mark.parametrize("case,R", [("1x1", 1), ("1x1", 17), ("17x3", 17), ("65x8", 40), ("17x3x4", 40), ("40+65+17", 40), ("split-K", 40)])
def test_score_against_the_twin(bohip, e2e_models, case, R):
    """Three and four members with mixed kernel ids, members of unequal N, and N = 1000 on the split-K posterior."""
    X, ys, Xs, fr, ref, twins = e2e_data(case)
    M = len(twins)
    tw = qr.score_mom(twins, fr, ref, Xs[:R])
    ts, tg = qr.propagate(twins, tw)
    ms = e2e_models(case)
    xs = Xs[:R].T
    val = bohip.score_mom(ms, fr, ref, xs)
    grd = bohip.score_mom(ms, fr, ref, xs, want_grad=True)
    for a, b in ((val.scores, grd.scores), (val.mu, grd.mu), (val.var, grd.var)):
        assert a.tobytes() == b.tobytes()                                       # value call == gradient call, bit for bit
    assert (val.best_value, val.best_index) == (grd.best_value, grd.best_index) and val.grad is None and grd.grad.shape == (xs.shape[0], R)
    assert val.mu.shape == (M, R) and val.var.shape == (M, R)
    s_share = np.max(np.abs(val.scores - tw["scores"]) / ts)
    smooth = smooth_mask(tw, fr, ref)
    g_share = np.max(np.abs(grd.grad.T - tw["grad"])[smooth] / tg[smooth]) if smooth.any() else 0.0
    print(f"{case} R={R} M={M} n_front={fr.shape[1]} boxes={qr.boxes(fr, ref)[1].shape[1]}: worst share of the bound: score {s_share:.3g}, "
          f"gradient {g_share:.3g} on {int(smooth.sum())} smooth candidates")
    assert s_share <= 1.0 and g_share <= 1.0
    assert np.all(np.isfinite(grd.grad)) and np.all(np.isfinite(val.scores))
    for m_ in range(M):
        bm, bv = cr.moment_bounds(twins[m_], tw["mu"][m_], tw["var"][m_])
        assert np.all(np.abs(val.mu[m_] - tw["mu"][m_]) <= bm) and np.all(np.abs(val.var[m_] - tw["var"][m_]) <= bv)
    assert (val.best_value, val.best_index) == qr.record(val.scores)
    # the bitwise properties: the stage alone on the returned moments, and a slice scored alone
    again = bohip.ehvi_values_many(ms[0], fr, ref, val.mu, val.var)
    assert again[0].tobytes() == val.scores.tobytes() and again[3:] == (val.best_value, val.best_index)
    if R > 1:
        h = R // 2
        a, b = (bohip.score_mom(ms, fr, ref, part, want_grad=True) for part in (xs[:, :h], xs[:, h:]))
        assert np.concatenate([a.scores, b.scores]).tobytes() == grd.scores.tobytes()
        assert np.concatenate([a.grad, b.grad], axis=1).tobytes(order="F") == grd.grad.tobytes(order="F")


def test_a_repeated_handle(bohip, e2e_models):
    """objs = (a, b, a): accepted; rows 0 and 2 of the moments are the same bytes, the score is the stage on them, and the model
    class scores the same bytes."""
    X, ys, Xs, fr, ref, twins = e2e_data("17x3")
    m0, m1, _ = e2e_models("17x3")
    Y = np.stack([np.asarray(m0.y), np.asarray(m1.y), np.asarray(m0.y)])
    r = Y.min(axis=1) - 1.0
    fr1, _ = qr.front(Y, r)
    res = bohip.score_mom((m0, m1, m0), fr1, r, Xs[:33].T, want_grad=True)
    assert res.mu[0].tobytes() == res.mu[2].tobytes() and res.var[0].tobytes() == res.var[2].tobytes()
    again = bohip.ehvi_values_many(m0, fr1, r, res.mu, res.var)
    assert again[0].tobytes() == res.scores.tobytes() and np.all(np.isfinite(res.grad)) and np.all(res.scores >= 0.0)
    mo = bohip.ManyObjectiveGPE((m0, m1, m0), ref=r)
    assert mo.front.tobytes() == fr1.tobytes() and mo.score(Xs[:33].T, want_grad=True).scores.tobytes() == res.scores.tobytes()


# ---- 6. error codes ---------------------------------------------------------------------------------------------------------------
def test_error_codes(bohip, anchor):
    from bohip import _lib

    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    R = 5
    mu, var, out, ref = np.zeros((3, R)), np.ones((3, R)), np.empty(R), np.array([-1.0, -1.0, -1.0])
    good = np.array([[0.0, 1.0, 2.0], [2.0, 1.0, 0.0], [0.5, 0.5, 0.25]])

    def ev(fr=good, n=None, r=ref, h=anchor._h, dm=None, dv=None, m=mu, M=3):
        return lib.bohip_mom_ehvi_values(h, M, ptr(fr), fr.shape[1] if n is None else n, ptr(r), ptr(m), ptr(var), R, ptr(out), dm, dv, None)

    assert ev() == _lib.OK and ev(h=None) == _lib.E_ARG and ev(r=None) == _lib.E_ARG and ev(m=None) == _lib.E_ARG
    assert ev(M=1) == _lib.E_ARG and ev(M=5) == _lib.E_ARG
    rng = np.random.default_rng(0)
    assert ev(fr=qr.sphere_front(3, 257, rng), r=qr.REF4[:3]) == _lib.E_UNSUPPORTED and b"257" in lib.bohip_last_error()
    assert ev(fr=qr.sphere_front(3, 256, rng), r=qr.REF4[:3]) == _lib.OK
    mu4, var4 = np.zeros((4, R)), np.ones((4, R))
    assert lib.bohip_mom_ehvi_values(anchor._h, 4, ptr(qr.sphere_front(4, 256, rng)), 256, ptr(qr.REF4), ptr(mu4), ptr(var4), R, ptr(out),
                                     None, None, None) == _lib.E_UNSUPPORTED and b"65536" in lib.bohip_last_error()
    assert ev(fr=np.array([[0.0, 1.0, 1.0], [2.0, 1.0, 1.0], [0.5, 0.5, 0.5]])) == _lib.E_ARG              # a duplicated point
    assert ev(fr=np.array([[0.0, 1.0, 1.0], [2.0, 1.0, 0.5], [0.5, 0.5, 0.5]])) == _lib.E_ARG              # a weakly dominated point
    assert ev(fr=np.array([[0.0, 1.0, 2.0], [2.0, 1.0, -1.0], [0.5, 0.5, 0.25]])) == _lib.E_ARG            # on ref, not above it
    assert ev(fr=np.array([[0.0, 1.0, np.nan], [2.0, 1.0, 0.0], [0.5, 0.5, 0.25]])) == _lib.E_ARG
    assert ev(r=np.array([0.0, np.inf, 0.0])) == _lib.E_ARG and ev(n=-1) == _lib.E_ARG
    assert ev(dm=ptr(mu.copy())) == _lib.E_ARG                                                              # only one of dmu / dvar
    X, y, Xs = synth(9, 3, R, seed=4)
    a, b_, c_ = model_of(bohip, "SEArd", X, y), model_of(bohip, "Mat52Ard", X, -y), model_of(bohip, "Mat32Iso", X, y * y)
    xs = np.asfortranarray(Xs.T)

    def sc(objs=(a, b_, c_), fr=good, x=xs, M=None):
        hs = (C.c_void_p * len(objs))(*[getattr(o, "_h", o) for o in objs])
        return lib.bohip_gp_score_mom(hs, len(objs) if M is None else M, ptr(fr), fr.shape[1], ptr(ref), ptr(x), R, ptr(out), None, None, None, None)

    assert sc() == _lib.OK and sc(objs=(a, None, c_)) == _lib.E_ARG and sc(x=None) == _lib.E_ARG and sc(M=1) == _lib.E_ARG and sc(M=5) == _lib.E_ARG
    assert lib.bohip_gp_score_mom(None, 3, ptr(good), 3, ptr(ref), ptr(xs), R, ptr(out), None, None, None, None) == _lib.E_ARG
    other, empty = bohip.ElasticGPE(4), bohip.ElasticGPE(3)
    assert sc(objs=(a, b_, other)) == _lib.E_ARG and b"dimension" in lib.bohip_last_error()
    assert sc(objs=(a, empty, c_)) == _lib.E_STATE and sc(objs=(empty, b_, c_)) == _lib.E_STATE
    if lib.bohip_device_count() > 1:
        far = bohip.ElasticGPE(3, device=1)
        assert sc(objs=(a, b_, far)) == _lib.E_ARG and b"device" in lib.bohip_last_error()
        far.close()
    for m in (a, b_, c_, other, empty):
        m.close()


# ---- 7. the loop -----------------------------------------------------------------------------------------------------------------------
def test_bopt_with_three_quadratic_objectives(bohip):
    """d = 3, f_m = -|x - a_m|^2 for three centres, 8 initial points and 15 iterations with "refine": 3, against a fixed reference
    point: the hypervolume of the observations never decreases, ends above its value after the initial design, and every proposal
    lies inside the bounds."""
    centres = np.array([[0.2, 0.3, 0.5], [0.8, 0.7, 0.4], [0.3, 0.8, 0.8]])
    ref = np.array([-1.5, -1.5, -1.5])
    seen, hvs = [], []

    def func(x):
        y = tuple(-float(np.sum((x - c) ** 2)) for c in centres)
        seen.append((np.array(x), y))
        hvs.append(qr.front(np.array([s[1] for s in seen]).T, ref)[1])
        return y

    mk = lambda: bohip.ElasticGPE(3, mean=bohip.MeanConst(-0.4), kernel=bohip.SEArd(np.full(3, -0.3), -0.7), logNoise=-4.0,   # noqa: E731
                                  capacity=32)
    mo = bohip.ManyObjectiveGPE((mk(), mk(), mk()), ref=ref)
    o = bohip.BOpt(func, mo, bohip.ExpectedHypervolumeImprovement(), bohip.NoModelOptimizer(), [0.0] * 3, [1.0] * 3, sense=bohip.Max,
                   maxiterations=23, initializer_iterations=8, verbosity=bohip.Silent, rng=np.random.default_rng(11),
                   acquisitionoptions=dict(maxeval=512, refine=3))
    res = bohip.boptimize_(o)
    X = np.array([s[0] for s in seen])
    assert len(seen) == 23 and np.all(X >= 0.0) and np.all(X <= 1.0) and mo.nobs == 23
    assert all(b >= a for a, b in zip(hvs, hvs[1:])), hvs
    print(f"hypervolume after the initial design {hvs[7]:.6g}, at the end {hvs[-1]:.6g}; {sum(b > a for a, b in zip(hvs[7:], hvs[8:]))} of 15 "
          f"proposals improved it; the front has {res['observed_front']['y'].shape[1]} points")
    assert hvs[-1] > hvs[7]
    assert res["hypervolume"] == hvs[-1] == mo.hypervolume and res["observed_optimum"] is None
    tf, _ = qr.front(np.array([s[1] for s in seen]).T, ref)
    np.testing.assert_array_equal(res["observed_front"]["y"], tf)
    np.testing.assert_array_equal(res["ref"], ref)
    mo.close()
