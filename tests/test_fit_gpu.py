"""bohip_gp_mll_grad_batch (kernels_fit.hip: one workgroup per hyper-parameter setting) and the multi-start MAP fit on the device.

Shapes: N below, at and across the kernel's 16-wide blocks (1, 2, 17, 64, 65, 128, 200) and at its cap (512), one d from every
dimension bucket (1, 2 | 3 | 5, 8 | 17 | 33).  References: the NumPy twin (tests/matern_reference.py) for all eight kernels, the C
oracle for the three it has.  Tolerances are those of test_mll_gradient_vs_oracle: mll 1e-9 relative, gradient rtol 1e-6 with the
floor 1e-8 max|g_ref| (every entry is a sum of ~N^2/2 signed terms)."""
import ctypes as C
import math

import numpy as np
import pytest

import fit_reference as fr
from conftest import synth
from matern_reference import KERNELS, MaternGP
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ALL = list(KERNELS)
SHAPES = {(1, 1): ["SEArd", "Mat12Iso"], (2, 2): ["SEIso", "Mat32Ard"], (17, 3): ["Mat52Ard", "Mat12Ard", "Mat32Iso"], (65, 8): ALL,
          (128, 5): ["Mat32Iso", "SEArd", "Mat52Iso"], (200, 17): ["Mat52Iso", "Mat12Ard", "SEIso"], (64, 33): ["Mat32Ard", "Mat52Ard", "Mat12Iso"]}
CASES = [(k, N, d) for (N, d), ks in SHAPES.items() for k in ks]


def centre(kern, d):
    nl = 1 if KERNELS[kern][1] else d
    return np.concatenate([[-1.5, 0.2], np.full(nl, -0.6), [0.3]])          # [logNoise, mean, ll..., lsigma]


def settings(kern, d, H, seed):
    c = centre(kern, d)
    return c + np.random.default_rng(seed).uniform(-1, 1, (H, c.size))


def model_of(bohip, kern, X, y, theta=None, capacity=None):
    d = X.shape[1]
    t = centre(kern, d) if theta is None else theta
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(t[1]), kernel=getattr(bohip, kern)(t[2:-1], t[-1]), logNoise=t[0],
                         capacity=capacity or max(len(y), 1))
    m.append_(X.T, y)
    return m


def twin(kern, X, y, t):
    m, dn, dm, dk = MaternGP(kern, X, y, t[2:-1], t[-1], t[0], t[1]).mll_grad()
    return m, np.concatenate([[dn, dm], np.ravel(dk)])


def check_row(mll, g, mll_ref, g_ref, what):
    print(f"{what}: mll {mll:.12g} (ref {mll_ref:.12g}, rel {abs(mll - mll_ref) / abs(mll_ref):.2e}), "
          f"max |dg| / max|g_ref| {np.abs(g - g_ref).max() / np.abs(g_ref).max():.2e}")
    assert mll == pytest.approx(mll_ref, rel=1e-9)
    np.testing.assert_allclose(g, g_ref, rtol=1e-6, atol=1e-8 * np.abs(g_ref).max())


# ---- 1. parity over shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d", CASES)
def test_batch_matches_the_twin(bohip, kern, N, d):
    X, y, _ = synth(N, d, 1, seed=100 + N)
    m = model_of(bohip, kern, X, y)
    assert m.mll_batch_dims() == (centre(kern, d).size, 512)
    Theta = settings(kern, d, 3, seed=N + d)
    mll, G, piv = m.mll_grad_batch(Theta)
    assert np.all(piv == 0) and G.shape == Theta.shape
    for h in range(3):
        check_row(mll[h], G[h], *twin(kern, X, y, Theta[h]), f"{kern} N={N} d={d} row {h}")


def test_batch_at_the_size_cap(bohip):
    X, y, _ = synth(512, 8, 1, seed=9)
    m = model_of(bohip, "SEArd", X, y)
    Theta = settings("SEArd", 8, 2, seed=3)
    mll, G, piv = m.mll_grad_batch(Theta)
    assert np.all(piv == 0)
    for h in range(2):
        check_row(mll[h], G[h], *twin("SEArd", X, y, Theta[h]), f"SEArd N=512 row {h}")


@pytest.mark.parametrize("kern", ["SEArd", "Mat52Iso", "Mat32Ard", "Mat12Iso"])
def test_value_only(bohip, kern):
    X, y, _ = synth(65, 8, 1, seed=5)
    m = model_of(bohip, kern, X, y)
    Theta = settings(kern, 8, 3, seed=8)
    mll, G, piv = m.mll_grad_batch(Theta, want_grad=False)
    assert G is None and np.all(piv == 0)
    full = m.mll_grad_batch(Theta)[0]
    for h in range(3):
        assert mll[h] == pytest.approx(twin(kern, X, y, Theta[h])[0], rel=1e-9)
    np.testing.assert_array_equal(mll, full)          # the value does not depend on whether the gradient was asked for


@pytest.mark.parametrize("kern", ["SEArd", "SEIso", "Mat52Ard"])
def test_batch_matches_the_oracle(bohip, orc, kern):
    X, y, _ = synth(65, 8, 1, seed=21)
    m = model_of(bohip, kern, X, y)
    Theta = settings(kern, 8, 3, seed=4)
    mll, G, _ = m.mll_grad_batch(Theta)
    for h, t in enumerate(Theta):
        ll = t[2:-1] if t.size > 4 else float(t[2])
        mll_o, g_o = orc.mll_grad(X, y, ll, t[-1], t[0], t[1], kern=kern)
        check_row(mll[h], G[h], mll_o, g_o, f"{kern} oracle row {h}")


# ---- 2. against the resident path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,N,d", [("Mat52Ard", 200, 17), ("SEIso", 65, 8), ("Mat12Ard", 128, 5), ("Mat32Iso", 17, 3)])
def test_batch_matches_the_resident_path(bohip, kern, N, d):
    X, y, _ = synth(N, d, 1, seed=31)
    m, second = model_of(bohip, kern, X, y), model_of(bohip, kern, X, y)
    Theta = settings(kern, d, 3, seed=12)
    mll, G, _ = m.mll_grad_batch(Theta)
    for h, t in enumerate(Theta):
        second.set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
        r, dn, dm, dk = second.mll_grad()
        check_row(mll[h], G[h], r, np.concatenate([[dn, dm], dk]), f"{kern} N={N} resident row {h}")


# ---- 3. batch invariance, bit for bit ----------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_the_batch(bohip, monkeypatch):
    X, y, _ = synth(65, 8, 1, seed=2)
    m = model_of(bohip, "Mat52Ard", X, y)
    t = settings("Mat52Ard", 8, 1, seed=1)[0]
    others = settings("Mat52Ard", 8, 300, seed=6)
    alone = m.mll_grad_batch(t[None])
    first = m.mll_grad_batch(np.vstack([t, others[:2]]))
    big = np.vstack([others[:299], t])
    last = m.mll_grad_batch(big)                              # more workgroups than compute units
    monkeypatch.setenv("BOHIP_FIT_WS_MAX_MB", "1")            # 9 settings per launch: 34 consecutive launches inside the call
    chunked = m.mll_grad_batch(big)
    for res, row in ((first, 0), (last, 299), (chunked, 299)):
        assert res[0][row].tobytes() == alone[0][0].tobytes()
        assert res[1][row].tobytes() == alone[1][0].tobytes()
    assert chunked[0].tobytes() == last[0].tobytes() and chunked[1].tobytes() == last[1].tobytes()


# ---- 4. the model is untouched -----------------------------------------------------------------------------------------------------
def test_the_model_is_untouched(bohip):
    X, y, Xs = synth(140, 5, 64, seed=13)
    m = model_of(bohip, "Mat32Ard", X[:120], y[:120], capacity=256)

    def state():
        mu, var = m.predict_f(Xs.T)
        return mu.tobytes(), var.tobytes(), np.float64(m.mll()).tobytes(), m.alpha().tobytes(), m.info(2)

    Theta = settings("Mat32Ard", 5, 4, seed=3) + 0.5
    before = state()
    mll, _, piv = m.mll_grad_batch(Theta)
    assert np.all(piv == 0) and state() == before
    m.append_(X[120:].T, y[120:])                             # an incremental extension, no refit after it
    before = state()
    mll2, G2, _ = m.mll_grad_batch(Theta)
    assert state() == before
    for h in range(4):                                        # ... and the call saw the appended rows
        check_row(mll2[h], G2[h], *twin("Mat32Ard", X, y, Theta[h]), f"after append row {h}")


# ---- 5. failed rows ----------------------------------------------------------------------------------------------------------------
def test_failed_rows_stay_alone(bohip):
    X, y, _ = synth(65, 8, 1, seed=17)
    m = model_of(bohip, "SEArd", X, y)
    good = settings("SEArd", 8, 2, seed=5)
    nan_noise, inf_ll = good[0].copy(), good[1].copy()
    nan_noise[0] = math.nan
    inf_ll[4] = math.inf
    mll, G, piv = m.mll_grad_batch(np.vstack([good[0], nan_noise, inf_ll, good[1]]))
    assert piv[0] == 0 and piv[3] == 0 and piv[1] >= 1 and piv[2] >= 1
    assert np.all(mll[1:3] == -np.inf) and not G[1:3].any()
    for row, t in ((0, good[0]), (3, good[1])):
        alone = m.mll_grad_batch(t[None])
        assert mll[row].tobytes() == alone[0][0].tobytes() and G[row].tobytes() == alone[1][0].tobytes()
    # numerically singular: two observations twice, almost no noise, a large signal variance -- flagged or finite, never contagious
    Xd, yd = np.vstack([X, X[:2]]), np.concatenate([y, y[:2]])
    md = model_of(bohip, "SEArd", Xd, yd)
    sing = good[0].copy()
    sing[0], sing[-1] = -40.0, 3.0
    mll, G, piv = md.mll_grad_batch(np.vstack([good[0], sing, good[1]]))
    print("singular row: pivot", piv[1], "mll", mll[1])
    assert (piv[1] > 0 and mll[1] == -np.inf and not G[1].any()) or (piv[1] == 0 and np.isfinite(mll[1]))
    for row, t in ((0, good[0]), (2, good[1])):
        alone = md.mll_grad_batch(t[None])
        assert piv[row] == 0 and mll[row].tobytes() == alone[0][0].tobytes() and G[row].tobytes() == alone[1][0].tobytes()


# ---- 6. limits ---------------------------------------------------------------------------------------------------------------------
def test_limits(bohip):
    from bohip import _lib

    X, y, _ = synth(513, 2, 1, seed=1)
    m = model_of(bohip, "SEArd", X, y)
    with pytest.raises(bohip.BohipError) as e:
        m.mll_grad_batch(centre("SEArd", 2)[None])
    assert e.value.code == _lib.E_UNSUPPORTED and "512" in str(e.value)
    small = model_of(bohip, "SEArd", X[:5], y[:5])
    dp = C.POINTER(C.c_double)
    th, out = centre("SEArd", 2), np.zeros(1)
    assert small._lib.bohip_gp_mll_grad_batch(small._h, 0, th.ctypes.data_as(dp), out.ctypes.data_as(dp), None, None) == _lib.E_ARG
    assert small._lib.bohip_gp_mll_grad_batch(small._h, 1, None, out.ctypes.data_as(dp), None, None) == _lib.E_ARG
    empty = bohip.ElasticGPE(2)
    with pytest.raises(bohip.BohipError) as e:
        empty.mll_grad_batch(centre("SEArd", 2)[None])
    assert e.value.code == _lib.E_STATE


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------
def multimodal_model(bohip):
    X, y = fr.problem()
    return bohip.ElasticGPE.from_data(X.T, y, mean=bohip.MeanConst(fr.X0[1]), kernel=bohip.SEIso(fr.X0[2], fr.X0[3]), logNoise=fr.X0[0])


def test_multistart_fit_leaves_the_poor_basin(bohip):
    from bohip.bopt import MAPGPOptimizer, optimizemodel_

    bounds = dict(noisebounds=[-4, 2], meanbounds=[[-2], [2]], kernbounds=[[-4, -3], [3, 3]])
    m = multimodal_model(bohip)
    optimizemodel_(MAPGPOptimizer(every=1, restarts=fr.RESTARTS, seed=fr.SEED, **bounds), m)
    ref = fr.scipy_best().max()
    print("multi-start mll", m.mll(), "SciPy on the twin", ref)
    assert m.mll() > -11 and m.mll() >= ref - 1e-6 * abs(ref)
    one = multimodal_model(bohip)
    optimizemodel_(MAPGPOptimizer(every=1, **bounds), one)            # today's single search: the basin it starts in
    assert one.mll() < -13


def test_multistart_fit_beyond_the_size_cap_loops(bohip):
    from bohip.bopt import MAPGPOptimizer, optimizemodel_

    X, y, _ = synth(513, 2, 1, seed=3)
    m = model_of(bohip, "SEArd", X, y)
    m.fit_()
    start = m.mll()
    optimizemodel_(MAPGPOptimizer(every=1, restarts=2, seed=0, maxeval=4, noisebounds=[-4, 2], meanbounds=[[-2], [2]],
                                  kernbounds=[[-3, -3, -3], [3, 3, 3]]), m)
    assert math.isfinite(m.mll()) and m.mll() >= start
