"""The knowledge gradient over a candidate set on the device (bohip_gp_kg / bohip_kg_lines, ElasticGPE.kg / kg_lines,
KnowledgeGradient through acquisitionfunction, acquire_max and BOpt).

References: tests/kg_reference.py -- kg_march, the NumPy twin of the contract of include/bohip_kg.h (the sequence of lines, nseg
and the products of every term are the device's bit for bit; exp and erfc are libm's there and the device's here), and kg_hull, the
independent sorted-hull form, on the oracle's posterior.

Tolerances (profiles/kg_ab.txt).  TWIN_REL: 16 x the largest |device - twin| / twin measured on an MI355X over the
kg_lines cases of this file, 2.249e-15 (normal, R = E = 2) -- the device's exp / erfc against libm's; the end-to-end cases, held to
the same figure, measured 5.9e-16 (SEArd) and 3.4e-15 (Mat32Ard).  The project's parity bar of 1e-10 is the cap it must stay
under.  ORACLE_ABS: 16 x the largest |device - kg_hull(oracle's mu, Sigma)| / max(1, max|mu|) measured the same way, 1.694e-15
(Mat32Ard; SEArd 1.3e-16); cap 1e-10."""
import math

import numpy as np
import pytest

import kg_reference as kr
from conftest import synth
from test_parity_gpu import bohip  # noqa: F401  (fixture)
from test_qei_gpu import LNOISE, empty_model, model_of

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TWIN_REL = 16 * 2.249e-15
ORACLE_ABS = 16 * 1.694e-15
assert TWIN_REL <= 1e-10 and ORACLE_ABS <= 1e-10
NU = math.exp(2.0 * LNOISE) + EPS                                       # what the model has on the diagonal of cK (no jitter step)


def twin_of(a, B):
    out = [kr.kg_march(a, row) for row in np.atleast_2d(B)]
    return np.array([v for v, _ in out]), np.array([n for _, n in out], dtype=np.int32)


def check_against_twin(kg, nseg, tkg, tseg, what):
    np.testing.assert_array_equal(nseg, tseg, err_msg=what)
    pos = tkg > 0
    np.testing.assert_array_equal(kg[~pos], tkg[~pos], err_msg=what)   # a twin of exactly 0 is a device of exactly 0
    rel = float(np.max(np.abs(kg[pos] - tkg[pos]) / tkg[pos])) if pos.any() else 0.0
    print(f"  {what}: worst |device - twin| / twin = {rel:.3e}")
    assert rel <= TWIN_REL, what
    assert np.all(kg >= 0.0)
    return rel


def lines_of(kind, R, E, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal(R), rng.standard_normal((E, R))
    if kind == "quarter":                                               # ties everywhere: equal slopes, equal z, equal everything
        return np.round(rng.standard_normal(R) * 4) / 4, np.round(rng.standard_normal((E, R)) * 4) / 4
    b = np.linspace(-1.0, 1.0, R)                                       # the parabola: every line is on the envelope
    return -b * b, np.stack([b * (1.0 + 0.25 * e) for e in range(E)])


# ---- 1. kg_lines against the twin over the edges of the mapping -----------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 257, 1025])
def test_lines_match_the_twin(bohip, R):
    m = empty_model(bohip)                                              # the handle supplies the device and the stream only
    for E in sorted({1, min(R, 5)}):
        for kind in ("normal", "quarter") + (("parabola",) if R in (257, 1025) else ()):
            a, B = lines_of(kind, R, E, 100 * R + E)
            kg, nseg = m.kg_lines(a, B)
            tkg, tseg = twin_of(a, B)
            check_against_twin(kg, nseg, tkg, tseg, f"{kind} R = {R} E = {E}")
            if kind == "parabola":
                assert np.all(nseg == R - 1)
    m.close()


# ---- 2. crafted lines -----------------------------------------------------------------------------------------------------------
def test_crafted_lines(bohip):
    m = empty_model(bohip)
    nan, inf = math.nan, math.inf
    kg, nseg = m.kg_lines([0, 0, 0], [-1, 0, 1])
    assert nseg.tolist() == [1] and kg[0] == pytest.approx(0.7978845608028654, rel=TWIN_REL)
    kg, nseg = m.kg_lines([1.0, 3.0, 2.0], [0.5, 0.5, 0.5])           # equal slopes
    assert kg.tolist() == [0.0] and nseg.tolist() == [0]
    kg, nseg = m.kg_lines([2.5], [-0.3])                                # one line
    assert kg.tolist() == [0.0] and nseg.tolist() == [0]
    kg, nseg = m.kg_lines([0, 1, 0], [-1, 0, 1])
    assert nseg.tolist() == [2] and kg[0] == pytest.approx(0.16663094117537258, rel=TWIN_REL)
    a, b = [0, nan, 1, 5.0, 0, inf, 7.0], [-1, 9.0, 0, nan, 1, 0.5, -inf]                   # NaN / Inf lines are ignored
    kg2, nseg2 = m.kg_lines(a, b)
    assert kg2.tobytes() == kg.tobytes() and nseg2.tolist() == [2]
    kg, nseg = m.kg_lines([nan, 1.0], [0.0, inf])                       # ... and none is left
    assert kg.tolist() == [0.0] and nseg.tolist() == [0]
    b = np.linspace(-1.0, 1.0, 257)
    kg, nseg = m.kg_lines(-b * b, b)
    assert nseg.tolist() == [256]
    s = 1e100                                                           # the deep tail: z = 40, h(-40) ~ 9.1e-352 on its own
    kg, nseg = m.kg_lines([0.0, -40.0 * s], [0.0, s])
    t, _ = kr.kg_march([0.0, -40.0 * s], [0.0, s])                      # (checked against 60 digits in tests/test_kg_host.py)
    assert nseg.tolist() == [1] and 0.0 < kg[0] < inf and kg[0] == pytest.approx(t, rel=TWIN_REL)
    kg, _ = m.kg_lines([0.0, -11.0], [0.0, 1.0])                        # a KG of 1e-29 keeps its relative accuracy
    assert kg[0] == pytest.approx(kr.kg_march([0.0, -11.0], [0.0, 1.0])[0], rel=TWIN_REL)
    m.close()


# ---- 3. bohip_gp_kg end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["SEArd", "Mat32Ard"])
def test_gp_kg_end_to_end(bohip, orc, kern):
    from test_joint_gpu import posterior

    m, Xs, y = model_of(bohip, kern)
    R = 600
    xs = np.asfortranarray(Xs[:, :R])
    before = [v.tobytes() for v in m.predict_f(xs[:, :64])]
    mu, cov = m.predict_cov(xs)
    res = m.kg(xs)
    assert res.values.shape == (R,) and res.nseg.dtype == np.int32
    assert res.mu.tobytes() == mu.tobytes()                             # mu is predict_cov's, bit for bit
    # the twin on the device's own posterior: b_j = Sigma_je / sqrt(Sigma_ee + nu)
    B = np.stack([cov[e] / math.sqrt(cov[e, e] + NU) for e in range(R)])
    tkg, tseg = twin_of(mu, B)
    check_against_twin(res.values, res.nseg, tkg, tseg, f"{kern} R = E = {R}")
    assert res.best_idx == int(np.argmax(tkg)) and res.best_val == res.values[res.best_idx]
    print(f"  {kern}: segments per point {res.nseg.min()} .. {res.nseg.max()}, mean {res.nseg.mean():.1f}; KG max {res.values.max():.3e}")
    few = m.kg(xs, 7)                                                   # E = 7: the first 7 of the E = 600 call, bit for bit
    assert few.values.tobytes() == res.values[:7].tobytes() and few.nseg.tolist() == res.nseg[:7].tolist()
    assert few.mu.tobytes() == mu.tobytes() and few.best_idx == int(np.argmax(res.values[:7]))
    values, nseg, mu2, bv, bi = res                                     # iterable, as QEIBatch
    assert values is res.values and bi == res.best_idx
    # the independent form on the reference's posterior
    X, yy, _ = synth(300, 4, 1500, seed=31)
    mu_o, cov_o, _ = posterior(orc, kern, X, yy, np.full(4, -0.4), xs.T)
    hull = np.array([kr.kg_hull(mu_o, cov_o[e] / math.sqrt(cov_o[e, e] + NU))[0] for e in range(R)])
    err = float(np.max(np.abs(res.values - hull))) / max(1.0, float(np.abs(mu_o).max()))
    print(f"  {kern}: worst |device - hull(oracle)| / max(1, max|mu|) = {err:.3e}")
    assert err <= ORACLE_ABS
    f = bohip.acquisitionfunction(bohip.KnowledgeGradient(), m)         # the acquisition function is the same call
    assert f(xs).tobytes() == res.values.tobytes()
    assert [v.tobytes() for v in m.predict_f(xs[:, :64])] == before     # the model is unchanged


# ---- 4. edges and errors --------------------------------------------------------------------------------------------------------
def test_edges_and_errors(bohip):
    from bohip import _lib

    m, Xs, y = model_of(bohip, "SEArd")
    one = m.kg(Xs[:, :1])                                               # R = 1: nothing to learn about a maximum of one
    assert one.values.tolist() == [0.0] and one.nseg.tolist() == [0] and (one.best_val, one.best_idx) == (0.0, 0)
    for call in (lambda: m.kg(Xs[:, :10], 11), lambda: m.kg_lines(np.zeros(3), np.zeros((4, 3))),      # E > R
                 lambda: m.kg(Xs[:, :10], 0), lambda: m.kg_lines(np.zeros(3), np.zeros((0, 3)))):      # E < 1
        with pytest.raises(_lib.BohipError) as e:
            call()
        assert e.value.code == _lib.E_ARG
    big = np.zeros((4, _lib.KG_RMAX + 1), order="F")                    # refused before anything is allocated for it
    with pytest.raises(_lib.BohipError, match=r"kg: R exceeds BOHIP_KG_RMAX \(8192\)") as e:
        m.kg(big, 1)
    assert e.value.code == _lib.E_UNSUPPORTED
    lib = _lib.load()
    import ctypes as C
    dp = C.POINTER(C.c_double)
    z, out = np.zeros(4), np.zeros(1)
    rc = lib.bohip_kg_lines(m._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), _lib.KG_RMAX + 1, 1, out.ctypes.data_as(dp), None)
    assert rc == _lib.E_UNSUPPORTED and b"8192" in lib.bohip_last_error()
    empty = empty_model(bohip)
    with pytest.raises(_lib.BohipError) as e:
        empty.kg(Xs[:, :10])
    assert e.value.code == _lib.E_STATE
    kg, nseg = empty.kg_lines([0, 0, 0], [-1, 0, 1])                    # ... while the march alone needs no observations
    assert nseg.tolist() == [1]
    empty.close()
    ok = m.kg(Xs[:, :10])                                               # the handle works on
    assert ok.values.shape == (10,) and ok.best_idx >= 0


# ---- 5. the BO loop -------------------------------------------------------------------------------------------------------------
def test_bopt_loop_with_the_knowledge_gradient(bohip):
    from test_bo_loop_gpu import branin

    lb, ub = [-5.0, 0.0], [10.0, 15.0]
    model = bohip.ElasticGPE(2, mean=bohip.MeanConst(-10.0), kernel=bohip.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=64)
    opt = bohip.BOpt(lambda x: branin(x), model, bohip.KnowledgeGradient(), bohip.NoModelOptimizer(), lb, ub, sense=bohip.Min,
                     verbosity=bohip.Silent, rng=np.random.default_rng(5), maxiterations=13, initializer_iterations=10)
    assert opt.acquisitionoptions == dict(method="LD_LBFGS", restarts=1, maxeval=1024)
    calls, real = [], model.kg
    model.kg = lambda xs, n_eval=None: (calls.append(np.asarray(xs).shape), real(xs, n_eval))[1]
    bohip.boptimize_(opt)
    assert len(model.y) == 13 and calls == [(2, 1024)] * 3              # three proposals, one kg call each
    new = model.x[:, 10:]
    assert np.all(new >= np.array(lb)[:, None]) and np.all(new <= np.array(ub)[:, None])
    assert len({tuple(c) for c in new.T}) == 3
    model.close()
