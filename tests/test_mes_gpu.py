"""Max-value entropy search over a candidate set on the device (bohip_gp_mes / bohip_mes_values / bohip_mes_gumbel, ElasticGPE.mes /
mes_values / mes_gumbel, MaxValueEntropySearch through acquisitionfunction, acquire_max and BOpt).

References: tests/mes_reference.py -- the float64 twin of the contract of include/bohip_mes.h and its mpmath evaluator.

Tolerances.  REL = 1e-10, the project's parity bar (README), for the functor against mpmath and against the twin, with an absolute
floor of 1e-300 where u underflows.  The quantiles and max values of the Gumbel mode: the derived bounds of
mes_reference.quantile_bounds / maxval_bounds (the final bracket, the probes' rounding, the rounding of the sum S moved through its
slope).  The figures an MI355X gave are in DESIGN.md 6o."""
import ctypes as C
import math

import numpy as np
import pytest

import mes_reference as mr
from conftest import synth, var_tol
from test_parity_gpu import bohip, mu_floor  # noqa: F401  (fixture)
from test_qei_gpu import empty_model

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
REL, TINY = 1e-10, 1e-300
_cache = {}


def rel_err(dev, ref):
    """worst |dev - ref| / (|ref| + TINY / REL): <= REL means |dev - ref| <= REL |ref| + TINY."""
    return float(np.max(np.abs(dev - ref) / (np.abs(ref) + TINY / REL))) if np.size(dev) else 0.0


# ---- 1. bohip_mes_values ----------------------------------------------------------------------------------------------------------
def sweep(R, K):
    """gamma over [-60, 38] on a half-integer grid, exact in float64: candidates below every max value (gamma >= 0) and above every
    max value (gamma <= 0), so that the K terms of a partial have one sign; sigma in {1/2, 1, 2}."""
    mv = np.array([(k % 17) * 0.5 for k in range(K)])                       # 0 .. 8
    j = np.arange(R)
    s2 = np.array([1.0, 0.25, 4.0])[j % 3] if R > 1 else np.array([1.0])
    sd = np.sqrt(s2)
    below = -(np.round(np.linspace(0.0, 60.0, R)) * 0.5) * sd               # gamma = (m - mu) / sd in [0, 30 + 16]
    above = 8.0 + (np.round(np.linspace(0.0, 104.0, R)) * 0.5) * sd         # gamma in [-60, 0]
    mu = np.where(j % 2 == 0, above, below) if R > 1 else np.array([12.0])  # (R = 1: gamma in [-12, -4])
    return mu, s2, mv


def mp_values(mu, s2, mv):
    """MES and its partials from mpmath: every distinct gamma once (the grid makes gamma exact), the K terms added by fsum."""
    table = _cache.setdefault("mp", {})
    out = np.empty((3, mu.size))
    for j in range(mu.size):
        sd = math.sqrt(s2[j])
        us, ds = [], []
        for m in mv:
            g = (m - mu[j]) / sd
            assert g * sd + mu[j] == m                                       # exact
            if g not in table:
                table[g] = (float(mr.mp_u(g)), float(mr.mp_dudg(g)))
            us.append(table[g][0])
            ds.append((table[g][1], g))
        out[0, j] = math.fsum(us) / mv.size
        out[1, j] = math.fsum(-d / sd for d, _ in ds) / mv.size
        out[2, j] = math.fsum(-d * g / (2.0 * s2[j]) for d, g in ds) / mv.size
    return out


@pytest.mark.parametrize("R", [1, 255, 257])
@pytest.mark.parametrize("K", [1, 2, 33, 1024])
def test_values_match_mpmath_and_the_twin(bohip, R, K):
    m = empty_model(bohip)                                                  # the handle supplies the device and the stream only
    mu, s2, mv = sweep(R, K)
    val, dmu, ds2, bv, bi = m.mes_values(mu, s2, mv, want_grad=True)
    ref = mp_values(mu, s2, mv)
    errs = [rel_err(val, ref[0]), rel_err(dmu, ref[1]), rel_err(ds2, ref[2])]
    tw = mr.values(mu, s2, mv)
    terr = [rel_err(val, tw[0]), rel_err(dmu, tw[1]), rel_err(ds2, tw[2])]
    print(f"  R = {R} K = {K}: worst relative error against mpmath: value {errs[0]:.3e}, d/dmu {errs[1]:.3e}, d/ds2 {errs[2]:.3e}; "
          f"against the twin {max(terr):.3e}")
    assert max(errs) <= REL and max(terr) <= REL
    assert (bv, bi) == mr.record(val)
    only, bv2, bi2 = m.mes_values(mu, s2, mv)                               # without the partials: the same values
    assert only.tobytes() == val.tobytes() and (bv2, bi2) == (bv, bi)
    m.close()


def test_values_edges(bohip):
    m = empty_model(bohip)
    nan, inf = math.nan, math.inf
    # gamma = +-1e-9, +-4 and the neighbours of the switch, one max value
    mu = np.array([1e-9, -1e-9, 4.0, -4.0, math.nextafter(4.0, 0.0), math.nextafter(4.0, 8.0), 0.0, -37.0, 60.0])
    val, dmu, ds2, _, _ = m.mes_values(mu, np.ones(mu.size), [0.0], want_grad=True)
    want = np.array([[float(mr.mp_u(-x)), float(-mr.mp_dudg(-x)), float(-mr.mp_dudg(-x) * (-x) / 2.0)] for x in mu]).T
    errs = [rel_err(val, want[0]), rel_err(dmu, want[1]), rel_err(ds2, want[2])]
    print(f"  edges: worst relative error against mpmath: value {errs[0]:.3e}, d/dmu {errs[1]:.3e}, d/ds2 {errs[2]:.3e}")
    assert max(errs) <= REL
    assert val[3] < 1e-3 and val[7] > 0.0                                    # gamma = 4 and 37: small, positive, not cancelled
    # sigma^2 = 0, and entries that are not finite
    mu = np.array([0.3, 0.5, nan, 0.1, 0.2, inf, 0.4])
    s2 = np.array([0.0, 1.0, 1.0, inf, -1.0, 1.0, nan])
    val, dmu, ds2, bv, bi = m.mes_values(mu, s2, [0.7, 1.1], want_grad=True)
    assert (val[0], dmu[0], ds2[0]) == (0.0, 0.0, 0.0)
    assert np.isfinite([val[1], dmu[1], ds2[1]]).all() and val[1] > 0.0
    for a in (val, dmu, ds2):
        assert np.isnan(a[2:]).all()
    assert (bv, bi) == (val[1], 1) == mr.record(val)
    tw = mr.values(mu, s2, [0.7, 1.1])
    np.testing.assert_array_equal(np.isnan(val), np.isnan(tw[0]))
    val, bv, bi = m.mes_values(mu, s2, [0.7, inf])                           # a max value that is not finite: every term is NaN
    assert np.isnan(val).all() and (bv, bi) == (-inf, -1)
    val, bv, bi = m.mes_values([nan, nan, nan], [1.0, 1.0, 1.0], [0.5])      # an all-NaN batch
    assert np.isnan(val).all() and (bv, bi) == (-inf, -1)
    val, bv, bi = m.mes_values([0.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.5])   # the FIRST maximum wins
    assert val[1] == val[2] and (bv, bi) == (val[1], 1)
    m.close()


def test_batch_equals_single(bohip):
    """A candidate's value depends on (mu_j, s2_j, m) alone, bit for bit: not on R, not on its position."""
    m = empty_model(bohip)
    mu, s2, mv = sweep(257, 33)
    val, dmu, ds2, _, _ = m.mes_values(mu, s2, mv, want_grad=True)
    for j in (0, 1, 63, 64, 255, 256):
        v1, a1, b1, bv, bi = m.mes_values(mu[j:j + 1], s2[j:j + 1], mv, want_grad=True)
        assert (v1[0], a1[0], b1[0]) == (val[j], dmu[j], ds2[j]) and (bv, bi) == (val[j], 0)
    perm = np.random.default_rng(3).permutation(257)
    vp, _, _ = m.mes_values(mu[perm], s2[perm], mv)
    assert vp.tobytes() == val[perm].tobytes()
    m.close()


# ---- 2. bohip_mes_gumbel ----------------------------------------------------------------------------------------------------------
def candidates(kind, R, seed):
    rng = np.random.default_rng(seed)
    mu, var = rng.standard_normal(R), rng.uniform(0.01, 2.0, R)
    if kind == "flat":
        var[:] = 0.0
    elif kind == "some_flat":
        var[rng.random(R) < 0.3] = 0.0
        if R == 1:
            var[:] = 0.0
    elif kind == "offset":
        mu, var = 1e3 + 1e-3 * mu, 1e-6 * var
    return mu, var


def check_gumbel(q, mv, mu, var, K, seed, floor, what):
    tq, tm = mr.maxvals(mu, var, K, seed, floor)
    lo0, hi0 = mr.bracket(mu, var)
    if hi0 == lo0:                                                          # every sigma is 0: exact
        assert q.tolist() == [lo0] * 3 and mv.tolist() == [max(lo0, floor)] * K, what
        return 0.0, 0.0
    qb = mr.quantile_bounds(mu, var, tq)
    mb = mr.maxval_bounds(qb, seed, K, tm)
    share_q, share_m = float(np.max(np.abs(q - tq) / qb)), float(np.max(np.abs(mv - tm) / mb))
    print(f"  {what}: worst share of the bound: quantiles {share_q:.3f}, max values {share_m:.3f}  (y = {q}, bounds {qb})")
    assert np.all(np.abs(q - tq) <= qb) and np.all(np.abs(mv - tm) <= mb), what
    assert q[0] <= q[1] <= q[2] and lo0 <= q[0] and q[2] <= hi0
    return share_q, share_m


@pytest.mark.parametrize("R", [1, 2, 257, 4097, 8193])                      # (8193: the sum S in two slices of workgroups)
def test_gumbel_max_values(bohip, R):
    m = empty_model(bohip)
    K = 16
    for kind in ("random", "flat", "some_flat", "offset"):
        mu, var = candidates(kind, R, 40 * R + len(kind))
        q, mv = m.mes_gumbel(mu, var, samples=K, seed=11)
        check_gumbel(q, mv, mu, var, K, 11, -math.inf, f"{kind} R = {R}")
        q2, mv2 = m.mes_gumbel(mu, var, samples=K, seed=11)                  # two calls, identical bits
        assert q2.tobytes() == q.tobytes() and mv2.tobytes() == mv.tobytes()
        qf, mf = m.mes_gumbel(mu, var, samples=K, seed=11, floor=float(mv.max()) + 1.0)   # a floor above every sample
        assert qf.tobytes() == q.tobytes() and mf.tolist() == [float(mv.max()) + 1.0] * K
        part = float(np.sort(mv)[K // 2])                                    # ... and one between them
        _, mp_ = m.mes_gumbel(mu, var, samples=K, seed=11, floor=part)
        assert mp_.tobytes() == np.maximum(mv, part).tobytes()
    if R == 1:                                                              # the closed form: y_p = mu + sigma Phi^-1(p)
        q, _ = m.mes_gumbel([0.25], [4.0], samples=1, seed=0)
        want = 0.25 + 2.0 * np.array([-0.6744897501960817, 0.0, 0.6744897501960817])
        assert np.all(np.abs(q - want) <= mr.quantile_bounds([0.25], [4.0], want))
    mu, var = candidates("random", 257, 5)
    mu[3], var[9], var[20] = math.nan, math.inf, -1.0                        # candidates that are not finite take no part
    keep = np.ones(257, dtype=bool)
    keep[[3, 9, 20]] = False
    q, mv = m.mes_gumbel(mu, var, samples=4, seed=2)
    q2, mv2 = m.mes_gumbel(mu[keep], var[keep], samples=4, seed=2)
    check_gumbel(q, mv, mu[keep], var[keep], 4, 2, -math.inf, "not finite R = 257")
    assert np.all(np.abs(q - q2) <= 2.0 * mr.quantile_bounds(mu[keep], var[keep], q2))   # (both within the bound of the root)
    m.close()


# ---- 3. bohip_gp_mes end to end -------------------------------------------------------------------------------------------------
def model_and_posterior(bohip, orc, kern, N, d):
    """One model per (kernel, N, d), its 600 candidates and the reference's posterior of them."""
    import test_joint_gpu as tj

    key = (kern, N, d)
    if key not in _cache:
        X, y, Xs = synth(N, d, 600, seed=7 * N + d)
        ll = np.full(d, -0.4)
        m = bohip.ElasticGPE(d, mean=bohip.MeanConst(tj.BETA), kernel=getattr(bohip, kern)(ll, tj.LSIG), logNoise=tj.LNOISE, capacity=N)
        m.append_(X.T, y)
        mu_o, cov_o, alpha = tj.posterior(orc, kern, X, y, ll, Xs)
        _cache[key] = (m, np.asfortranarray(Xs.T), mu_o, np.maximum(np.diag(cov_o), 0.0), alpha, tj.S2F)
    return _cache[key]


@pytest.mark.parametrize("kern", ["SEArd", "Mat32Ard"])
@pytest.mark.parametrize("N", [60, 300])
@pytest.mark.parametrize("d", [2, 8, 17])
def test_gp_mes_end_to_end(bohip, orc, kern, N, d):
    m, xs, mu_o, var_o, alpha, s2f = model_and_posterior(bohip, orc, kern, N, d)
    factor, al = m.factor().tobytes(), m.alpha().tobytes()
    for K in (1, 16):
        res = m.mes(xs, samples=K, seed=5 + K)
        assert res.values.shape == (600,) and res.maxvals.shape == (K,) and (res.jitter, res.tries) == (0.0, 0)
        # the posterior against the reference, at test_parity_gpu's tolerances
        assert np.all(np.abs(res.mu - mu_o) <= 1e-6 * np.abs(mu_o) + mu_floor(alpha, s2f))
        assert np.all(np.abs(res.var - var_o) <= var_tol(var_o, N, s2f))
        # the values against the twin at the device's own (mu, var, maxvals)
        tw = mr.values(res.mu, res.var, res.maxvals)[0]
        err = rel_err(res.values, tw)
        sq, sm = check_gumbel(res.quantiles, res.maxvals, res.mu, res.var, K, 5 + K, -math.inf, f"{kern} N = {N} d = {d} K = {K}")
        print(f"  {kern} N = {N} d = {d} K = {K}: worst |device - twin| / twin of the values {err:.3e}")
        assert err <= REL
        assert (res.best_val, res.best_idx) == mr.record(res.values) and res.best_idx == mr.record(tw)[1]
        assert np.all(res.values >= 0.0)
    values, maxvals, quantiles, mu, var, bv, bi = res                        # iterable, as KGResult
    assert values is res.values and bi == res.best_idx
    fl = float(np.max(m.y))
    floored = m.mes(xs, samples=16, seed=21, floor=fl)                       # the floor: the best observation
    assert np.all(floored.maxvals >= fl) and floored.quantiles.tobytes() == res.quantiles.tobytes()
    f = bohip.acquisitionfunction(bohip.MaxValueEntropySearch(16), m, rng=np.random.default_rng(1))
    seed = int(np.random.default_rng(1).integers(0, 2**63))
    assert f(xs).tobytes() == m.mes(xs, samples=16, seed=seed).values.tobytes()   # the acquisition function is the same call
    assert m.factor().tobytes() == factor and m.alpha().tobytes() == al      # the model is unchanged


def test_joint_mode(bohip, orc):
    m, xs, *_ = model_and_posterior(bohip, orc, "SEArd", 300, 8)
    xs = np.asfortranarray(xs[:, :200])
    js = m.sample_joint(xs, S=8, seed=17, jitter=1e-12, max_tries=40)
    res = m.mes(xs, samples=8, mode="joint", seed=17, jitter_rel=1e-12, max_tries=40)
    assert res.maxvals.tobytes() == js.samples.max(axis=1).tobytes()         # the row maxima of the same draws, bit for bit
    assert (res.jitter, res.tries) == (js.jitter, js.tries)
    assert np.isnan(res.quantiles).all()
    assert res.mu.tobytes() == js.mu.tobytes()
    tw = mr.values(res.mu, res.var, res.maxvals)[0]
    assert rel_err(res.values, tw) <= REL and (res.best_val, res.best_idx) == mr.record(res.values)
    fl = float(np.sort(js.samples.max(axis=1))[4])
    floored = m.mes(xs, samples=8, mode="joint", seed=17, floor=fl)
    assert floored.maxvals.tobytes() == np.maximum(js.samples.max(axis=1), fl).tobytes()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------
def test_errors(bohip, orc):
    from bohip import _lib

    m, xs, *_ = model_and_posterior(bohip, orc, "SEArd", 60, 2)
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    z, out = np.zeros(8), np.zeros(8)
    pz, po = z.ctypes.data_as(dp), out.ctypes.data_as(dp)
    inf = math.inf

    def gp_mes(h, R, K, mode=0, floor=-inf, xs_=pz, mes=po):
        return lib.bohip_gp_mes(h, xs_, R, K, mode, 0, floor, 1e-12, 40, mes, None, None, None, None, None, None, None)

    V, G = lib.bohip_mes_values, lib.bohip_mes_gumbel
    for call, word in [(lambda: gp_mes(m._h, 0, 1), b"at least 1"), (lambda: gp_mes(m._h, 2, 0), b"at least 1"),
                       (lambda: gp_mes(None, -1, 1), b"at least 1"),                            # sizes before null pointers
                       (lambda: gp_mes(m._h, 2, 2, mode=2), b"unknown mode"), (lambda: gp_mes(None, 2, 2), b"null"),
                       (lambda: gp_mes(m._h, 2, 2, xs_=None), b"null"), (lambda: gp_mes(m._h, 2, 2, mes=None), b"null"),
                       (lambda: gp_mes(m._h, 2, 2, floor=math.nan), b"NaN"),
                       (lambda: V(m._h, pz, pz, 0, pz, 1, po, None, None, None), b"at least 1"),
                       (lambda: V(m._h, pz, pz, 2, pz, 0, po, None, None, None), b"at least 1"),
                       (lambda: V(m._h, pz, None, 2, pz, 1, po, None, None, None), b"null"),
                       (lambda: V(None, pz, pz, 2, pz, 1, po, None, None, None), b"null"),
                       (lambda: V(m._h, pz, pz, 2, pz, 1, po, po, None, None), b"together"),
                       (lambda: V(m._h, pz, pz, 2, pz, 1, po, None, po, None), b"together"),
                       (lambda: G(m._h, pz, pz, 0, 1, 0, -inf, po, po), b"at least 1"),
                       (lambda: G(m._h, pz, pz, 2, 1, 0, -inf, None, po), b"null"),
                       (lambda: G(m._h, pz, pz, 2, 1, 0, -inf, po, None), b"null"),
                       (lambda: G(m._h, pz, pz, 2, 1, 0, math.nan, po, po), b"NaN")]:
        rc = call()
        assert rc == _lib.E_ARG and word in lib.bohip_last_error(), (rc, word, lib.bohip_last_error())
    # the limits, refused before anything is allocated (the pointers are never read)
    KX, RX = _lib.MES_KMAX + 1, _lib.MES_RMAX + 1
    for call, word in [(lambda: gp_mes(m._h, 2, KX), b"BOHIP_MES_KMAX (1024)"), (lambda: gp_mes(m._h, RX, 2), b"BOHIP_MES_RMAX (524288)"),
                       (lambda: V(m._h, pz, pz, 2, pz, KX, po, None, None, None), b"BOHIP_MES_KMAX (1024)"),
                       (lambda: V(m._h, pz, pz, RX, pz, 1, po, None, None, None), b"BOHIP_MES_RMAX (524288)"),
                       (lambda: G(m._h, pz, pz, 2, KX, 0, -inf, po, po), b"BOHIP_MES_KMAX (1024)"),
                       (lambda: G(m._h, pz, pz, RX, 1, 0, -inf, po, po), b"BOHIP_MES_RMAX (524288)")]:
        rc = call()
        assert rc == _lib.E_UNSUPPORTED and word in lib.bohip_last_error(), (rc, word, lib.bohip_last_error())
    with pytest.raises(_lib.BohipError, match=r"K exceeds BOHIP_MES_KMAX \(1024\)") as e:
        m.mes_values(np.zeros(3), np.ones(3), np.zeros(1025))
    assert e.value.code == _lib.E_UNSUPPORTED
    rc = gp_mes(m._h, 65536 + 1, 2, mode=1)                                  # joint mode beyond one chunk (65536 is the largest a model has)
    msg = lib.bohip_last_error()
    assert rc == _lib.E_UNSUPPORTED and b"one candidate chunk (" in msg and re_int(msg) >= 1024, (rc, msg)
    with pytest.raises(ValueError, match="mode must be"):
        m.mes(xs, mode="exact")
    empty = empty_model(bohip)
    with pytest.raises(_lib.BohipError) as e:
        empty.mes(np.zeros((4, 3)))
    assert e.value.code == _lib.E_STATE
    val, _, _ = empty.mes_values([0.0], [1.0], [1.0])                        # ... while the functor alone needs no observations
    assert val[0] > 0.0
    empty.close()
    ok = m.mes(xs[:, :10], samples=2)                                        # the handle works on
    assert ok.values.shape == (10,) and ok.best_idx >= 0


def re_int(msg):
    import re

    return int(re.search(rb"chunk \((\d+)\)", msg).group(1))


# ---- 5. the BO loop -------------------------------------------------------------------------------------------------------------
def test_bopt_loop_with_max_value_entropy_search(bohip):
    from test_bo_loop_gpu import branin

    lb, ub = [-5.0, 0.0], [10.0, 15.0]
    model = bohip.ElasticGPE(2, mean=bohip.MeanConst(-10.0), kernel=bohip.SEArd([0.0, 0.0], 5.0), logNoise=-2.0, capacity=64)
    opt = bohip.BOpt(lambda x: -branin(x), model, bohip.MaxValueEntropySearch(), bohip.NoModelOptimizer(), lb, ub, sense=bohip.Max,
                     verbosity=bohip.Silent, rng=np.random.default_rng(5), maxiterations=20, initializer_iterations=8)
    assert opt.acquisitionoptions == dict(method="LD_LBFGS", restarts=1, maxeval=1024)
    calls, real = [], model.mes
    model.mes = lambda xs, **kw: (calls.append((np.asarray(xs).shape, kw["samples"], kw["mode"], kw["seed"])), real(xs, **kw))[1]
    bohip.boptimize_(opt)
    assert len(model.y) == 20 and len(calls) == 12                          # 8 Sobol points, then 12 proposals, one mes call each
    assert all(c[:3] == ((2, 1024), 16, "gumbel") for c in calls) and len({c[3] for c in calls}) == 12
    new = model.x[:, 8:]
    assert new.shape[1] == 12 and np.all(new >= np.array(lb)[:, None]) and np.all(new <= np.array(ub)[:, None])
    assert opt.observed_optimum == np.max(model.y)
    model.close()
