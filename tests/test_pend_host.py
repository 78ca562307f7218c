"""Pending evaluations without a GPU (include/bohip_pend.h): the two CPU statements of tests/pend_reference.py against
each other, the non-vacuity of what the device tests compare, the ABI in every table that binds it, and the ask / tell bookkeeping
of BOpt on host models.

Bounds.  The device (tests/test_pend_gpu.py) is held to test_batch_gpu.compare's bounds against ``refit_per_fantasy``: values and mu
1e-6 relative + 64 eps s_f^2 sum|alpha| + 1e-12, s^2 conftest.var_tol.  ``recurrence`` claims to be that definition exactly, so here
it has to sit within a TENTH of those bounds.  The other way round the mistakes the device tests exist to catch -- the conditioning
dropped, nu or the refit's jitter left off Sigma_p, LogEI's logarithms averaged -- must lie at least 100 bounds away on the chosen
inputs, or the device tests could not tell them apart."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pend_reference as pr   # noqa: E402
from batch_reference import gp_factory   # noqa: E402
from conftest import ROOT, synth, var_tol   # noqa: E402

LL, LSIG, LNOISE, BETA = math.log(0.5), 0.0, -2.0, 0.0           # BASELINE recipe
S2F = math.exp(2 * LSIG)
WANT = {"bohip_gp_pending_set", "bohip_gp_pending_info", "bohip_gp_score_pending", "bohip_pend_values"}
SHAPES = [(17, 3, 1), (129, 3, 17), (300, 4, 32)]                # (N, d, p)
UCB_BETA = 30.0   # the non-vacuity inputs: an exploring UCB, whose best candidates are the uncertain ones
ACQS = ("EI", "PI", "UCB", "MI", "MaxMean", "LogEI")


def factory(kern, d, lnoise=LNOISE):
    return gp_factory(kern, np.array([LL]) if kern.endswith("Iso") else np.full(d, LL), LSIG, lnoise, BETA)


def params_of(acq, y):
    return {"EI": [float(y.max()) - 1.0], "PI": [float(y.max()) - 1.0], "LogEI": [float(y.max()) - 1.0], "UCB": [2.0], "MI": [1.0, 0.3],
            "MaxMean": []}[acq]


def inputs(N, d, p, R=64, S=3, seed=0, stress=None):
    X, y, Xs = synth(N, d, R, seed)
    rng = np.random.default_rng(1000 + seed)
    Xp = rng.random((p, d))
    if stress == "dup" and p >= 2:
        Xp[1] = Xp[0]
    if stress == "obs":
        Xp[p // 2] = X[N // 2]
    return X, y, Xs, Xp, rng.standard_normal((S, p))


def shares(got, ref, N):
    """How far `got` lies from `ref` in units of the device's bounds: (score, mu, var)."""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(ref["score"])
        assert np.array_equal(fin, np.isfinite(got["score"])) and np.array_equal(got["score"][~fin], ref["score"][~fin], equal_nan=True)
        return (float(np.max(np.abs(got["score"] - ref["score"])[fin] / pr.value_bound(ref["score"], S2F, ref["asum"])[fin], initial=0.0)),
                float(np.max(np.abs(got["mu"] - ref["mu"]) / pr.value_bound(ref["mu"], S2F, ref["asum"]))),
                float(np.max(np.abs(got["var"] - ref["var"]) / var_tol(ref["var"], N, S2F))))


# ---- 1. the two statements agree ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["SEArd", "Mat52Ard", "Mat12Iso"])
@pytest.mark.parametrize("N,d,p", SHAPES)
def test_recurrence_is_the_definition(kern, N, d, p):
    for stress in (None, "dup", "obs"):
        if stress == "dup" and p < 2:
            continue
        X, y, Xs, Xp, Z = inputs(N, d, p, stress=stress)
        for acq in ACQS:
            for raise_tau in (False, True):
                ref = pr.refit_per_fantasy(factory(kern, d), X, y, Xp, Xs, acq, params_of(acq, y), Z, raise_tau)
                got = pr.recurrence(factory(kern, d), X, y, Xp, Xs, acq, params_of(acq, y), Z, raise_tau)
                s = shares(got, ref, N + p)
                print(f"{kern} N={N} p={p} {stress} {acq} raise={raise_tau}: shares of the device's bounds {s[0]:.2e} {s[1]:.2e} {s[2]:.2e}")
                assert max(s) <= 0.1
    X, y, Xs, Xp, _ = inputs(N, d, p)                            # S = 0, the Kriging believer: z = 0
    Z0 = np.zeros((1, p))
    ref = pr.refit_per_fantasy(factory(kern, d), X, y, Xp, Xs, "UCB", [2.0], Z0)
    got = pr.recurrence(factory(kern, d), X, y, Xp, Xs, "UCB", [2.0], Z0)
    assert max(shares(got, ref, N + p)) <= 0.1
    assert np.max(np.abs(ref["each"][0] - (ref["mu"] + 2.0 * np.sqrt(ref["var"])))) <= 1e-9   # the mean stays, the variance shrinks


# ---- 2. non-vacuity ----------------------------------------------------------------------------------------------------------------
def _near_the_top(N, d, p, R=257):
    """Pending points ON the p best candidates of the unconditioned UCB score: the conditioning must move the arg-max away."""
    X, y, Xs = synth(N, d, R, 2)
    gp = factory("SEArd", d)(X, y)
    mu, var = gp.predict(Xs)
    top = np.argsort(-(mu + UCB_BETA * np.sqrt(var)), kind="stable")[:p]
    return X, y, Xs, Xs[top].copy(), np.random.default_rng(7).standard_normal((64, p))


@pytest.mark.parametrize("N,d,p", [(129, 3, 2), (300, 4, 17)])
def test_dropping_the_conditioning_is_visible(N, d, p):
    X, y, Xs, Xp, Z = _near_the_top(N, d, p)
    good = pr.recurrence(factory("SEArd", d), X, y, Xp, Xs, "UCB", [UCB_BETA], Z)
    bad = pr.recurrence(factory("SEArd", d), X, y, Xp, Xs, "UCB", [UCB_BETA], Z, condition=False)
    moved = np.max(np.abs(bad["var"] - good["var"]) / var_tol(good["var"], N + p, S2F))
    print(f"N={N} p={p}: s^2 moves by {moved:.3g} bounds, arg-max {pr.top_two_gap(bad['score'])[0]} -> {pr.top_two_gap(good['score'])[0]}")
    assert moved >= 100
    assert pr.top_two_gap(bad["score"])[0] != pr.top_two_gap(good["score"])[0]


def test_sigma_p_needs_nu_and_the_jitter():
    N, d, p = 129, 3, 17
    X, y, Xs, Xp, Z = inputs(N, d, p)
    gp = factory("SEArd", d)(X, y)
    _, Sig, Vp = pr.pending_moments(gp, Xp)
    bare = gp.cov(Xp, Xp) - Vp.T @ Vp
    bound = var_tol(np.diag(Sig), N, S2F)
    assert np.min(np.abs(np.diag(Sig) - np.diag(bare)) / bound) >= 100
    J = 1e-3 * (S2F + math.exp(2 * LNOISE))                      # set_jitter(1e-3, .): the first try adds 1e-3 x mean(diag cK)
    gj = factory("SEArd", d, 0.5 * math.log(math.exp(2 * LNOISE) + J))(X, y)
    _, Sig_j, _ = pr.pending_moments(gj, Xp)
    assert np.min(np.abs(np.diag(Sig_j) - np.diag(Sig)) / var_tol(np.diag(Sig_j), N, S2F)) >= 100


def test_logei_mean_of_logs_is_not_the_log_of_the_mean():
    N, d, p = 129, 3, 17
    X, y, Xs, Xp, Z = _near_the_top(N, d, p)
    prm = params_of("LogEI", y)
    good = pr.recurrence(factory("SEArd", d), X, y, Xp, Xs, "LogEI", prm, Z, raise_tau=True)
    bad = pr.recurrence(factory("SEArd", d), X, y, Xp, Xs, "LogEI", prm, Z, raise_tau=True, log_of_mean=False)
    fin = np.isfinite(good["score"]) & np.isfinite(bad["score"])
    far = np.abs(bad["score"] - good["score"])[fin] / pr.value_bound(good["score"], S2F, good["asum"])[fin]
    assert fin.sum() >= 200 and far.max() >= 100
    with np.errstate(all="ignore"):                              # what the log-mean-exp IS: the logarithm of the averaged exp(LogEI_s)
        np.testing.assert_allclose(np.exp(good["score"][fin]), np.exp(good["each"][:, fin]).mean(axis=0), rtol=1e-12, atol=1e-300)


# ---- 3. the ABI ----------------------------------------------------------------------------------------------------------------------
def test_pend_header_exports_ctypes_and_julia_agree():
    """include/bohip_pend.h <-> exports <-> _lib.PEND_SIGNATURES <-> julia/BOHipPend.jl: the same four symbols, the same types argument
    by argument, none of them in the model's header or table; the constants agree."""
    from bohip import _lib

    raw = open(os.path.join(ROOT, "include", "bohip_pend.h")).read()
    hdr = re.sub(r"#.*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    c_types = {"int": "int", "double*": "ptr(double)", "int64_t*": "ptr(int64)", "bohip_gp*": "ptr(void)", "int64_t": "int64",
               "uint64_t": "uint64", "bohip_best*": "ptr(best)"}
    protos = {}
    for m in re.finditer(r"([\w \*]+?)\b(bohip_\w+)\s*\(([^()]*)\)\s*;", hdr):
        args = [re.match(r"^(.*?)(\w+)$", a.strip()).group(1) for a in m.group(3).split(",")]
        protos[m.group(2)] = [c_types[re.sub(r"\bconst\b", "", t).replace(" ", "")] for t in [m.group(1)] + args]
    assert set(protos) == WANT == set(_lib.PEND_SIGNATURES)
    assert not WANT & set(_lib.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bohip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", main))
    assert not WANT & declared and len(declared) == len(_lib.SIGNATURES) == 62
    consts = dict(re.findall(r"#define\s+(BOHIP_PEND_\w+)\s+(\d+)", raw))
    assert consts == {"BOHIP_PEND_PMAX": "32", "BOHIP_PEND_SMAX": "1024", "BOHIP_PEND_RAISE_TAU": "1"}
    assert (_lib.PEND_PMAX, _lib.PEND_SMAX, _lib.PEND_RAISE_TAU) == (32, 1024, 1)
    lib = C.CDLL(_lib.LIB_PATH)
    ct = {C.c_int: "int", C.c_int64: "int64", C.c_uint64: "uint64", C.c_void_p: "ptr(void)", C.POINTER(C.c_double): "ptr(double)",
          C.POINTER(C.c_int64): "ptr(int64)", C.POINTER(_lib.Best): "ptr(best)"}
    jl_types = {"Cint": "int", "Int64": "int64", "UInt64": "uint64", "Ptr{Cvoid}": "ptr(void)", "Ptr{Float64}": "ptr(double)",
                "Ptr{Int64}": "ptr(int64)", "Ptr{Best}": "ptr(best)"}
    src = open(os.path.join(ROOT, "julia", "BOHipPend.jl")).read()
    jl = {}
    for m in re.finditer(r"ccall\(\(:(\w+), libbohip\),\s*([\w{}]+),\s*\(([^()]*)\)", src):
        assert m.group(1) not in jl
        jl[m.group(1)] = [jl_types[m.group(2)]] + [jl_types[a.strip()] for a in m.group(3).split(",") if a.strip()]
    assert set(jl) == WANT
    for name in sorted(WANT):
        assert hasattr(lib, name), name
        res, args = _lib.PEND_SIGNATURES[name]
        assert [ct[res]] + [ct[a] for a in args] == protos[name] == jl[name], name
    assert 'include("BOHipPend.jl")' in open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    for fn in ("pending_set!", "pending_info", "score_pending", "acquire_max_pending"):
        assert re.search(r"^function " + re.escape(fn) + r"\(", src, flags=re.M), fn
    code = re.sub(r'"""(.|\n)*?"""', '""', src)
    code = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"#.*", "", code))
    opens = len(re.findall(r"\b(function|if|for|while|begin|struct|module|let|do|try)\b", code))
    assert opens == len(re.findall(r"\bend\b", code))
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b)


# ---- 4. ask / tell on host models --------------------------------------------------------------------------------------------------
class PendingHostModel:
    """The slice of the ElasticGPE interface BOpt and acquire_max_pending touch, on pend_reference: a GP on the CPU that grows, with
    a pending set.  No device."""

    def __init__(self, d):
        self.dim, self.X, self._y = d, np.zeros((0, d)), np.zeros(0)
        self._pending = np.zeros((d, 0), order="F")
        self.calls = []

    x = property(lambda s: np.asfortranarray(s.X.T))
    y = property(lambda s: s._y)
    nobs = property(lambda s: len(s._y))
    pending = property(lambda s: s._pending.copy(order="F"))

    def append_(self, x, y):
        x = np.asarray(x, float).reshape(self.dim, -1)
        self.calls.append(("append", x.shape[1]))
        self.X, self._y = np.concatenate([self.X, x.T]), np.concatenate([self._y, np.atleast_1d(y)])
        return self

    def set_pending(self, xp):
        self._pending = np.asfortranarray(np.asarray(xp, float).reshape(self.dim, -1))
        return self

    def _gp(self):
        return gp_factory("SEArd", np.full(self.dim, -0.3), 0.0, -2.0, 0.0)

    def predict_f(self, xs):
        return self._gp()(self.X, self._y).predict(np.asarray(xs, float).reshape(self.dim, -1).T)

    def score(self, acq, params, xs, want_scores=True):
        xs = np.asarray(xs, float).reshape(self.dim, -1)
        mu, var = self._gp()(self.X, self._y).predict(xs.T)
        sc = pr.acq(acq, list(params), mu, var)
        return sc, float(sc.max()), int(np.argmax(sc))

    def score_pending(self, acq, params, xs, fantasies=0, seed=0, raise_tau=False):
        from bohip.model import PendingScore

        xs = np.asarray(xs, float).reshape(self.dim, -1)
        p = self._pending.shape[1]
        Z = np.random.default_rng(seed).standard_normal((max(fantasies, 1), p)) * (fantasies > 0)
        r = pr.recurrence(self._gp(), self.X, self._y, self._pending.T, xs.T, acq, list(params), Z, raise_tau)
        self.calls.append(("score_pending", p))
        i, _ = pr.top_two_gap(r["score"])
        return PendingScore(r["score"], r["mu"], r["var"], r["score"][i] if i >= 0 else -math.inf, i)


def _opt(bohip, model, n_init=4, maxiter=12, seed=0, fantasies=4, **kw):
    return bohip.BOpt(lambda x: -float(((x - 0.2) ** 2).sum()), model, kw.pop("acq", None) or bohip.UpperConfidenceBound(),
                      bohip.NoModelOptimizer(), [-1.0, -1.0], [1.0, 1.0], maxiterations=maxiter, initializer_iterations=n_init,
                      verbosity=bohip.Silent, acquisitionoptions=dict(method="LN_COBYLA", restarts=2, maxeval=64, **({"fantasies": fantasies} if fantasies else {})),
                      rng=np.random.default_rng(seed), **kw)


def test_ask_tell_bookkeeping():
    import bohip

    f = lambda x: -float(((x - 0.2) ** 2).sum())   # noqa: E731
    m = PendingHostModel(2)
    o = _opt(bohip, m)
    X0 = o.ask(4)                                                 # the initial design comes from the initializer
    assert X0.shape == (2, 4) and o.iterations.i == 4 and m.pending.shape[1] == 4 and m.nobs == 0
    with pytest.raises(ValueError, match="not a pending point"):
        o.tell(X0[:, 0] + 1e-9, 0.0)
    assert m.nobs == 0 and m.pending.shape[1] == 4                # (nothing changed)
    o.tell(X0[:, [2, 0]], [f(X0[:, 2]), f(X0[:, 0])])            # out of order, ONE model update for both
    assert m.calls == [("append", 2)] and m.pending.shape[1] == 2
    o.tell(X0[:, [1, 3]], [f(X0[:, 1]), f(X0[:, 3])])
    assert m.nobs == 4 and m.pending.shape[1] == 0
    o.tell(np.array([0.5, 0.5]), f(np.array([0.5, 0.5])), pending=False)   # an unsolicited observation
    assert m.nobs == 5 and o.observed_optimum == max(m.y)
    X1 = o.ask(3)                                                 # three proposals that see each other
    assert X1.shape == (2, 3) and m.pending.shape[1] == 3 and o.iterations.i == 7
    assert len({X1[:, j].tobytes() for j in range(3)}) == 3
    assert [c for c in m.calls if c[0] == "score_pending"][-1] == ("score_pending", 2)      # the third saw the first two
    dist = [np.linalg.norm(X1[:, a] - X1[:, b]) for a in range(3) for b in range(a)]
    assert min(dist) > 1e-3
    o.tell(X1[:, 1], f(X1[:, 1]))
    assert m.pending.shape[1] == 2 and np.array_equal(m.pending, X1[:, [0, 2]])
    res = o.result()
    assert set(res) == {"observed_optimum", "observed_optimizer", "model_optimum", "model_optimizer"}
    assert res["observed_optimum"] == max(m.y) and np.array_equal(res["observed_optimizer"], m.x[:, int(np.argmax(m.y))])


def test_ask_tell_refusals():
    import bohip

    with pytest.raises(ValueError, match="batchsize"):
        _opt(bohip, PendingHostModel(2), batchsize=2).ask()
    with pytest.raises(ValueError, match="repetitions"):
        _opt(bohip, PendingHostModel(2), repetitions=2).ask()
    with pytest.raises(ValueError, match="repetitions"):
        _opt(bohip, PendingHostModel(2), repetitions=2).tell(np.zeros(2), 0.0, pending=False)

    class NoPending(PendingHostModel):
        set_pending = property(lambda s: (_ for _ in ()).throw(AttributeError("set_pending")))   # (hasattr is False)

    o = _opt(bohip, NoPending(2))
    with pytest.raises(ValueError, match="no pending set"):
        o.ask()
    m = PendingHostModel(2)
    m.append_(np.array([[0.1, -0.4], [0.3, 0.2]]), [0.5, 0.1])
    m.set_pending(np.array([[0.0], [0.0]]))
    for a in (bohip.KnowledgeGradient(), bohip.MaxValueEntropySearch(), bohip.ThompsonSamplingSimple()):
        with pytest.raises(ValueError, match="with pending evaluations is not built"):
            bohip.acquire_max_pending(a, m, [-1.0, -1.0], [1.0, 1.0], dict(restarts=1, maxeval=8))
    with pytest.raises(NotImplementedError):
        bohip.MultiGPE.set_pending(None, np.zeros((2, 1)))
    with pytest.raises(ValueError, match="not a positive integer"):
        _opt(bohip, PendingHostModel(2)).ask(0)


# ---- 5. one point at a time IS boptimize_ -------------------------------------------------------------------------------------------
def test_ask_tell_one_at_a_time_is_boptimize():
    import bohip

    f = lambda x: -float(((x - 0.2) ** 2).sum())   # noqa: E731
    ma, mb = PendingHostModel(2), PendingHostModel(2)
    oa, ob = _opt(bohip, ma, seed=3, fantasies=None), _opt(bohip, mb, seed=3)   # (boptimize_ knows no "fantasies" key)
    ra = bohip.boptimize_(oa)
    while not bohip.isdone(ob):
        x = ob.ask()
        ob.tell(x, f(x[:, 0]))
    rb = ob.result()
    assert ma.x.tobytes() == mb.x.tobytes() and ma.y.tobytes() == mb.y.tobytes() and ma.nobs == 12
    assert ra["observed_optimum"] == rb["observed_optimum"]
    assert np.asarray(ra["observed_optimizer"]).tobytes() == np.asarray(rb["observed_optimizer"]).tobytes()
    assert not [c for c in mb.calls if c[0] == "score_pending"]   # an empty pending set: acquire_max itself
