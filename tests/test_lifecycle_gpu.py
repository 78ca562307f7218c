"""The life cycle of a handle: the resident W = L^-1 and W', and every feature, on models that have lived.

Every feature family is tested elsewhere on a handle that was made, filled with one append_ and factored once.  A Bayesian-optimisation
loop never leaves a handle in that state, so here one scripted history per (kernel, d) pair (tests/lifecycle_inputs.py HISTORY) takes a
handle from capacity 100 (ld = 144) through incremental appends of 1, 2, 3, 5 and 32 rows, two capacity doublings (ld = 272, 528), the
step N0 = 127 -> 128 that moves the alpha row into a new tile, and a change of every hyper-parameter with no fit_() behind it.  The
feature under test is called before the first growth (its scratch then exists at ld = 144) and at the checkpoints A (after a growth),
B (the factor is incremental), C (stale hyper-parameters) and D (after the second growth); after every step INFO_REFITS, INFO_APPENDS,
INFO_CAPACITY and the stage labels say which route the step took.  The call of the entry point under test comes first at every
checkpoint, before any reference call, and goes through `Own`: at C it must be that call which raises INFO_REFITS by one.

  A  the resident state itself: L, alpha, W and W' read back (bohip_debug_read_w) against the np.longdouble inverse of the device's own
     L within the componentwise forward bound of triangular inversion, and W'[c, i] == W[i, c] bit for bit
  B  every feature with its family's twin, bounds and check helpers, on the data and hyper-parameters of the checkpoint
  C  the jittered model (test_hardening_gpu's): batch conditioning and the path draw read jitter_last
  D  MultiGPE.kg / .mes give ElasticGPE's bytes

Every test prints its worst share of its bound (profiles/lifecycle_tests.txt holds the output of a run on an MI355X).  The references
are computed once per checkpoint on the CPU and never written to (the path twin is copied before it takes the device's frequencies)."""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest

import batch_reference as br
import con_reference as cr
import ens_grad_reference as eg
import ens_reference as er
import high_dim_inputs as hd
import joint_reference as jr
import kg_reference as kr
import lifecycle_inputs as li
import logei_reference as lr
import mes_reference as mr
import path_reference as pr
import qei_reference as qr
import test_con_gpu as tc
import test_ens_gpu as te
import test_ens_grad_gpu as tg
import test_fit_gpu as tf
import test_joint_gpu as tj
import test_kg_gpu as tk
import test_mes_gpu as tm
from conftest import var_tol
from matern_reference import MaternGP, first_argmax
from test_high_dim_gpu import SMALL, SPLIT, WHOLE, assert_route, labels
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DEV = 8.0                                                                   # test_logei_gpu.DEV
PAIRS = list(li.PAIRS)
R2, R3 = li.R_SCORE[1:]


# ==== the history =====================================================================================================================
def new_handle(bohip, kern, d, hyp, capacity):
    ll, lsig, lnoise, beta = hyp
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(beta), kernel=getattr(bohip, kern)(ll, lsig), logNoise=lnoise, capacity=capacity)
    m.enable_timing(True)
    return m


def fresh_handle(bohip, ck):
    """A handle made, filled with one append_ and factored once, on the checkpoint's data and hyper-parameters."""
    m = new_handle(bohip, ck.kern, ck.d, ck.hyp, ck.n)
    m.append_(ck.X.T, ck.y)
    return m


class Own:
    """The feature's own entry-point calls go through this: across each of them INFO_REFITS rises by one exactly when the handle was
    stale, so the entry point under test -- not a reference call made before it -- is what reached ensure_fresh.  restale() (at C
    only: anywhere else it would throw the incremental factor away) pushes the same hyper-parameters again, which is all set_hyper
    needs to mark the handle stale, so that a second entry point of one test meets a stale handle too."""

    def __init__(self, m):
        self.m, self.stale, self.at_c, self.extra, self.met_stale = m, False, False, 0, 0

    def refits(self):
        from bohip import _lib

        return self.m.info(_lib.INFO_REFITS)

    def __call__(self, fn, *args, **kwargs):
        r0 = self.refits()
        out = fn(*args, **kwargs)
        rose = self.refits() - r0
        assert rose == (1 if self.stale else 0), (getattr(fn, "__name__", fn), "stale" if self.stale else "fresh", rose)
        self.met_stale += self.stale
        self.stale = False
        return out

    def restale(self):
        if self.at_c:
            assert not self.stale
            self.m.set_params_()
            self.stale, self.extra = True, self.extra + 1


def plain(fn, *args, **kwargs):
    """Own's stand-in for a fresh handle."""
    return fn(*args, **kwargs)


def live(bohip, kern, d, feature, reads_model=True):
    """Runs the history of a pair and calls feature(m, ck, which, state) at every call step: ck the lifecycle_inputs.Checkpoint, which
    the index into the feature's triple of candidate counts, state a dict that lives as long as the handle; state["own"] is the Own
    through which the feature makes the calls of the entry point under test."""
    from bohip import _lib

    X, y, _ = li.data(kern, d)
    m = new_handle(bohip, kern, d, li.hyper(kern, "A"), li.CAPACITY)
    base = (m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS))
    own = Own(m)
    state = {"own": own}
    try:
        for step in li.plan(reads_model=reads_model):
            action, arg, n = step["action"], step["arg"], step["n"]
            if action == "append":
                m.append_(X[n - arg:n].T, y[n - arg:n])
                lab = labels(m)
                if step["route"] == "incremental":
                    assert "append_cov_rows" in lab and "append_W21" in lab and "build_cov" not in lab, (step, lab)
                else:
                    assert "build_cov" in lab and "append_W21" not in lab, (step, lab)
            elif action == "hyper":
                ll, lsig, lnoise, beta = li.hyper(kern, "C")
                m.set_params_(ll=ll, lsigma=lsig, logNoise=lnoise, beta=beta)   # no fit_(): the next reader has to factor again
                own.stale = reads_model
            else:
                ck = li.checkpoint(kern, d, arg)
                assert m.nobs == ck.n
                own.at_c = arg == "C"
                for which in li.CALLS[arg]:
                    feature(m, ck, which, state)
                if own.at_c and reads_model:                                # the feature itself met the stale handle, and factored it
                    assert own.met_stale >= 1 and not own.stale, (ck, own.met_stale, own.stale)
                own.at_c = False
            got = (m.info(_lib.INFO_REFITS) - base[0] - own.extra, m.info(_lib.INFO_APPENDS) - base[1], m.info(_lib.INFO_CAPACITY))
            assert got == (step["refits"], step["appends"], step["cap"]), (step, got)
            if step["freshen"]:                                             # the feature reads the observations alone
                m.predict_f(X[:1].T)
                assert m.info(_lib.INFO_REFITS) - base[0] - own.extra == step["refits"] + 1
    finally:
        m.close()
    return state


def xs_of(ck, R):
    return np.asfortranarray(ck.Xs[:R].T)


@functools.lru_cache(maxsize=None)
def moments(kern, d, name, R):
    ck = li.checkpoint(kern, d, name)
    mu, var = ck.ref.predict(ck.Xs[:R])
    mu.setflags(write=False)
    var.setflags(write=False)
    return mu, var


def mu_tol(ck, mu_r):
    return 1e-6 * np.abs(mu_r) + ck.floor


def share(err, tol):
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    return float(np.max(err / np.maximum(tol, 1e-300))) if err.size else 0.0


class Shares:
    """The worst share of each named bound over a test, printed once and asserted <= 1."""

    def __init__(self, what):
        self.what, self.worst = what, {}

    def note(self, name, err, tol):
        s = share(err, tol)
        self.worst[name] = max(self.worst.get(name, 0.0), s)
        return s

    def done(self):
        print(f"  {self.what}: worst share of each bound: " + ", ".join(f"{k} {v:.2e}" for k, v in self.worst.items()))
        for k, v in self.worst.items():
            assert v <= 1.0, (self.what, k, v)


def per_checkpoint(what):
    """{checkpoint name: Shares} made on demand and closed together."""
    class D(dict):
        def __missing__(self, key):
            self[key] = Shares(f"{what} at {key}")
            return self[key]

        def done(self):
            for k in sorted(self):
                self[k].done()
    return D()


# ==== A. the resident state ===========================================================================================================
def read_w(m, which):
    from bohip import _lib

    lib = C.CDLL(_lib.LIB_PATH)                                             # as tools/w_check.py binds it
    lib.bohip_debug_read_w.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.bohip_debug_read_w.restype = C.c_int
    out = np.zeros((m.nobs, m.nobs))
    assert lib.bohip_debug_read_w(m._h, which, out.ctypes.data_as(C.c_void_p)) == 0
    return out


@pytest.mark.parametrize("kern,d", PAIRS)
def test_resident_factor_inverse_and_its_transpose(bohip, orc, kern, d):
    """L and alpha against the from-scratch fit at test_incremental_append_is_used_and_matches_refit's bounds; tril(W) and triu(W')
    against the extended-precision inverse of the device's own L within N eps |W| |L| |W| entry by entry (a float64 substitution uses
    a hundredth of it: tests/test_lifecycle_host.py); and the two copies of every entry the same bits -- on the rows appends wrote
    that is a property of the code (k_schur_chol and k_apply_w22 store one value twice), on the rows a refit wrote it is asserted as
    well since it holds.  Only the triangles anybody reads count: the strictly upper tiles of W are scratch (tools/w_check.py)."""
    seen = []

    def feature(m, ck, which, state):
        state["own"](m.predict_f, ck.Xs[:1].T)                              # (C: the reader that factors the stale handle)
        if ck.name == "warm" or which != li.CALLS[ck.name][0]:
            return
        n, lo = ck.n, li.APPENDED_FROM[ck.name]
        L, alpha = m.factor(), m.alpha()
        np.testing.assert_allclose(L, ck.ref.L, rtol=1e-9, atol=1e-12, err_msg=repr(ck))
        np.testing.assert_allclose(alpha, ck.ref.alpha, rtol=1e-7, atol=1e-10 * np.abs(ck.ref.alpha).max(), err_msg=repr(ck))
        if kern == "SEArd":                                                 # the C oracle as well, where it has the kernel
            Lo, ao = orc.fit(ck.X, ck.y, ck.ll, ck.lsig, ck.lnoise, ck.beta)
            np.testing.assert_allclose(L, Lo, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(alpha, ao, rtol=1e-7, atol=1e-10 * np.abs(ao).max())
        assert not np.any(np.triu(L, 1))
        W, WT = np.tril(read_w(m, 0)), np.triu(read_w(m, 1))
        Wref = li.inv_lower_ld(L)
        comp, norm = li.inverse_bounds(L, Wref)
        refit_rows, app_rows = slice(0, lo), slice(lo, n)
        s = {"W refit rows": li.inverse_share(W, Wref, comp, refit_rows), "W append rows": li.inverse_share(W, Wref, comp, app_rows),
             "W' refit rows": li.inverse_share(WT.T, Wref, comp, refit_rows), "W' append rows": li.inverse_share(WT.T, Wref, comp, app_rows),
             "W normwise": li.inverse_share(W, Wref, norm)}
        same_app = np.array_equal(WT.T[app_rows], W[app_rows])
        same_all = np.array_equal(WT.T, W)
        a_ref = np.asarray(Wref.T @ (Wref @ (ck.y - ck.beta).astype(np.longdouble)), dtype=np.float64)
        s["alpha vs W'(W r)"] = share(np.abs(alpha - a_ref), 1e-7 * np.abs(a_ref) + 1e-10 * np.abs(a_ref).max())
        print(f"  {ck}: rows [{lo}, {n}) written by appends; share of N eps |W||L||W|: " + ", ".join(f"{k} {v:.2e}" for k, v in s.items())
              + f"; W' == W.T bit for bit: append rows {same_app}, all rows {same_all}")
        seen.append(ck.name)
        assert same_app, (ck, "W' lags W on the rows appends wrote")
        assert same_all, (ck, "W' differs from W.T on rows a refit wrote")
        assert all(v <= 1.0 for v in s.values()), (ck, s)

    live(bohip, kern, d, feature)
    assert seen == ["A", "B", "C", "D"]


@pytest.mark.parametrize("kern,d", PAIRS)
def test_one_append_after_a_refit(bohip, kern, d):
    """The state in which W is right whatever happens to W': a refit (203 rows) and ONE incremental append (3 rows).  The next append
    would compute its W21 from W' and so carry a lagging W' into W, where predict_f sees it; here nothing has read W' yet, so only its
    readers can tell: the two copies of the appended rows bit for bit, and score_grad (U' = V' W through W') against the twin -- with
    predict_f and score, which read W alone, as the control beside them."""
    ck = li.checkpoint(kern, d, "D")
    m = new_handle(bohip, kern, d, ck.hyp, 400)
    m.append_(ck.X[:203].T, ck.y[:203])
    m.append_(ck.X[203:].T, ck.y[203:])
    assert "append_W21" in labels(m) and "build_cov" not in labels(m)
    sh = Shares(f"{ck}, one append after a refit")
    R = li.R_SCORE[0]
    xs = xs_of(ck, R)
    mu_r, var_r = moments(kern, d, "D", R)
    mu, var = m.predict_f(xs)
    sh.note("predict_f mu", np.abs(mu - mu_r), mu_tol(ck, mu_r))
    sh.note("predict_f var", np.abs(var - var_r), var_tol(var_r, ck.n, ck.s2f))
    W, WT = np.tril(read_w(m, 0)), np.triu(read_w(m, 1))
    same = np.array_equal(WT.T[203:], W[203:])
    grad_tol = lambda g_r: 1e-6 * np.abs(g_r) + 1e-9 * np.abs(g_r).max() + 1e-12   # noqa: E731  (test_matern_gpu's)
    for Rg, hint in ((R, 0), (R2, R3), (R2, 0)):                            # gemm_U on the whole-K route (twice), the row-wise U' on the small one
        m.set_batch_hint(hint)
        sc, g = m.score_grad("UCB", [2.5], xs_of(ck, Rg))
        if route_of(Rg, hint) == "small":
            assert_route(m, ["small_V+U"], WHOLE + SPLIT)
        else:
            assert_route(m, ["trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT)
        sc_r, g_r = twin_score_grad(kern, d, "D", Rg, "UCB", (2.5,))
        sh.note(f"score_grad value, {route_of(Rg, hint)} route", np.abs(sc[sub_of(Rg)] - sc_r), 1e-6 * np.abs(sc_r) + ck.floor + 1e-12)
        sh.note(f"score_grad grad, {route_of(Rg, hint)} route", np.abs(g.T[sub_of(Rg)] - g_r), grad_tol(g_r))
    m.set_batch_hint(0)
    m.close()
    print(f"  {ck}, one append after a refit: W' == W.T on the appended rows: {same}")
    sh.done()
    assert same


# ==== B. every feature ================================================================================================================
ACQS = [("EI", None), ("PI", None), ("UCB", [2.5]), ("MI", [1.0, 0.3]), ("MaxMean", [])]


def params_of(p, ck):
    return [float(np.median(ck.y))] if p is None else p


def route_of(R, hint):
    """N <= 206 is two row tiles: no split-K (eight tiles), no pruning (prune_tiles needs three); small_limit = 256."""
    return "small" if max(R, hint) <= 256 else "whole"


# ---- predict_f / score: the control ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d", PAIRS)
def test_predict_and_scores(bohip, kern, d):
    """The control: this is what the suite already compared on lived-in handles.  R2 = 40 runs twice, on the small route and (under
    set_batch_hint) on the whole-K route of the larger calls."""
    sh = per_checkpoint(f"{kern} d={d} predict_f / score")

    def feature(m, ck, which, state):
        own = state["own"]
        R = li.R_SCORE[which]
        xs = xs_of(ck, R)
        mu_r, var_r = moments(kern, d, ck.name, R)
        for hint in ((0, R3) if R <= 256 else (0,)):
            m.set_batch_hint(hint)
            route = route_of(R, hint)
            mu, var = own(m.predict_f, xs)
            own.restale()                                                   # (C: bohip_gp_score meets a stale handle as well)
            s = sh[ck.name]
            s.note("mu", np.abs(mu - mu_r), mu_tol(ck, mu_r))
            s.note("var", np.abs(var - var_r), var_tol(var_r, ck.n, ck.s2f))
            for acq, p in ACQS:
                p = params_of(p, ck)
                sc, bv, bi = own(m.score, acq, p, xs)
                if route == "small":
                    assert_route(m, ["small_V"], WHOLE + SPLIT + ("kstar", "score"))
                else:
                    assert_route(m, ["kstar", "trigemm_sq"], SMALL + SPLIT + ("score",))
                sc_r = ck.ref.score(acq, p, ck.Xs[:R])
                fl = hd.score_floor(acq, p, ck.floor, var_r, ck.n, ck.s2f)
                s.note(acq, np.abs(sc - sc_r), 1e-6 * np.abs(sc_r) + fl)
                assert (bv, bi) == first_argmax(sc)
                if not hd.near_tie(sc_r, fl):
                    assert bi == first_argmax(sc_r)[1], (ck, acq, R)
            tau = float(np.median(ck.y))
            sc, bv, bi = m.score("LogEI", [tau], xs)
            lr.assert_close("value", sc, lr.logei(mu, var, tau)[0], DEV, f"{ck} R={R} LogEI")
            # ... and against the twin's moments: their bounds through the twin's partials, first order (as con_reference.propagate)
            le, a, b = lr.logei(mu_r, var_r, tau)
            s.note("LogEI vs twin moments", np.abs(sc - le),
                   np.abs(a) * mu_tol(ck, mu_r) + np.abs(b) * var_tol(var_r, ck.n, ck.s2f) + 1e-6 * np.abs(le) + 1e-12)
            assert bi == int(np.argmax(sc)) and np.float64(bv).tobytes() == sc[bi].tobytes()
        m.set_batch_hint(0)

    live(bohip, kern, d, feature)
    sh.done()


# ---- score_grad ------------------------------------------------------------------------------------------------------------------------
def sub_of(R, k=24):
    """k candidates spread over [0, R), the first and the last among them."""
    return np.unique(np.linspace(0, R - 1, min(k, R)).round().astype(int))


@functools.lru_cache(maxsize=None)
def twin_score_grad(kern, d, name, R, acq, p):
    ck = li.checkpoint(kern, d, name)
    return ck.ref.score_grad(acq, list(p), ck.Xs[:R][sub_of(R)])


@pytest.mark.parametrize("kern,d", PAIRS)
def test_score_grad(bohip, kern, d):
    """The gradient passes read W' (U' = V' W row-wise on the small route, gemm_U on the whole-K route)."""
    sh = per_checkpoint(f"{kern} d={d} score_grad")

    def feature(m, ck, which, state):
        R = li.R_SCORE[which]
        xs, sub = xs_of(ck, R), sub_of(R)
        for hint in ((0, R3) if R <= 256 else (0,)):
            m.set_batch_hint(hint)
            for acq, p in ACQS:
                p = params_of(p, ck)
                sc, g = state["own"](m.score_grad, acq, p, xs)
                if route_of(R, hint) == "small":
                    assert_route(m, ["small_V+U"], WHOLE + SPLIT)
                else:
                    assert_route(m, ["trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT)
                sc_r, g_r = twin_score_grad(kern, d, ck.name, R, acq, tuple(p))
                s = sh[ck.name]
                s.note(f"{acq} value", np.abs(sc[sub] - sc_r), 1e-6 * np.abs(sc_r) + ck.floor + 1e-12)
                s.note(f"{acq} grad", np.abs(g.T[sub] - g_r), 1e-6 * np.abs(g_r) + 1e-9 * np.abs(g_r).max() + 1e-12)
                np.testing.assert_array_equal(sc, m.score(acq, p, xs)[0])   # value path == gradient path, bit for bit
        m.set_batch_hint(0)

    live(bohip, kern, d, feature)
    sh.done()


# ---- predict_cov, predict_grad -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d", PAIRS)
def test_predict_cov(bohip, kern, d):
    sh = per_checkpoint(f"{kern} d={d} predict_cov")

    def feature(m, ck, which, state):
        R = li.R_COV[which]
        mu, cov = state["own"](m.predict_cov, xs_of(ck, R))
        assert_route(m, ["kstar", "trigemm_sq+V", "gemm_VV", "post_cov"], SMALL + SPLIT)
        mu_r, cov_r = li.posterior(kern, d, ck.name, R)
        sh[ck.name].note("mu", np.abs(mu - mu_r), mu_tol(ck, mu_r))
        sh[ck.name].note("Sigma", np.abs(cov - cov_r), var_tol(cov_r, ck.n, ck.s2f))
        assert np.array_equal(cov, cov.T)

    live(bohip, kern, d, feature)
    sh.done()


@functools.lru_cache(maxsize=None)
def twin_jac(kern, d, name, R):
    ck = li.checkpoint(kern, d, name)
    return cr.posterior_jac(ck.ref, ck.Xs[:R])


@pytest.mark.parametrize("kern,d", PAIRS)
def test_predict_grad(bohip, kern, d):
    def feature(m, ck, which, state):
        R = li.R_SCORE[which]
        res = state["own"](m.predict_grad, xs_of(ck, R))
        # posterior_grad_core has no small pass and split-K needs eight row tiles: one route at every R, whatever the hint
        assert_route(m, ["kstar", "trigemm_sq+V", "gemm_U", "con_post"], SMALL + SPLIT + ("trigemm_sq",))
        tc.check_predict_grad(res, ck.ref, twin_jac(kern, d, ck.name, R), f"  {ck} R={R} predict_grad")

    live(bohip, kern, d, feature)


# ---- select_batch ------------------------------------------------------------------------------------------------------------------------
BATCH = (("UCB", [2.0], "believer"), ("MI", [1.0, 0.3], "max"))
BATCH_Q = 4


def compare_batch(tag, got, ref, N, s2f, sh):
    """test_batch_gpu.compare with the checkpoint's s_f^2; a near tie among the twin's picks is an error of the test's inputs."""
    idx, val, mu, var = got
    for t, row in enumerate(ref):
        i0, v0, mu0, var0, gap0, _ = row
        assert gap0 >= 1e-7, (tag, t, "the twin's top two are a near tie: choose other candidates")
        tv, tm_, ts = li.batch_tols(row, N, s2f)
        assert idx[t] == i0, (tag, t, idx[t], i0)
        sh.note("val", abs(val[t] - v0), tv)
        sh.note("mu", abs(mu[t] - mu0), tm_)
        sh.note("var", abs(var[t] - var0), ts)


@functools.lru_cache(maxsize=None)
def twin_batch(kern, d, name, R, acq, p, fantasy):
    ck = li.checkpoint(kern, d, name)
    fv = fantasy if fantasy == "believer" else float(ck.y.max())
    return br.recurrence(br.gp_factory(kern, ck.ll, ck.lsig, ck.lnoise, ck.beta), ck.X, ck.y, ck.Xs[:R], acq, list(p), BATCH_Q, fv)


@pytest.mark.parametrize("kern,d", PAIRS)
def test_select_batch(bohip, kern, d):
    """V' = K*' W' stays resident over the q rounds: the conditioning reads W' and the handle's noise."""
    sh = per_checkpoint(f"{kern} d={d} select_batch q={BATCH_Q}")

    def feature(m, ck, which, state):
        R = li.R_SCORE[which]
        for acq, p, fantasy in BATCH:
            fv = fantasy if fantasy == "believer" else float(ck.y.max())
            got = state["own"](m.select_batch, acq, p, xs_of(ck, R), BATCH_Q, fantasy=fv)
            # q > 1 has one route whatever R is: K*' chunks with V' kept, then the rounds (bohip_gp_select_batch; q = 1 is bohip_gp_score)
            assert_route(m, ["kstar", "trigemm_sq+V", "batch_rounds"], SMALL + SPLIT + ("trigemm_sq",))
            compare_batch(f"{ck} R={R} {acq} {fantasy}", got, twin_batch(kern, d, ck.name, R, acq, tuple(p), fantasy), ck.n, ck.s2f,
                          sh[ck.name])

    live(bohip, kern, d, feature)
    sh.done()


# ---- thompson ----------------------------------------------------------------------------------------------------------------------------
def thompson_check(m, ck, R, S, seed, sh, lib, own=plain, hint=0):
    """hint: the batch hint in force; the posterior behind the draws is score_core's, which picks its route by size."""
    xs = xs_of(ck, R)
    bv, bi = own(m.thompson, xs, S, seed=seed)
    if route_of(R, hint) == "small":
        assert_route(m, ["small_V", "thompson"], WHOLE + SPLIT + ("kstar",))
    else:
        assert_route(m, ["kstar", "trigemm_sq", "thompson"], SMALL + SPLIT)
    mu_d, var_d = m.predict_f(xs)
    mu_r, var_r = moments(ck.kern, ck.d, ck.name, R)
    for s in range(S):
        z = np.array([lib.bohip_thompson_normal(seed, s, j) for j in range(R)])
        assert (bv[s], bi[s]) == first_argmax(mu_d + np.sqrt(var_d) * z), (ck, s)      # test_matern_gpu's identity
        j = int(bi[s])                                                      # ... and the twin's draw at the winner
        assert var_r[j] > 0
        tol = mu_tol(ck, mu_r)[j] + abs(z[j]) * var_tol(var_r, ck.n, ck.s2f)[j] / math.sqrt(var_r[j])
        sh.note("winner's draw vs twin", abs(bv[s] - (mu_r[j] + math.sqrt(var_r[j]) * z[j])), tol)
    return bv, bi


@pytest.mark.parametrize("kern,d", PAIRS)
def test_thompson(bohip, kern, d):
    from bohip import _lib

    lib = _lib.load()
    sh = per_checkpoint(f"{kern} d={d} thompson")

    def feature(m, ck, which, state):
        R = li.R_SCORE[which]
        bv, bi = thompson_check(m, ck, R, 3, 77 + which, sh[ck.name], lib, state["own"])
        if R <= 256:                                                        # R2 on the whole-K route of the larger calls as well
            m.set_batch_hint(R3)
            thompson_check(m, ck, R, 3, 77 + which, sh[ck.name], lib, state["own"], hint=R3)
            m.set_batch_hint(0)
        if ck.name == "C":                                                  # the same draws on a fresh handle of the new model
            f = fresh_handle(bohip, ck)
            fsh = Shares(f"{ck} thompson, fresh handle")
            fv, fi = thompson_check(f, ck, R, 3, 77 + which, fsh, lib)
            fsh.done()
            np.testing.assert_array_equal(bi, fi)
            mu_r, var_r = moments(kern, d, ck.name, R)
            z = np.array([lib.bohip_thompson_normal(77 + which, s, int(bi[s])) for s in range(3)])
            tol = mu_tol(ck, mu_r)[bi] + np.abs(z) * var_tol(var_r, ck.n, ck.s2f)[bi] / np.sqrt(var_r[bi])
            sh[ck.name].note("lived-in vs fresh / 2", np.abs(bv - fv), 2.0 * tol)
            f.close()

    live(bohip, kern, d, feature)
    sh.done()


# ---- sample_joint, qei_batch ---------------------------------------------------------------------------------------------------------------
def joint_factor_bound(cov_r, N, s2f, jitter):
    """test_joint_gpu.factor_bound with the checkpoint's s_f^2."""
    R = cov_r.shape[0]
    return var_tol(cov_r, N, s2f) + 64 * R * EPS * (float(np.max(np.diag(cov_r))) + jitter)


def joint_check(m, ck, R, S, seed, sh, own=plain):
    xs = xs_of(ck, R)
    js = own(m.sample_joint, xs, S, seed, want_factor=True)
    assert_route(m, ["kstar", "trigemm_sq+V", "gemm_VV", "sample_cholesky", "sample_draw"], SMALL + SPLIT)
    mu_pc, _ = m.predict_cov(xs)
    np.testing.assert_array_equal(js.mu, mu_pc)                             # predict_cov's mean, bit for bit
    mu_r, cov_r = li.posterior(ck.kern, ck.d, ck.name, R)
    Cf = js.factor                                                          # (Sigma of 200 SEArd candidates is singular in float64: jitter)
    assert np.all(np.diag(Cf) > 0) and not np.any(np.triu(Cf, 1))
    sh.note("mu", np.abs(js.mu - mu_r), mu_tol(ck, mu_r))
    sh.note("C C' - Sigma", np.abs(Cf @ Cf.T - (cov_r + js.jitter * np.eye(R))), joint_factor_bound(cov_r, ck.n, ck.s2f, js.jitter))
    Z = jr.normals(seed, S, R)
    sh.note("draw identity", np.abs(js.samples - (js.mu[None, :] + Z @ Cf.T)), jr.draw_identity_bound(js.mu, Cf, Z))
    tj.check_best(js)
    return js


@pytest.mark.parametrize("kern,d", PAIRS)
def test_sample_joint(bohip, kern, d):
    """S = 3 takes the row-panel form, S = 200 the MFMA form (g_sample_mfma_min)."""
    sh = per_checkpoint(f"{kern} d={d} sample_joint")

    def feature(m, ck, which, state):
        R = li.R_COV[which]
        for S in (3, 200):
            js = joint_check(m, ck, R, S, 1000 * R + S, sh[ck.name], state["own"])
            if ck.name == "C":
                f = fresh_handle(bohip, ck)
                fsh = Shares(f"{ck} sample_joint S={S}, fresh handle")
                fj = joint_check(f, ck, R, S, 1000 * R + S, fsh)
                fsh.done()
                mu_r, cov_r = li.posterior(kern, d, ck.name, R)
                sh[ck.name].note("C C' - jitter I, lived-in vs fresh / 2",
                                 np.abs(js.factor @ js.factor.T - fj.factor @ fj.factor.T - (js.jitter - fj.jitter) * np.eye(R)),
                                 2.0 * joint_factor_bound(cov_r, ck.n, ck.s2f, max(js.jitter, fj.jitter)))
                sh[ck.name].note("mu lived-in vs fresh / 2", np.abs(js.mu - fj.mu), 2.0 * mu_tol(ck, mu_r))
                f.close()

    live(bohip, kern, d, feature)
    sh.done()


@pytest.mark.parametrize("kern,d", PAIRS)
def test_qei_batch(bohip, kern, d):
    """The draws are sample_joint's bit for bit (checked against the twin's posterior there and here), the selection the twin's."""
    sh = per_checkpoint(f"{kern} d={d} qei_batch")

    def feature(m, ck, which, state):
        R, S, q = li.R_COV[which], 64, 4
        seed = 500 + which
        xs = xs_of(ck, R)
        tau = float(ck.y.max()) - 1.0
        res = state["own"](m.qei_batch, xs, q, S, seed, tau=tau, want_samples=True)
        assert "qei_select" in labels(m), labels(m)
        js = joint_check(m, ck, R, S, seed, sh[ck.name], state["own"])
        np.testing.assert_array_equal(res.samples, js.samples)
        assert (res.jitter, res.tries) == (js.jitter, js.tries)
        ri, rg = qr.qei_greedy(js.samples, tau, q)
        np.testing.assert_array_equal(res.idx, ri)
        np.testing.assert_array_equal(res.gain, rg)
        assert np.all(res.idx >= 0) and np.all(res.gain > 0)                # non-vacuity: every round had something to gain
        bare = m.qei_batch(xs, q, S, seed, tau=tau)
        np.testing.assert_array_equal(bare.idx, ri)
        np.testing.assert_array_equal(bare.gain, rg)

    live(bohip, kern, d, feature)
    sh.done()


# ---- knowledge gradient, max-value entropy search ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d", PAIRS)
def test_kg(bohip, kern, d):
    """E = 8.  The twin on the device's own posterior (TWIN_REL), that posterior against the twin's, and the hull on the twin's
    posterior (ORACLE_ABS): the last two see a posterior built from a wrong W'."""
    sh = per_checkpoint(f"{kern} d={d} kg")
    E = 8

    def feature(m, ck, which, state):
        R = li.R_COV[which]
        xs = xs_of(ck, R)
        res = state["own"](m.kg, xs, E)
        assert_route(m, ["kg"], SMALL + SPLIT)
        mu, cov = m.predict_cov(xs)
        assert res.mu.tobytes() == mu.tobytes()
        nu = math.exp(2.0 * ck.lnoise) + EPS
        tkg, tseg = tk.twin_of(mu, np.stack([cov[e] / math.sqrt(cov[e, e] + nu) for e in range(E)]))
        rel = tk.check_against_twin(res.values, res.nseg, tkg, tseg, f"{ck} R={R} E={E}")
        assert np.all(tkg > 0.0) and res.best_idx == int(np.argmax(tkg)) and res.best_val == res.values[res.best_idx]
        mu_r, cov_r = li.posterior(kern, d, ck.name, R)
        hull = np.array([kr.kg_hull(mu_r, cov_r[e] / math.sqrt(cov_r[e, e] + nu))[0] for e in range(E)])
        s = sh[ck.name]
        s.note("TWIN_REL", rel, tk.TWIN_REL)
        s.note("mu", np.abs(res.mu - mu_r), mu_tol(ck, mu_r))
        s.note("ORACLE_ABS", np.max(np.abs(res.values - hull)) / max(1.0, float(np.abs(mu_r).max())), tk.ORACLE_ABS)

    live(bohip, kern, d, feature)
    sh.done()


@pytest.mark.parametrize("kern,d", PAIRS)
@pytest.mark.parametrize("mode", ["gumbel", "joint"])
def test_mes(bohip, kern, d, mode):
    sh = per_checkpoint(f"{kern} d={d} mes {mode}")

    def feature(m, ck, which, state):
        R = (li.R_SCORE if mode == "gumbel" else li.R_COV)[which]
        K, seed = (16, 21 + which) if mode == "gumbel" else (8, 17 + which)
        xs = xs_of(ck, R)
        for hint in ((0, R3) if mode == "gumbel" and R <= 256 else (0,)):   # (gumbel: score_core's posterior, its route by size)
            m.set_batch_hint(hint)
            res = state["own"](m.mes, xs, samples=K, mode=mode, seed=seed)
            if mode == "joint":
                assert_route(m, ["mes_rowmax", "mes_values"], SMALL + SPLIT)
            elif route_of(R, hint) == "small":
                assert_route(m, ["small_V", "mes_bracket", "mes_values"], WHOLE + SPLIT + ("kstar",))
            else:
                assert_route(m, ["kstar", "trigemm_sq", "mes_bracket", "mes_values"], SMALL + SPLIT)
            check(m, ck, R, K, seed, xs, res)
        m.set_batch_hint(0)

    def check(m, ck, R, K, seed, xs, res):
        mu_r, var_r = moments(kern, d, ck.name, R)
        s = sh[ck.name]
        s.note("mu", np.abs(res.mu - mu_r), mu_tol(ck, mu_r))
        s.note("var", np.abs(res.var - var_r), var_tol(var_r, ck.n, ck.s2f))
        s.note("values vs twin", tm.rel_err(res.values, mr.values(res.mu, res.var, res.maxvals)[0]), tm.REL)
        assert (res.best_val, res.best_idx) == mr.record(res.values) and np.all(res.values >= 0.0)
        if mode == "gumbel":
            assert (res.jitter, res.tries) == (0.0, 0)
            sq, sm = tm.check_gumbel(res.quantiles, res.maxvals, res.mu, res.var, K, seed, -math.inf, f"{ck} R={R} K={K}")
            s.note("quantiles", sq, 1.0)
            s.note("max values", sm, 1.0)
        else:
            js = m.sample_joint(xs, S=K, seed=seed, jitter=1e-12, max_tries=40, want_factor=True)
            assert res.maxvals.tobytes() == js.samples.max(axis=1).tobytes()     # the row maxima of the same draws
            assert (res.jitter, res.tries) == (js.jitter, js.tries) and np.isnan(res.quantiles).all()
            assert res.mu.tobytes() == js.mu.tobytes()
            _, cov_r = li.posterior(kern, d, ck.name, R)
            s.note("C C' - Sigma", np.abs(js.factor @ js.factor.T - cov_r - js.jitter * np.eye(R)),
                   joint_factor_bound(cov_r, ck.n, ck.s2f, js.jitter))

    live(bohip, kern, d, feature)
    sh.done()


# ---- marginalised acquisition ---------------------------------------------------------------------------------------------------------------
ENS_H = 8


@functools.lru_cache(maxsize=None)
def ens_theta(kern, d):
    T = tf.settings(kern, d, ENS_H, seed=88 + d)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def ens_twin(kern, d, n, R):
    """(row models, mu[H, R], var[H, R]) on the first n observations: the hyper-parameters of the handle play no part."""
    X, y, Xs = li.data(kern, d)
    refs = [er.row_model(kern, X[:n], y[:n], t) for t in ens_theta(kern, d)]
    mv = [r.predict(Xs[:R]) for r in refs]
    return refs, np.array([a for a, _ in mv]), np.array([b for _, b in mv])


@pytest.mark.parametrize("kern,d", PAIRS)
def test_score_ensemble(bohip, kern, d):
    """The same Theta at every checkpoint: a factor slab kept from a shorter model would show.  The call reads the observations
    alone, so at C the handle stays stale (the driver freshens it)."""
    sh = per_checkpoint(f"{kern} d={d} score_ensemble H={ENS_H}")
    Theta = ens_theta(kern, d)
    piv0 = np.zeros(ENS_H, dtype=np.int64)

    def feature(m, ck, which, state):
        R = li.R_SCORE[which]
        refs, mu_r, var_r = ens_twin(kern, d, ck.n, R)
        for acq, p in te.ACQS:
            p = te.params(p, ck.y)
            res = m.score_ensemble(acq, p, xs_of(ck, R), Theta, want_each=True, want_moments=True)
            assert res.route == "device" and np.all(res.pivot == 0)
            assert (te.launches(m, "ens_factor"), te.launches(m, "ens_score")) == (1, 1), labels(m)
            each_r = np.array([er.from_moments(acq, p, mu_r[h], var_r[h]) for h in range(ENS_H)])
            tol = te.score_tols(refs, each_r)
            s = sh[ck.name]
            fin = np.isfinite(each_r)
            assert np.array_equal(res.each[~fin], each_r[~fin])
            for h in range(ENS_H):
                s.note("mu", np.abs(res.mu[h] - mu_r[h]), 1e-6 * np.abs(mu_r[h]) + cr.mu_floor(refs[h].alpha, refs[h].s2f))
                s.note("var", np.abs(res.var[h] - var_r[h]), var_tol(var_r[h], ck.n, refs[h].s2f))
                s.note(f"{acq} each", np.abs(res.each[h] - each_r[h])[fin[h]], tol[h][fin[h]])
            sc_r = er.average(each_r, None, piv0)
            ok = np.isfinite(sc_r)
            s.note(f"{acq} scores", np.abs(res.scores - sc_r)[ok], (tol.sum(axis=0) / ENS_H)[ok])
            assert (res.best_val, res.best_idx) == first_argmax(res.scores)

    live(bohip, kern, d, feature, reads_model=False)
    sh.done()


@functools.lru_cache(maxsize=None)
def ens_twin_grad(kern, d, n, R, acq, p):
    X, y, Xs = li.data(kern, d)
    refs, _, _ = ens_twin(kern, d, n, R)
    sg = [eg.row_score_grad(r, acq, list(p), Xs[:R][sub_of(R, 12)]) for r in refs]
    return np.array([s for s, _ in sg]), np.array([g for _, g in sg])


@pytest.mark.parametrize("kern,d", PAIRS)
def test_score_ensemble_grad(bohip, kern, d):
    """After an append the factor stage must run again (the stage labels say so); a second call on the same data reuses it."""
    sh = per_checkpoint(f"{kern} d={d} score_ensemble_grad H={ENS_H}")
    Theta = ens_theta(kern, d)

    def feature(m, ck, which, state):
        R = li.R_SCORE[which]
        sub = sub_of(R, 12)
        xs = xs_of(ck, R)
        refs, _, _ = ens_twin(kern, d, ck.n, R)
        s = sh[ck.name]
        kept = None
        for acq, p in (("EI", None), ("UCB", [2.5]), ("LogEI", None)):
            p = te.params(p, ck.y)
            res, grad, each_grad = m.score_ensemble_grad(acq, p, xs, Theta, want_each=True)
            nf = te.launches(m, "ens_factor")
            # the slabs hold the factors of Theta for the observations of the last gradient call: stale after an append
            assert nf == (0 if state.get("ens_n") == ck.n else 1), (ck, acq, R, nf, labels(m))
            state["ens_n"] = ck.n
            assert res.route == "device" and np.all(res.pivot == 0) and "ens_grad" in labels(m)
            each_r, g_r = ens_twin_grad(kern, d, ck.n, R, acq, tuple(p))
            tol = tg.grad_tols(g_r)
            fin = np.isfinite(each_r)
            for h in range(ENS_H):
                s.note(f"{acq} each_grad", np.abs(each_grad[h].T[sub] - g_r[h]), tol[h])
                s.note(f"{acq} each", np.abs(res.each[h][sub] - each_r[h])[fin[h]],
                       (1e-6 * np.abs(each_r[h]) + cr.mu_floor(refs[h].alpha, refs[h].s2f) + 1e-12)[fin[h]])
            s.note(f"{acq} grad", np.abs(grad.T[sub] - tg.avg(g_r, None)), tol.sum(axis=0) / ENS_H)
            kept = (acq, p, res, grad, each_grad)
        acq, p, res, grad, each_grad = kept
        val = m.score_ensemble(acq, p, xs, Theta, want_each=True)           # the values are score_ensemble's, bit for bit
        np.testing.assert_array_equal(res.scores, val.scores)
        np.testing.assert_array_equal(res.each, val.each)
        res2, grad2, each2 = m.score_ensemble_grad(acq, p, xs, Theta, want_each=True)
        assert te.launches(m, "ens_factor") == 1                            # (score_ensemble wrote the slabs: test_factor_reuse)
        np.testing.assert_array_equal(grad2, grad)
        np.testing.assert_array_equal(each2, each_grad)

    live(bohip, kern, d, feature, reads_model=False)
    sh.done()


# ---- marginal likelihood ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d", PAIRS)
def test_mll_and_its_gradients(bohip, kern, d):
    """mll_grad forms cK^-1 = W'W from the resident pair; mll_grad_batch keeps its own workspace (fit_ws) across the growths."""
    Theta = ens_theta(kern, d)

    def feature(m, ck, which, state):
        mr_, dnr, dmr, dkr = ck.ref.mll_grad()
        own = state["own"]
        mll, dn, dm, dk = own(m.mll_grad)
        m.synchronize()                                                     # (collects the call's stage labels)
        assert_route(m, ["kinv", "dmll_reduce"])
        own.restale()                                                       # (C: bohip_gp_mll has an ensure_fresh of its own)
        assert own(m.mll) == pytest.approx(mr_, rel=1e-9)
        tf.check_row(mll, np.concatenate([[dn, dm], dk]), mr_, np.concatenate([[dnr, dmr], np.ravel(dkr)]), f"  {ck} mll_grad")
        rows = Theta[:ENS_H - 2 * which]                                    # (8, 6 or 4 settings: the workspace is sized by H too)
        vals, G, piv = m.mll_grad_batch(rows)
        assert np.all(piv == 0)
        for h in range(len(rows)):
            tf.check_row(vals[h], G[h], *tf.twin(kern, ck.X, ck.y, rows[h]), f"  {ck} mll_grad_batch row {h}")
        own = m.mll_grad_batch(li.theta_of(ck.hyp)[None, :])                # the handle's own setting through the batched form
        tf.check_row(own[0][0], own[1][0], mr_, np.concatenate([[dnr, dmr], np.ravel(dkr)]), f"  {ck} mll_grad_batch, own setting")

    live(bohip, kern, d, feature)


# ---- sample paths ------------------------------------------------------------------------------------------------------------------------------
PATH_M, PATH_SEED = 256, 4321


@functools.lru_cache(maxsize=None)
def path_twin(kern, d, name):
    ck = li.checkpoint(kern, d, name)
    return pr.PathTwin(kern, ck.X, ck.y, ck.ll, ck.lsig, ck.lnoise, ck.beta, PATH_M, PATH_SEED)


def path_check(p, ck, tw, om_twin, S, xs, sh):
    """test_path_gpu's checks of one paths object on the points xs (R x d): frequencies, weights, K u = rhs, values, gradients."""
    N, M = ck.n, PATH_M
    tw = copy.copy(tw)                                                      # (the cached twin keeps its own frequencies)
    assert (p.S, p.M, p.N, p.dim) == (S, M, N, ck.d)
    vals, bv, bi = p.eval(xs.T)
    rv, ri = jr.first_argmax_rows(vals)
    np.testing.assert_array_equal(bi, ri)
    np.testing.assert_array_equal(bv, rv)
    pts, coefs = xs[:40], {}
    for s in sorted({0, S // 2, S - 1}):
        om, w, u = p.coef(s)
        coefs[s] = (w, u, None)
        sh.note("omega", np.abs(om - om_twin), pr.frequencies_tol(ck.kern, ck.ll, ck.d, M // 2, PATH_SEED))
        tw.Om = om                                                          # the twin with the device's own frequencies
        tw.PhiX = pr.features(om, tw.X, tw.s2f)
        wt = tw.w(s)
        sh.note("w", np.abs(w - wt), pr.normal_tol(wt))
        ze = pr.noise_normals(PATH_SEED, s, M, N)
        rhs = (ck.y - ck.beta) - tw.PhiX @ w - math.sqrt(tw.diag) * ze
        coefs[s] = (w, u, li.path_solve_bound(tw, u, w, rhs, ze))
        sh.note("K u = rhs", np.abs(tw.K @ u - rhs), coefs[s][2])
        sh.note("values", np.abs(vals[s] - tw.value(xs, u, w)), tw.value_bound(xs, u, w))
        f, g = p.eval_grad(pts.T, np.full(len(pts), s))
        sh.note("grad values", np.abs(f - tw.value(pts, u, w)), tw.value_bound(pts, u, w))
        sh.note("gradients", np.abs(g.T - tw.grad(pts, u, w)), tw.grad_bound(pts, u, w))
    return vals, coefs


@pytest.mark.parametrize("kern,d", PAIRS)
def test_draw_paths(bohip, kern, d):
    """S = 3: the row form of eval, S = 32: the MFMA form (g_path_mfma_min = 24).  The path solve is u = W'(W rhs).  The objects drawn
    at A are kept open and return the bytes of A at D: a paths object does not follow its model."""
    sh = per_checkpoint(f"{kern} d={d} draw_paths M={PATH_M}")

    def feature(m, ck, which, state):
        R = li.R_SCORE[which]
        xs = np.ascontiguousarray(ck.Xs[:R])
        tw = path_twin(kern, d, ck.name)
        om_twin = pr.frequencies(kern, ck.ll, ck.d, PATH_M // 2, PATH_SEED)
        for S in (3, 32):
            p = state["own"](m.draw_paths, S, PATH_M, PATH_SEED)
            assert_route(m, ["path_basis", "path_prior_at_X", "path_solve"])
            vals, coefs = path_check(p, ck, tw, om_twin, S, xs, sh[ck.name])
            assert_route(m, ["path_grad"])
            if ck.name == "C":                                              # the same draw on a fresh handle of the new model
                f = fresh_handle(bohip, ck)
                fsh = Shares(f"{ck} draw_paths S={S}, fresh handle")
                with f.draw_paths(S, PATH_M, PATH_SEED) as fp:
                    _, fcoefs = path_check(fp, ck, tw, om_twin, S, xs, fsh)
                fsh.done()
                for s_, (w, u, bound) in coefs.items():
                    assert np.array_equal(w, fcoefs[s_][0])
                    sh[ck.name].note("K (u lived-in - u fresh) / 2", np.abs(tw.K @ (u - fcoefs[s_][1])), 2.0 * bound)
                f.close()
            if ck.name == "A" and which == 2:
                state.setdefault("kept", []).append((p, S, vals.tobytes(), p.coef(S - 1)[2].tobytes()))
            else:
                p.close()
        if ck.name == "D":
            xa = np.ascontiguousarray(ck.Xs[:R3])
            for p, S, vbytes, ubytes in state["kept"]:
                assert p.N == li.N_AT["A"] and p.eval(xa.T)[0].tobytes() == vbytes and p.coef(S - 1)[2].tobytes() == ubytes
                p.close()
            assert len(state["kept"]) == 2

    live(bohip, kern, d, feature)
    sh.done()


# ---- ascent, DIRECT-L --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,d", PAIRS)
def test_ascend(bohip, kern, d):
    """8 starts; N <= 256 and d <= 16 take the one-workgroup-per-start form.  The twin's score at every returned point."""
    sh = per_checkpoint(f"{kern} d={d} ascend")

    def feature(m, ck, which, state):
        lb, ub = np.zeros(d), np.ones(d)
        starts = np.asfortranarray(np.random.default_rng(d + which).random((d, 8)) * 1.4 - 0.2)     # partly outside the box
        clipped = np.asfortranarray(np.clip(starts, 0.0, 1.0))
        tau = float(np.min(ck.y))                                           # EI alive at every start (test_high_dim_gpu.test_ascent)
        for acq, p in (("UCB", [2.0]), ("EI", [tau]), ("LogEI", [tau])):
            f, Xb, bf, bi, bx, ev = state["own"](m.ascend, acq, p, lb, ub, starts, maxeval=1000)
            lab = labels(m)
            assert "ascent_wg" in lab and "small_V+U" not in lab, lab
            f0, _ = m.score_grad(acq, p, clipped)                           # (after the ascent: at C the ascent meets the stale handle)
            assert 1 <= ev < 1000
            assert np.all(f >= f0 - 1e-12) and np.all(Xb >= lb[:, None]) and np.all(Xb <= ub[:, None])
            fchk, _ = m.score_grad(acq, p, Xb)
            np.testing.assert_allclose(fchk, f, rtol=1e-9, atol=1e-12)      # the returned value is the score at the returned point
            f_twin = lr.logei(*ck.ref.predict(Xb.T), p[0])[0] if acq == "LogEI" else ck.ref.score(acq, p, Xb.T)
            sh[ck.name].note(acq, np.abs(f - f_twin), 1e-6 * np.abs(f_twin) + ck.floor + 1e-12)
            j = int(np.argmax(f))
            assert bi == j and bf == f[j]
            np.testing.assert_array_equal(bx, Xb[:, j])

    live(bohip, kern, d, feature)
    sh.done()


@pytest.mark.parametrize("kern,d", PAIRS)
def test_direct_max(bohip, kern, d):
    """test_direct_l_in_one_library_call's identity (the search evaluates what its NumPy twin asks for through the same entry
    points) and the twin's score at the reported point."""
    from bohip.acquisition import _batched_direct_l

    sh = per_checkpoint(f"{kern} d={d} direct_max")

    def feature(m, ck, which, state):
        lb, ub = np.full(d, -0.2), np.full(d, 1.1)
        maxeval = (300, 120, 500)[which]
        for acq, p in (("UCB", [2.0]), ("EI", [float(np.median(ck.y))])):
            calls = []
            f2, x2, e2, dc = state["own"](m.direct_max, acq, p, lb, ub, maxeval)
            f1, x1, e1 = _batched_direct_l(lambda Z: (calls.append(Z.shape[1]), m.score(acq, p, Z)[0])[1], lb, ub, maxeval)
            assert (f1, e1, len(calls)) == (f2, e2, dc) and np.array_equal(x1, x2) and e2 <= maxeval, (ck, acq)
            assert np.all(x2 >= lb) and np.all(x2 <= ub)
            sc_r = ck.ref.score(acq, p, x2[None, :])[0]
            sh[ck.name].note(acq, abs(f2 - sc_r), 1e-6 * abs(sc_r) + 1e-9)

    live(bohip, kern, d, feature)
    sh.done()


# ---- constrained scores: the members reach D by different histories --------------------------------------------------------------------------
CON_KERNS = ("Mat52Ard", "Mat12Iso")                                        # the two constraint models
CON_CAPS = (1024, 60)                                                       # never re-allocated (ld = 1168); grown at 90 and 127 (ld = 144, 272)
CON_THR, CON_SENSES = (-0.3, 0.25), (1, -1)


@functools.lru_cache(maxsize=None)
def con_data(kern, d):
    """The constraints' observations g[2, 206] at the objective's points, centred as test_con_gpu.member_data's."""
    X = li.data(kern, d)[0]
    out = []
    for c in range(2):
        g = np.cos(2.0 * X + c).sum(1) + 0.1 * np.random.default_rng(700 + 10 * d + c).standard_normal(len(X))
        out.append(g - float(np.median(g)))
    G = np.stack(out)
    G.setflags(write=False)
    return G


def con_hyper(c, d, new):
    """test_fit_gpu.centre for the constraint models; member 1's setting changes at step 7 together with the objective's."""
    t = tf.centre(CON_KERNS[c], d).copy()
    if new and c == 1:
        t = t + np.concatenate([[0.3, -0.1], np.full(t.size - 3, 0.2), [-0.15]])
    return t


@functools.lru_cache(maxsize=None)
def con_twin(kern, d, name, R, acq):
    ck = li.checkpoint(kern, d, name)
    G = con_data(kern, d)
    new = name in ("C", "D")
    twins = [ck.ref] + [tc.twin_of(CON_KERNS[c], ck.X, G[c, :ck.n], con_hyper(c, d, new)) for c in range(2)]
    Xs = np.random.default_rng(1900 + 31 * d + R).random((R, d))
    # tau: the median observation; PI saturates there (test_con_gpu.e2e_twin), and at the maximum fewer than half of its scores are
    # alive once the model has 165 observations (0.42, 0.28, 0.19 at B, C, D for SEArd), so PI takes the 0.9 quantile.  The test asserts
    # what it needs of these inputs, on the twin alone: at least half of the product scores alive, and a winner that leads by more than
    # four times the two tolerances (check_score_con's lead_ok) -- both hold for this seed at every call, no other was tried
    tau = float(np.quantile(ck.y, 0.9)) if acq == "PI" else float(np.median(ck.y))
    tw = cr.score_con(twins, acq, [tau], CON_THR, CON_SENSES, Xs)
    ts, tgb = cr.propagate(twins, acq, tw)
    for a in (Xs, ts, tgb):
        a.setflags(write=False)
    return Xs, twins, tau, tw, ts, tgb


@pytest.mark.parametrize("kern,d", PAIRS)
def test_constrained_scores(bohip, kern, d):
    """ConstrainedGPE over three handles whose leading dimensions differ at every checkpoint (objective 144 / 272 / 528, member 0
    1168 throughout, member 1 144 / 272): one bohip_gp_score_con call, with and without the gradient, the appends through update_."""
    from bohip import _lib
    from test_limits_gpu import check_score_con, live_scores

    X, y, _ = li.data(kern, d)
    G = con_data(kern, d)
    obj = new_handle(bohip, kern, d, li.hyper(kern, "A"), li.CAPACITY)
    cons = []
    for c in range(2):
        t = con_hyper(c, d, False)
        cons.append(new_handle(bohip, CON_KERNS[c], d, (t[2:-1], t[-1], t[0], t[1]), CON_CAPS[c]))
    cm = bohip.ConstrainedGPE(obj, cons, CON_THR, CON_SENSES)
    members = [obj] + cons
    # every member's own route through the history: its capacity, and whether step 7 changes its hyper-parameters (member 0's stay)
    same = tuple(("same", None) if a == "hyper" else (a, v) for a, v in li.HISTORY)
    plans = [li.plan(), li.plan(history=same, capacity=CON_CAPS[0]), li.plan(capacity=CON_CAPS[1])]
    assert [[s_["route"] for s_ in p if s_["action"] == "append"] for p in plans[1:]] == \
        [["refit"] + ["incremental"] * 10, ["refit", "incremental", "refit"] + ["incremental"] * 8]
    base = [(m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS)) for m in members]
    lds = []
    try:
        for k, step in enumerate(plans[0]):
            action, arg, n = step["action"], step["arg"], step["n"]
            if action == "append":
                cm.update_(X[n - arg:n].T, y[n - arg:n], G[:, n - arg:n])
                for m, p in zip(members, plans):
                    lab = labels(m)
                    if p[k]["route"] == "incremental":
                        assert "append_cov_rows" in lab and "append_W21" in lab and "build_cov" not in lab, (p[k], lab)
                    else:
                        assert "build_cov" in lab and "append_W21" not in lab, (p[k], lab)
            elif action == "hyper":
                ll, lsig, lnoise, beta = li.hyper(kern, "C")
                obj.set_params_(ll=ll, lsigma=lsig, logNoise=lnoise, beta=beta)
                t = con_hyper(1, d, True)
                cons[1].set_params_(ll=t[2:-1], lsigma=t[-1], logNoise=t[0], beta=t[1])
            else:
                first = True
                for which in li.CALLS[arg]:
                    R = li.R_SCORE[which]
                    for acq in cr.FORMS:
                        Xs, twins, tau, tw, ts, tgb = con_twin(kern, d, arg, R, acq)
                        if acq in cr.PRODUCT:
                            assert live_scores(tw) >= 0.5                   # non-vacuity: not 0 against 0
                        check_score_con(bohip, members, twins, acq, tau, CON_THR, CON_SENSES, Xs, tw, ts, tgb,
                                        f"  {kern} d={d} {arg} R={R} {acq}", halves=(R == R2))
                        if first:                                           # C: the first score_con call factors both stale members
                            got = [m.info(_lib.INFO_REFITS) - b_[0] for m, b_ in zip(members, base)]
                            assert got == [p[k]["refits"] for p in plans], (arg, got)
                            first = False
                lds.append(tuple(li.ld_of(m.info(_lib.INFO_CAPACITY)) for m in members))
            for m, p, b_ in zip(members, plans, base):                      # the counters of every member after every step
                got = (m.info(_lib.INFO_REFITS) - b_[0], m.info(_lib.INFO_APPENDS) - b_[1], m.info(_lib.INFO_CAPACITY), m.nobs)
                assert got == (p[k]["refits"], p[k]["appends"], p[k]["cap"], n), (p[k], got)
    finally:
        cm.close()
    assert lds == [(144, 1168, 144), (272, 1168, 272), (272, 1168, 272), (272, 1168, 272), (528, 1168, 272)], lds


# ==== C. the jittered model ==========================================================================================================
@pytest.fixture
def jittered(bohip, orc):
    """test_hardening_gpu's singular model under set_jitter(1e-3, 3): one try, J = 1e-3 x mean diag, the oracle's twin agreeing.
    One handle per test: the second test appends to it."""
    from bohip import _lib
    from oracle.oracle import fit_with_jitter

    X, y, Xa, ya = li.jitter_data()
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(li.JIT_BETA), kernel=bohip.SEArd(li.JIT_LL, li.JIT_LSIG), logNoise=li.JIT_LNOISE,
                         capacity=len(y) + 8)
    m.enable_timing(True)
    with pytest.raises(bohip.BohipError):
        m.append_(X.T, y)
    m.set_jitter(li.JIT_REL, li.JIT_TRIES)
    m.fit_()
    _, _, tries, J = fit_with_jitter(orc, X, y, li.JIT_LL, li.JIT_LSIG, li.JIT_LNOISE, li.JIT_BETA, li.JIT_REL, li.JIT_TRIES)
    assert m.info(_lib.INFO_JITTER_STEPS) == tries == 1
    assert J == li.JIT_REL * (math.exp(2.0 * li.JIT_LSIG) + math.exp(2.0 * li.JIT_LNOISE))
    print(f"  jittered model: J = {J:.6g} after {tries} try")
    yield m, X, y, Xa, ya, J
    m.close()


def jitter_ref(X, y, J):
    return MaternGP("SEArd", X, y, li.JIT_LL, li.JIT_LSIG, li.lognoise_with(li.JIT_LNOISE, J), li.JIT_BETA)


def jitter_batch_check(m, X, y, J, what):
    """select_batch against the twin whose noise is nu0 + J; the twin without J in the fantasy's noise is > 100 tolerances away."""
    Xs = li.jitter_candidates(li.JIT_R)
    s2f = math.exp(2.0 * li.JIT_LSIG)
    sh = Shares(what)
    for acq, p, fantasy in li.JIT_BATCH:
        ref = li.jitter_batch_twin(X, y, Xs, acq, p, fantasy, J)
        without = li.jitter_batch_twin(X, y, Xs, acq, p, fantasy, J, fantasy_noise_has_j=False)
        moved = li.batch_moved(ref, without, len(y), s2f)
        print(f"  {what} {acq} {fantasy}: the twin without J differs by {moved:.3g} x the tolerance")
        assert moved > 100.0, "choose another JIT_SEED"
        fv = fantasy if fantasy == "believer" else float(y.max())
        got = m.select_batch(acq, p, np.asfortranarray(Xs.T), li.JIT_Q, fantasy=fv)
        compare_batch(f"{what} {acq} {fantasy}", got, ref, len(y), s2f, sh)
    sh.done()


def test_jittered_select_batch_and_paths(bohip, jittered):
    """bf.noise and k_path_rhs's sqrt(noise) carry jitter_last: a jittered model is exactly a model whose noise is nu0 + J."""
    m, X, y, _, _, J = jittered
    jitter_batch_check(m, X, y, J, "jittered select_batch")
    twin = li.jitter_path_twin(X, y, J)
    om_twin, tw = twin.Om, copy.copy(twin)                                  # tw: the twin with the device's own frequencies
    nu0 = math.exp(2.0 * li.JIT_LNOISE) + EPS
    xs = li.jitter_candidates(129, seed=li.JIT_SEED + 1)
    sh = Shares("jittered draw_paths")
    for S in (3, 32):
        with m.draw_paths(S, li.JIT_M, li.JIT_PATH_SEED) as p:
            vals, _, _ = p.eval(xs.T)
            for s in sorted({0, S - 1}):
                om, w, u = p.coef(s)
                sh.note("omega", np.abs(om - om_twin), pr.frequencies_tol("SEArd", li.JIT_LL, 2, li.JIT_M // 2, li.JIT_PATH_SEED))
                tw.Om = om
                tw.PhiX = pr.features(om, X, tw.s2f)
                sh.note("w", np.abs(w - tw.w(s)), pr.normal_tol(tw.w(s)))
                ze = pr.noise_normals(li.JIT_PATH_SEED, s, li.JIT_M, len(y))
                rhs = (y - li.JIT_BETA) - tw.PhiX @ w - math.sqrt(tw.diag) * ze
                bound = li.path_solve_bound(tw, u, w, rhs, ze)
                without = (y - li.JIT_BETA) - tw.PhiX @ w - math.sqrt(nu0) * ze
                moved = float(np.max(np.abs(rhs - without) / bound))
                assert moved > 100.0, moved                                 # non-vacuity: a right-hand side without J is far outside
                sh.note("K u = rhs", np.abs(tw.K @ u - rhs), bound)
                sh.note("values", np.abs(vals[s] - tw.value(xs, u, w)), tw.value_bound(xs, u, w))
    print(f"  jittered draw_paths: the right-hand side without J lies {moved:.3g} bounds away")
    sh.done()


def test_jittered_cov_mll_and_an_append(bohip, jittered):
    """predict_cov, mll and mll_grad on the jittered model, then one incremental append (p = 3: its new diagonal entries carry J too)
    and select_batch again on the longer model."""
    from bohip import _lib

    m, X, y, Xa, ya, J = jittered
    sh = Shares("jittered predict_cov / mll / append")

    def check(Xn, yn, what):
        ref = jitter_ref(Xn, yn, J)
        Xs = li.jitter_candidates(200, seed=li.JIT_SEED + 2)
        mu, cov = m.predict_cov(np.asfortranarray(Xs.T))
        mu_r, cov_r = ref.predict_cov(Xs)
        sh.note(f"{what} mu", np.abs(mu - mu_r), 1e-6 * np.abs(mu_r) + cr.mu_floor(ref.alpha, ref.s2f))
        sh.note(f"{what} Sigma", np.abs(cov - cov_r), var_tol(cov_r, len(yn), ref.s2f))
        mr_, dnr, dmr, dkr = ref.mll_grad()
        mll, dn, dm, dk = m.mll_grad()
        # d/dlogNoise of the twin is taken through logNoise' = log sqrt(nu0 + J): the chain rule back to logNoise (J is a constant)
        dnr = dnr * math.exp(2.0 * li.JIT_LNOISE) / (math.exp(2.0 * li.JIT_LNOISE) + J)
        assert m.mll() == pytest.approx(mr_, rel=1e-9)
        g, g_r = np.concatenate([[dn, dm], dk]), np.concatenate([[dnr, dmr], np.ravel(dkr)])
        sh.note(f"{what} mll", abs(mll - mr_), 1e-9 * abs(mr_))
        sh.note(f"{what} mll_grad", np.abs(g - g_r), 1e-6 * np.abs(g_r) + 1e-8 * np.abs(g_r).max())

    check(X, y, "N=300")
    appends = m.info(_lib.INFO_APPENDS)
    m.append_(Xa.T, ya)
    assert m.info(_lib.INFO_APPENDS) == appends + 1 and "append_W21" in labels(m)       # the incremental route, p = 3
    X2, y2 = np.vstack([X, Xa]), np.concatenate([y, ya])
    check(X2, y2, "N=303")
    jitter_batch_check(m, X2, y2, J, "jittered select_batch after the append")
    sh.done()


# ==== D. MultiGPE.kg / .mes ===========================================================================================================
def test_multigpe_kg_and_mes_give_the_single_handle_bytes(bohip):
    kern, d = PAIRS[0]
    ck = li.checkpoint(kern, d, "B")
    single = fresh_handle(bohip, ck)
    ll, lsig, lnoise, beta = ck.hyp
    mg = bohip.MultiGPE(d, devices=(0,), shards_per_device=2, mean=bohip.MeanConst(beta), kernel=getattr(bohip, kern)(ll, lsig),
                        logNoise=lnoise, capacity=ck.n)
    mg.append_(ck.X.T, ck.y)
    xs = xs_of(ck, li.R_COV[0])
    a, b = single.kg(xs, 8), mg.kg(xs, 8)
    assert a.values.tobytes() == b.values.tobytes() and a.nseg.tolist() == b.nseg.tolist() and a.mu.tobytes() == b.mu.tobytes()
    assert (a.best_val, a.best_idx) == (b.best_val, b.best_idx) and np.all(a.values > 0)
    for mode, K in (("gumbel", 16), ("joint", 8)):
        a, b = single.mes(xs, samples=K, mode=mode, seed=9), mg.mes(xs, samples=K, mode=mode, seed=9)
        for name in ("values", "maxvals", "mu", "var"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (mode, name)
        assert a.quantiles.tobytes() == b.quantiles.tobytes() and (a.best_val, a.best_idx, a.jitter, a.tries) == \
            (b.best_val, b.best_idx, b.jitter, b.tries)
    mu_r, var_r = moments(kern, d, "B", li.R_COV[0])                        # ... and they are the model's: the posterior of the twin
    assert np.all(np.abs(a.mu - mu_r) <= mu_tol(ck, mu_r)) and np.all(np.abs(a.var - var_r) <= var_tol(var_r, ck.n, ck.s2f))
    single.close()
    mg.close()
