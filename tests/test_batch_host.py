"""Batch selection without a GPU: the mathematics of bohip_gp_select_batch (rank-one conditioning over the candidate set equals
"append the fantasy, refit, score again"), and the host layer's argument validation and call sequence.

An extension of the reference, whose iteration proposes ONE point (src/BayesianOptimization.jl:185-196)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_reference import gp_factory, recurrence, refit_per_pick   # noqa: E402
from conftest import synth   # noqa: E402

# BASELINE recipe
LL, LSIG, LNOISE, BETA = math.log(0.5), 0.0, -2.0, 0.0


@pytest.mark.parametrize("kern", ["SEArd", "Mat52Ard"])
@pytest.mark.parametrize("acq", ["EI", "UCB", "MI"])
@pytest.mark.parametrize("fantasy", ["believer", "max", "min"])
def test_recurrence_equals_refit_per_pick(kern, acq, fantasy):
    """(N, d, R, q, seed) = (500, 4, 2048, 8, 3): identical picks; values agree to 7e-12 relative where they exceed 1e-3 and to
    1e-8 below (EI under liar = min falls to 1e-29, where 1 + erf cancels: a float64 limit of both statements)."""
    N, d, R, q, seed = 500, 4, 2048, 8, 3
    X, y, Xs = synth(N, d, R, seed)
    params = {"EI": [float(y.max())], "UCB": [2.0], "MI": [1.0, 0.3]}[acq]
    fv = {"believer": "believer", "max": float(y.max()), "min": float(y.min())}[fantasy]
    fac = gp_factory(kern, np.full(d, LL), LSIG, LNOISE, BETA)
    ref = refit_per_pick(fac, X, y, Xs, acq, params, q, fv)
    rec = recurrence(fac, X, y, Xs, acq, params, q, fv)
    assert [r[0] for r in rec] == [r[0] for r in ref]
    assert len(set(r[0] for r in rec)) == q
    for (i, v, mu, var, gap, _), (_, v0, mu0, var0, gap0, _) in zip(rec, ref):
        assert gap0 > 1e-7
        assert abs(v - v0) <= (7e-12 if abs(v0) > 1e-3 else 1e-8) * abs(v0)
        assert abs(mu - mu0) <= 1e-9 * max(1.0, abs(mu0))
        assert abs(var - var0) <= 1e-9


@pytest.mark.parametrize("fantasy", ["believer", "max"])
def test_recurrence_raise_tau(fantasy):
    """EI at tau = max y - 1 with the incumbent following the fantasies (what setparams! does after a real append)."""
    N, d, R, q, seed = 500, 4, 2048, 8, 3
    X, y, Xs = synth(N, d, R, seed)
    fv = "believer" if fantasy == "believer" else float(y.max())
    fac = gp_factory("SEArd", np.full(d, LL), LSIG, LNOISE, BETA)
    ref = refit_per_pick(fac, X, y, Xs, "EI", [float(y.max()) - 1.0], q, fv, raise_tau=True)
    rec = recurrence(fac, X, y, Xs, "EI", [float(y.max()) - 1.0], q, fv, raise_tau=True)
    assert [r[0] for r in rec] == [r[0] for r in ref]
    for a, b in zip(rec, ref):
        assert abs(a[1] - b[1]) <= 1e-9 * abs(b[1])


# ---- the host layer, against a fake model (no device) ---------------------------------------------------------------------
class FakeModel:
    """Records the calls the loop makes; select_batch hands out the first q candidates."""

    def __init__(self, d=2, n=3):
        self.dim = d
        self.x = np.zeros((d, n), order="F")
        self.y = np.arange(n, dtype=float)
        self.calls = []

    @property
    def nobs(self):
        return self.y.size

    def predict_f(self, xs):
        xs = np.asarray(xs, float).reshape(self.dim, -1)
        return np.zeros(xs.shape[1]), np.ones(xs.shape[1])

    def select_batch(self, acq, params, xs, q, fantasy="believer", raise_tau=False):
        self.calls.append(("select_batch", acq, list(params), xs.shape, q, fantasy, raise_tau))
        return np.arange(q, dtype=np.int64), np.linspace(1.0, 0.5, q), np.zeros(q), np.ones(q)

    def score(self, acq, params, xs, want_scores=True):
        xs = np.asarray(xs, float).reshape(self.dim, -1)
        self.calls.append(("score", acq, xs.shape))
        return np.zeros(xs.shape[1]), 0.0, 0

    def append_(self, x, y):
        x = np.asarray(x, float).reshape(self.dim, -1)
        self.calls.append(("append_", x.shape[1]))
        self.x = np.asfortranarray(np.concatenate([self.x, x], axis=1))
        self.y = np.concatenate([self.y, np.atleast_1d(y)])
        return self


@pytest.fixture()
def bo():
    import bohip

    return bohip


def test_acquire_batch_validation(bo):
    m = FakeModel()
    ac = bo.ExpectedImprovement()
    lb, ub = [0.0, 0.0], [1.0, 1.0]
    with pytest.raises(ValueError, match="q = 0"):
        bo.acquire_batch(ac, m, lb, ub, 0)
    with pytest.raises(ValueError, match="exceeds"):
        bo.acquire_batch(ac, m, lb, ub, 9, {"candidates": 8})
    with pytest.raises(ValueError, match="fantasy"):
        bo.acquire_batch(ac, m, lb, ub, 2, {"fantasy": "optimist"})
    with pytest.raises(ValueError, match="unknown batch option"):
        bo.acquire_batch(ac, m, lb, ub, 2, {"restarts": 3})
    with pytest.raises(ValueError, match="xs"):
        bo.acquire_batch(ac, m, lb, ub, 2, {"xs": np.zeros((3, 5))})
    with pytest.raises(ValueError, match="deterministic"):
        bo.acquire_batch(bo.ThompsonSamplingSimple(), m, lb, ub, 2)
    with pytest.raises(RuntimeError, match="empty"):
        bo.acquire_batch(ac, FakeModel(n=0), lb, ub, 2)
    with pytest.raises(NotImplementedError):
        bo.MultiGPE.select_batch(None, "EI", [0.0], np.zeros((2, 5)), 2)   # a device list has no batch selection
    with pytest.raises(NotImplementedError):
        bo.acquire_batch(ac, object(), lb, ub, 2)


def test_acquire_batch_resolves_fantasy_and_candidates(bo):
    m = FakeModel()
    m.y = np.array([1.0, 4.0, -2.0])
    ac = bo.UpperConfidenceBound(bo.NoBetaScaling(), 2.0)
    rng = np.random.default_rng(0)
    for name, want in [("believer", "believer"), ("liar_max", 4.0), ("liar_min", -2.0), ("liar_mean", 1.0)]:
        vals, X = bo.acquire_batch(ac, m, [0.0, 0.0], [1.0, 2.0], 3, {"fantasy": name, "candidates": 16}, rng)
        call = m.calls[-1]
        assert call[0] == "select_batch" and call[1] == "UCB" and call[2] == [2.0] and call[3] == (2, 16) and call[4] == 3
        assert call[5] == want and call[6] is False
        assert X.shape == (2, 3) and len(vals) == 3
        assert np.all(X[1] <= 2.0) and np.all(X >= 0.0)
    xs = np.asfortranarray(rng.random((2, 7)))
    vals, X = bo.acquire_batch(ac, m, [0.0, 0.0], [1.0, 1.0], 2, {"xs": xs, "raise_tau": True})
    assert m.calls[-1][3] == (2, 7) and m.calls[-1][6] is True
    assert np.array_equal(X, xs[:, :2])                      # the fake picks the first q candidates
    assert bo.acquire_batch(ac, m, [0.0, 0.0], [1.0, 1.0], 1)[1].shape == (2, 1)   # default: 4096 candidates
    assert m.calls[-1][3] == (2, 4096)


def test_bopt_batchsize_validation(bo):
    common = (lambda x: 0.0, FakeModel(), bo.ExpectedImprovement(), bo.NoModelOptimizer())
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="batchsize"):
            bo.BOpt(*common, [0, 0], [1, 1], batchsize=bad, initializer_iterations=0)
    with pytest.raises(ValueError, match="batchoptions"):
        bo.BOpt(*common, [0, 0], [1, 1], batchoptions={"candidates": 8}, initializer_iterations=0)
    o = bo.BOpt(*common, [0, 0], [1, 1], initializer_iterations=0)
    assert o.batchsize == 1 and o.batchoptions == {}


def _loop(bo, model, **kw):
    o = bo.BOpt(lambda x: float(np.sum(x)), model, bo.MaxMean(), bo.NoModelOptimizer(), [0.0, 0.0], [1.0, 1.0],
                maxiterations=2, initializer_iterations=0, verbosity=bo.Silent, rng=np.random.default_rng(0),
                acquisitionoptions=dict(method="LN_COBYLA", restarts=2, maxeval=4), **kw)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bo.boptimize_(o)
    return o


def test_batchsize_one_keeps_the_call_sequence(bo):
    """batchsize = 1 is today's loop: per iteration one acquire_max (here a scored candidate set) and one append of
    `repetitions` columns; select_batch is never called."""
    plain, one = FakeModel(), FakeModel()
    _loop(bo, plain)
    _loop(bo, one, batchsize=1)
    assert one.calls == plain.calls
    assert [c[0] for c in one.calls] == ["score", "append_", "score", "append_", "score"]   # (the last: acquire_model_max)
    assert not any(c[0] == "select_batch" for c in one.calls)


def test_batchsize_four_is_one_update_per_iteration(bo):
    m = FakeModel()
    o = _loop(bo, m, batchsize=4, repetitions=2, batchoptions={"candidates": 32, "fantasy": "liar_min"})
    kinds = [c[0] for c in m.calls]
    assert kinds == ["select_batch", "append_", "select_batch", "append_", "score"]
    assert [c[1] for c in m.calls if c[0] == "append_"] == [8, 8]          # 4 points x 2 repetitions, ONE update
    assert m.nobs == 3 + 16 and o.iterations.i == 2
    assert m.calls[0][4] == 4 and m.calls[0][5] == 0.0                      # liar_min resolved from model.y = [0, 1, 2]
