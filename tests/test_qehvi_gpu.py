"""Greedy Monte-Carlo q-EHVI on the device (include/bohip_qehvi.h): the selection against the exact rational reference
(tests/qehvi_reference.py), the prefix property in q, the batch call against sample_joint + the selection, and one BOpt run."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import qehvi_reference as qh
from test_parity_gpu import bohip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = Fraction(2) ** -52
REF = (-0.125, 0.0625)
# (S, R, n_front, q, seed): S and R on both sides of the 32-draw block and of the 128- / 256-wide workgroups, fronts up to the limit
CASES = [(1, 1, 0, 1, 0), (33, 129, 1, 4, 1), (70, 300, 17, 16, 2), (33, 300, 0, 16, 3), (70, 129, 17, 4, 4), (1, 300, 1, 1, 5),
         (33, 129, 1024, 4, 6)]


def bound(S, n, q):
    """Relative: the roundings of the widest sum (n + q + 1 strips, S draws, the differences, the division); nothing cancels."""
    return (n + q + S + 8) * EPS


@functools.lru_cache(maxsize=None)
def problem(S, R, n, q, seed):
    """Entries outside ref, a NaN and a +Inf column, a strong column and its twin; every winner clear of the runner-up by > 2 bounds."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.random(n))
    front = np.stack([0.1 + 1.5 * t, 0.1 + 1.5 * (1.0 - t) ** 1.25 + 1e-3 * (n - np.arange(n))])
    m0, m1 = rng.uniform(-0.6, 1.9, R), rng.uniform(-0.6, 1.9, R)
    F0, F1 = m0 + 0.5 * rng.standard_normal((S, R)), m1 + 0.5 * rng.standard_normal((S, R))
    if R > 8:
        F0[:, 1], F1[:, 2] = np.nan, np.inf
        F0[:, 3], F1[:, 3] = 2.0 + 0.3 * rng.random(S), 2.0 + 0.3 * rng.random(S)      # dominates most of every staircase: picked first
        F0[:, 7], F1[:, 7] = F0[:, 3], F1[:, 3]                                        # its twin
    idx, gains, seconds, most = qh.greedy(F0, F1, front, REF, q)
    for k in range(q):
        if idx[k] >= 0:
            assert gains[k] - seconds[k] > 2 * bound(S, n, q) * gains[k], (S, R, n, q, seed, k)
    return F0, F1, front, idx, gains, most


def select(bohip, h, F0, F1, front, q):
    from bohip import _lib
    dp, idx, gain = C.POINTER(C.c_double), np.full(q, 7, dtype=np.int64), np.full(q, 7.0)
    F0, F1, front, ref = (np.ascontiguousarray(a, dtype=np.float64) for a in (F0, F1, front, REF))
    _lib.check(_lib.load().bohip_mo_qehvi_select(h, F0.ctypes.data_as(dp), F1.ctypes.data_as(dp), F0.shape[0], F0.shape[1],
                                                 front.ctypes.data_as(dp), front.shape[1], ref.ctypes.data_as(dp), q,
                                                 idx.ctypes.data_as(C.POINTER(C.c_int64)), gain.ctypes.data_as(dp)))
    return idx, gain


@pytest.mark.parametrize("S,R,n,q,seed", CASES)
def test_select_matches_the_exact_reference(bohip, S, R, n, q, seed):
    bare = gpe(bohip)                                                   # (no observations: the handle gives the device only)
    F0, F1, front, want, gains, most = problem(S, R, n, q, seed)
    idx, gain = select(bohip, bare._h, F0, F1, front, q)
    np.testing.assert_array_equal(idx, want)
    for k in range(q):
        err = abs(Fraction(float(gain[k])) - gains[k])
        print(f"round {k}: idx {idx[k]} gain {gain[k]:.17g} rel err {float(err / gains[k]) if gains[k] else 0.0:.2e}")
        assert err <= bound(S, n, q) * gains[k], (k, float(gain[k]), float(gains[k]))
    if R > 8 and S > 1:
        assert want[0] == 3 and 7 not in want.tolist()                  # the twin's gain after column 3 is exactly 0
    if n == 17:
        assert most >= 2                                                # a pick removed several staircase points at once
    if (S, R, q) == (33, 129, 4):                                       # the first 2 entries of a q = 4 call are the q = 2 call's
        i2, g2 = select(bohip, bare._h, F0, F1, front, 2)
        assert i2.tobytes() == idx[:2].tobytes() and g2.tobytes() == gain[:2].tobytes()


def gpe(bohip):
    return bohip.ElasticGPE(2, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd([-0.7, -0.7], 0.0), logNoise=-2.0, capacity=64)


def small_model(bohip, seed):
    rng, m = np.random.default_rng(seed), gpe(bohip)
    X = rng.random((2, 40))
    y = np.sin(3 * X[0] + seed) + np.cos(2 * X[1]) + 0.05 * rng.standard_normal(40)
    m.append_(X, y)
    return m


@pytest.mark.parametrize("same", [False, True])
def test_batch_is_sample_joint_then_select(bohip, same):
    from bohip import _lib
    from bohip.model import MultiObjectiveGPE

    m0 = small_model(bohip, 1)
    mo = MultiObjectiveGPE((m0, m0 if same else small_model(bohip, 2)))
    m1 = mo.objectives[1]
    xs = np.asfortranarray(np.random.default_rng(9).random((2, 300)))
    res = mo.qehvi_batch(xs, 4, 70, 5, want_samples=True)
    for m, seed, got in ((m0, 5, res.samples[0]), (m1, 5 ^ _lib.QEHVI_SEED_XOR, res.samples[1])):
        np.testing.assert_array_equal(got, m.sample_joint(xs, 70, seed).samples)
    idx, gain = mo.qehvi_select(res.samples[0], res.samples[1], 4)
    assert idx.tobytes() == res.idx.tobytes() and gain.tobytes() == res.gain.tobytes() and res.gain[0] > 0


def test_bopt_runs_batches_of_three(bohip):
    model = bohip.MultiObjectiveGPE((gpe(bohip), gpe(bohip)))
    two = lambda x: (-(x[0] - 0.2) ** 2 - x[1] ** 2, -(x[0] - 0.8) ** 2 - (x[1] - 1.0) ** 2)   # noqa: E731
    o = bohip.BOpt(two, model, bohip.ExpectedHypervolumeImprovement(), bohip.NoModelOptimizer(), [0.0, 0.0], [1.0, 1.0],
                   verbosity=bohip.Silent, maxiterations=6, initializer_iterations=3, batchsize=3, rng=np.random.default_rng(0),
                   batchoptions={"method": "qehvi", "candidates": 64, "draws": 32})
    out = bohip.boptimize_(o)
    assert out["observed_front"]["y"].shape[0] == 2 and [m.nobs for m in model.objectives] == [3 + 3 * 3] * 2
