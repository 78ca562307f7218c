"""GPU tests of the gradient under pending evaluations (include/bohip_pend_grad.h): bohip_gp_score_pending_grad,
ElasticGPE.score_pending_grad and acquire_max_pending's "refine".

The reference is the header's formula in NumPy (tests/pend_grad_reference.py, float64 twin).  The gradient's bound is
16 x pend_grad_reference.WORST_GRAD -- the float64 twin's own distance from its extended-precision twin on these very inputs
(tests/test_pend_grad_host.py).  Every comparison prints the share of the bound the device uses, and asserts that the scores, mu,
s^2 and the record are score_pending's bytes and that the three new stages ran."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pend_grad_reference as pg   # noqa: E402
from test_pend_gpu import bohip, make_model   # noqa: E402, F401

pytestmark = pytest.mark.gpu
STAGES = ("pend_weights", "pend_mix", "pend_grad_finish")


def same_bytes(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("scores", "mu", "var")) and \
        (a.best_val, a.best_idx) == (b.best_val, b.best_idx)


def check(m, case, acq):
    """The device's gradient at the candidates of a case against the float64 twin; m: the case's model."""
    ref = pg.reference(case, acq, pg.RAISE[acq])
    m.set_pending(ref["Xp"].T)
    kw = dict(fantasies=ref["S"], seed=ref["seed"], raise_tau=pg.RAISE[acq])
    m.enable_timing(True)
    got, grad = m.score_pending_grad(acq, ref["params"], ref["Xs"].T, **kw)
    labels = [n for n, _ in m.timing()]
    assert grad.shape == ref["grad"].T.shape
    share = float(np.max(pg.distance(acq, grad.T, ref["grad"]))) / (pg.DEVICE_FACTOR * pg.WORST_GRAD[acq])
    print(f"{case} {acq}: gradient uses {share:.3g} of its bound")
    assert same_bytes(got, m.score_pending(acq, ref["params"], ref["Xs"].T, **kw)), (case, acq)
    assert all(k in labels for k in STAGES), labels
    assert share <= 1, (case, acq, share)
    return got, grad


@pytest.mark.parametrize("case", list(pg.CASES))
def test_gradient(bohip, case):
    ref = pg.reference(case, "LogEI", True)
    m = make_model(bohip, ref["kern"], ref["X"], ref["y"])
    for acq in pg.ACQS:
        check(m, case, acq)
    m.close()


def test_empty_set_is_score_grad(bohip):
    ref = pg.reference("n129-p17obs-S64", "UCB", True)
    m = make_model(bohip, ref["kern"], ref["X"], ref["y"])
    got, grad = m.score_pending_grad("UCB", ref["params"], ref["Xs"].T, fantasies=5, seed=1)
    sc, g = m.score_grad("UCB", ref["params"], ref["Xs"].T)
    mu, var = m.predict_f(ref["Xs"].T)
    assert grad.tobytes() == g.tobytes() and got.scores.tobytes() == sc.tobytes()
    assert got.mu.tobytes() == mu.tobytes() and got.var.tobytes() == var.tobytes() and got.best_idx == int(np.argmax(sc))
    m.close()


def test_determinism_and_the_value_call_is_untouched(bohip):
    ref = pg.reference("n129-p17obs-S64", "LogEI", True)
    m, clean = (make_model(bohip, ref["kern"], ref["X"], ref["y"]) for _ in range(2))
    args, kw = ("LogEI", ref["params"], ref["Xs"].T), dict(fantasies=ref["S"], seed=ref["seed"], raise_tau=True)
    m.set_pending(ref["Xp"].T)
    clean.set_pending(ref["Xp"].T)
    a, ga = m.score_pending_grad(*args, **kw)
    b, gb = m.score_pending_grad(*args, **kw)
    assert ga.tobytes() == gb.tobytes() and same_bytes(a, b)
    assert same_bytes(m.score_pending(*args, **kw), clean.score_pending(*args, **kw))   # a clean handle never built the basis
    assert m.factor().tobytes() == clean.factor().tobytes() and m.alpha().tobytes() == clean.alpha().tobytes()
    assert np.array_equal(m.pending, ref["Xp"].T)
    m.close()
    clean.close()


def test_state_is_rebuilt_after_an_append_and_after_set_params(bohip):
    """The basis follows the model.  After an incremental append the gradient is the twin's of all the data; after set_params_ it
    is a fresh handle's at the new noise, within two device bounds (each side lies within one of the truth)."""
    case = "n129-p2dup-S3"
    ref = pg.reference(case, "UCB", True)
    X, y = ref["X"], ref["y"]
    args, kw = ("UCB", ref["params"], ref["Xs"].T), dict(fantasies=ref["S"], seed=ref["seed"], raise_tau=True)
    m = make_model(bohip, ref["kern"], X[:-1], y[:-1], capacity=len(y))
    m.set_pending(ref["Xp"].T)
    stale = m.score_pending_grad(*args, **kw)[1]                  # the basis of N - 1 observations
    m.append_(X[-1], y[-1:])
    assert check(m, case, "UCB")[1].tobytes() != stale.tobytes()
    m.set_params_(logNoise=-1.5)
    fresh = make_model(bohip, ref["kern"], X, y, lnoise=-1.5)
    fresh.set_pending(ref["Xp"].T)
    g1, g2 = m.score_pending_grad(*args, **kw)[1], fresh.score_pending_grad(*args, **kw)[1]
    assert float(np.max(pg.distance("UCB", g1.T, g2.T))) <= 2 * pg.DEVICE_FACTOR * pg.WORST_GRAD["UCB"]
    m.close()
    fresh.close()


def test_errors_leave_the_handle_usable(bohip):
    from bohip import _lib

    lib = _lib.load()
    ref = pg.reference("n17-p1-S1", "UCB", True)
    m = make_model(bohip, ref["kern"], ref["X"], ref["y"])
    m.set_pending(ref["Xp"].T)
    Xs = np.ascontiguousarray(ref["Xs"])
    R, d = Xs.shape
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    prm, sc, g = np.array([2.0, 0.0]), np.empty(R), np.empty((R, d))

    def call(acq_id, S=1, flags=0, grad=g, h=None):
        return lib.bohip_gp_score_pending_grad(h or m._h, acq_id, ptr(prm), ptr(Xs), R, S, 1, flags, ptr(sc),
                                               ptr(grad) if grad is not None else None, None, None, None)

    assert call(_lib.ACQ["UCB"], grad=None) == _lib.E_ARG
    assert call(5) == _lib.E_ARG and call(_lib.ACQ["UCB"], S=-1) == _lib.E_ARG and call(_lib.ACQ["UCB"], S=_lib.PEND_SMAX + 1) == _lib.E_ARG
    assert call(_lib.ACQ["UCB"], flags=2) == _lib.E_ARG
    empty = bohip.ElasticGPE(d, kernel=bohip.SEArd(np.zeros(d), 0.0))
    assert call(_lib.ACQ["UCB"], h=empty._h) == _lib.E_STATE
    empty.close()
    assert call(_lib.ACQ["UCB"]) == 0
    check(m, "n17-p1-S1", "UCB")
    m.close()


def test_ascent(bohip):
    """refine = 4 climbs the four best candidates on the gradient: never worse than the candidate maximum, inside the box, and the
    returned point scores the returned value through score_pending under the seed that produced it.  refine = 0 issues the calls
    it always has: (f, x[0]) below were returned by the commit before the gradient existed, on the same model, options and
    generator state."""
    PARENT = (-1.5792648088810863, 0.6278159693674986)   # recorded from a build of the parent commit on an MI355X
    ref = pg.reference("n17-p1-S1", "LogEI", True)
    m = make_model(bohip, ref["kern"], ref["X"], ref["y"])
    m.set_pending(pg.tp.XS_BOX * np.random.default_rng(3).random((3, 3)))
    a = bohip.LogExpectedImprovement(float(ref["y"].max()))
    lb, ub = np.zeros(3), np.ones(3)
    opts = dict(restarts=2, maxeval=256, fantasies=16, raise_tau=True)
    f0, x0 = bohip.acquire_max_pending(a, m, lb, ub, opts, rng=np.random.default_rng(7), setparams=False)
    f4, x4 = bohip.acquire_max_pending(a, m, lb, ub, dict(opts, refine=4), rng=np.random.default_rng(7), setparams=False)
    print(f"refine = 0: ({f0!r}, {x0[0]!r});  refine = 4: {f4!r} at {x4}")
    assert (f0, float(x0[0])) == PARENT
    assert f4 >= f0 and np.all((x4 >= lb) & (x4 <= ub))
    from bohip.utils import latin_hypercube_sampling

    rng, seeds = np.random.default_rng(7), []                     # the generator's draws, replayed: candidates, then the seed
    for _ in range(2):
        latin_hypercube_sampling(lb, ub, 256, rng)
        seeds.append(int(rng.integers(0, 2 ** 63 - 1)))
    seeds.append(int(rng.integers(0, 2 ** 63 - 1)))               # the ascent's
    again = [m.score_pending("LogEI", a.params(), x4[:, None], fantasies=16, seed=s, raise_tau=True).scores[0] for s in seeds]
    assert f4 in again, (f4, again)
    m.close()
