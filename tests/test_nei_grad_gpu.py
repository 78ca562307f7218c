"""GPU tests of the gradient of noisy expected improvement (include/bohip_nei_grad.h): bohip_gp_score_nei_grad,
ElasticGPE.nei_grad, NoisyExpectedImprovement under acquire_max's "refine".

The reference is the header's formula in NumPy (tests/nei_grad_reference.py, float64 twin).  The gradient's bound is
16 x nei_grad_reference.WORST_GRAD -- the float64 twin's own distance from its extended-precision twin on these very inputs
(tests/test_nei_grad_host.py test_tolerance_source) times nei_reference.DEVICE_FACTOR; the scores, mu and s^2 of the gradient call
are held to nei_reference.bounds as bohip_gp_score_nei's are (test_nei_gpu.check_scores).  Every comparison prints the share of the
bound the device uses.  LogEI is compared at synth's candidates; EI and PI, which are exactly 0 at most of those, at
candidates of their own, every one live and with a gradient of hundreds of bounds (nei_grad_reference.FAR_SHIFT / RING say where and why)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nei_grad_reference as ng   # noqa: E402
import nei_reference as nr   # noqa: E402
from test_nei_gpu import NAME, bohip, check_scores, grid_model, model_of   # noqa: E402, F401

pytestmark = pytest.mark.gpu


def check(tag, m, R, S, acq, N):
    """The device's gradient and scores at the first R candidates of an input against the float64 twin."""
    ref = ng.reference(tag, S, acq)
    Xs = ng.spec(tag, acq)["Xs"][:R]
    got, grad = m.nei_grad(Xs.T, S=S, seed=nr.SEED, acq=NAME[acq], jitter_rel=nr.JREL)
    assert grad.shape == (Xs.shape[1], R)
    share = float(np.max(ng.distance(acq, grad.T, dict(ref, grad=ref["grad"][:R])))) / (nr.DEVICE_FACTOR * ng.WORST_GRAD[acq])
    print(f"{tag} R={R} S={S} {acq}: gradient uses {share:.3g} of its bound")
    check_scores(f"{tag} R={R} S={S} [grad call]", got, ref, R, acq, N)
    assert share <= 1, (tag, R, S, acq, share)
    return got, grad


@pytest.mark.parametrize("model", list(nr.MODELS))
@pytest.mark.parametrize("N", ng.NS)
@pytest.mark.parametrize("R", ng.RS)
def test_gradient(bohip, model, N, R):
    m = grid_model(bohip, model, N)
    m.enable_timing(True)
    for S in ng.SS:
        for acq in nr.ACQS:
            check((model, N), m, R, S, acq, N)
            lab = [n for n, _ in m.timing()]
            assert all(k in lab for k in ("nei_means", "nei_weights", "nei_mix", "nei_grad_finish")) and "small_V" not in lab, lab
    m.close()


def test_s_step_edges(bohip):
    N, R = 129, 40
    m = grid_model(bohip, "se3", N)
    for S in ng.S_EDGES:
        for acq in nr.ACQS:
            check(("se3", N), m, R, S, acq, N)
    m.close()


def test_widest_dimension_bucket(bohip):
    m = model_of(bohip, ng.d20_spec(), lnoise=ng.D20["lnoise"])
    for acq in nr.ACQS:
        check("d20", m, ng.D20["R"], ng.D20["S"], acq, ng.D20["N"])
    m.close()


def test_nine_row_tiles_split_k(bohip):
    N, R, S = nr.BIG_N, 300, nr.BIG_S
    tag = ("se3", N, max(nr.BIG_RS))
    m = model_of(bohip, nr.spec(tag), lnoise=nr.MODELS["se3"]["lnoise"])
    m.enable_timing(True)
    for acq in nr.ACQS:
        check(tag, m, R, S, acq, N)
        assert "split_U" in [n for n, _ in m.timing()]
    m.close()


def test_weighted_handle(bohip):
    x_raw, y_raw, X, ybar, reps, Xs = nr.weighted_data()
    p = nr.MODELS["se3"]
    m = bohip.ElasticGPE.from_data(x_raw, y_raw, mean=bohip.MeanConst(p["beta"]), kernel=bohip.SEArd(nr.model_ll("se3"), p["lsig"]),
                                   logNoise=p["lnoise"], collapse=True)
    for acq in nr.ACQS:
        check("weighted", m, len(Xs), 5, acq, 40)
    m.close()


@pytest.mark.parametrize("N,R", [(129, 40), (300, 700)])
def test_determinism_and_handle_reuse(bohip, N, R):
    from bohip import _lib

    m, clean = grid_model(bohip, "se3", N), grid_model(bohip, "se3", N)
    Xs = nr.data("se3", N, R)[2]
    kw = dict(S=5, seed=nr.SEED, acq="logei", jitter_rel=nr.JREL)
    a, ga = m.nei_grad(Xs.T, **kw)
    builds = m.nei_info(_lib.NEI_INFO_REBUILDS)
    b, gb = m.nei_grad(Xs.T, **kw)
    assert ga.tobytes() == gb.tobytes() and a.score.tobytes() == b.score.tobytes() and a.best == b.best
    assert m.nei_info(_lib.NEI_INFO_REBUILDS) == builds == 1
    after, plain = m.nei(Xs.T, **kw), clean.nei(Xs.T, **kw)      # a gradient call leaves the value call's bytes and the model alone
    for name in ("score", "mu", "var", "tau"):
        assert getattr(after, name).tobytes() == getattr(plain, name).tobytes(), name
    assert m.nei_info(_lib.NEI_INFO_REBUILDS) == 1 and m.nei_info(_lib.NEI_INFO_BYTES) >= clean.nei_info(_lib.NEI_INFO_BYTES)
    assert m.factor().tobytes() == clean.factor().tobytes() and m.alpha().tobytes() == clean.alpha().tobytes()
    m.close()
    clean.close()


def test_errors_leave_the_handle_usable(bohip):
    from bohip import _lib

    lib = _lib.load()
    N, R = 17, 40
    m = grid_model(bohip, "se3", N)
    Xs = np.ascontiguousarray(nr.data("se3", N, R)[2])
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    sc, g = np.empty(R), np.empty((R, 3))

    def call(acq_id, grad=g, h=None):
        return lib.bohip_gp_score_nei_grad(h or m._h, acq_id, None, ptr(Xs), R, 5, nr.SEED, nr.JREL, ptr(sc), ptr(grad) if grad is not None else None,
                                           None, None, None)

    assert call(_lib.ACQ["UCB"]) == _lib.E_ARG
    assert call(_lib.ACQ["EI"], grad=None) == _lib.E_ARG
    empty = bohip.ElasticGPE(3, kernel=bohip.SEArd(np.zeros(3), 0.0))
    assert call(_lib.ACQ["EI"], h=empty._h) == _lib.E_STATE
    empty.close()
    assert call(_lib.ACQ["EI"]) == 0
    check(("se3", N), m, R, 5, "EI", N)
    m.close()


def test_ascent(bohip):
    """refine = 4 climbs the four best candidates on the gradient: never worse than the candidate maximum, and the returned point
    scores the returned value through model.nei (recorded: 0.258 -> 0.314).  refine = 0 issues the calls it always has: (f, x[0]) below were returned by the commit before the
    gradient existed, on the same model, options and generator state."""
    PARENT = (0.2580258693636221, 0.5984267199281258)   # recorded from a build of the parent commit on an MI355X
    m = grid_model(bohip, "se3", 17)
    a = bohip.NoisyExpectedImprovement(S=16, seed=1, jitter_rel=nr.JREL)
    lb, ub = np.zeros(3), np.ones(3)
    f0, x0 = bohip.acquire_max(a, m, lb, ub, dict(restarts=2, maxeval=256), rng=np.random.default_rng(7))
    f4, x4 = bohip.acquire_max(a, m, lb, ub, dict(restarts=2, maxeval=256, refine=4), rng=np.random.default_rng(7))
    print(f"refine = 0: ({f0!r}, {x0[0]!r});  refine = 4: {f4!r} at {x4}")
    assert (f0, float(x0[0])) == PARENT
    assert f4 >= f0 and np.all((x4 >= lb) & (x4 <= ub))
    # (f4 comes from the gradient call, whose variance pass runs another route than nei's: each lies within the EI bound of the twin)
    assert abs(m.nei(x4[:, None], S=16, seed=1, acq="ei", jitter_rel=nr.JREL).score[0] - f4) <= 2 * nr.DEVICE_FACTOR * nr.WORST["EI"]
    m.close()
