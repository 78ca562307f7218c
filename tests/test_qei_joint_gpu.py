"""GPU tests of the joint q-EI of a batch and its gradient (include/bohip_qei_joint.h): bohip_gp_qei_joint,
ElasticGPE.qei_joint and acquire_batch's "refine".

The reference is the header's statements in NumPy (tests/qei_joint_reference.py, float64 twin).  Value and gradient are held to
16 x qei_joint_reference.WORST_VALUE / WORST_GRAD -- the float64 twin's own distance from its extended-precision twin on these very
cases (tests/test_qei_joint_host.py, which also asserts that every sample's arg-max is unambiguous).  Every comparison prints the share
of the bound the device uses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qei_joint_reference as qj   # noqa: E402
from test_pend_gpu import bohip, make_model   # noqa: E402, F401

pytestmark = pytest.mark.gpu
GRAD_STAGES = ("gemm_U", "qeij_mix", "qeij_grad_finish")
BASE = "se-n129-q5-B27-S70"


def model_of(bohip, ref):
    return make_model(bohip, ref["kern"], ref["X"], ref["y"])


def call(m, ref, Xs=None, **kw):
    kw = {**dict(draws=ref["S"], seed=ref["seed"], tau=ref["tau"], jitter_rel=qj.JITTER_REL), **kw}
    return m.qei_joint((ref["Xs"] if Xs is None else Xs).T, ref["q"], **kw)


@pytest.mark.parametrize("case", list(qj.CASES))
def test_value_and_gradient(bohip, case):
    ref = qj.reference(case)
    m = model_of(bohip, ref)
    m.enable_timing(True)
    value, grad, pivot = call(m, ref)
    labels = [n for n, _ in m.timing()]
    dv, dg = qj.distances(value, grad.T, ref)
    sv, sg = dv / (qj.DEVICE_FACTOR * qj.WORST_VALUE), dg / (qj.DEVICE_FACTOR * qj.WORST_GRAD)
    print(f"{case}: value uses {sv:.3g} of its bound, gradient {sg:.3g}")
    assert not pivot.any() and all(k in labels for k in ("qeij_cov", "qeij_core") + GRAD_STAGES), labels
    v0, g0, _ = call(m, ref, grad=False)                          # the value alone: the same bytes, none of the gradient's stages
    labels = [n for n, _ in m.timing()]
    assert g0 is None and v0.tobytes() == value.tobytes() and not any(k in labels for k in GRAD_STAGES), labels
    assert sv <= 1 and sg <= 1, (case, sv, sg)
    m.close()


def test_determinism_and_a_group_stands_alone(bohip):
    """Two calls: identical bytes.  The groups permuted: the outputs permuted bit for bit.  A group scored alone (B = 1): its bytes
    inside the larger call.  The model is not changed."""
    ref = qj.reference(BASE)
    m, clean = model_of(bohip, ref), model_of(bohip, ref)
    q, Xs = ref["q"], ref["Xs"]
    B, d = len(Xs) // q, Xs.shape[1]
    v, g, _ = call(m, ref)
    v2, g2, _ = call(m, ref)
    assert v.tobytes() == v2.tobytes() and g.tobytes() == g2.tobytes()
    perm = np.random.default_rng(1).permutation(B)
    vp, gp, _ = call(m, ref, Xs.reshape(B, q, d)[perm].reshape(-1, d))
    assert vp.tobytes() == v[perm].tobytes() and gp.T.reshape(B, q, d).tobytes() == g.T.reshape(B, q, d)[perm].tobytes()
    for b in (0, B - 1):
        v1, g1, _ = call(m, ref, Xs[b * q:(b + 1) * q])
        assert v1.tobytes() == v[b:b + 1].tobytes() and g1.T.tobytes() == g.T[b * q:(b + 1) * q].tobytes(), b
    assert m.factor().tobytes() == clean.factor().tobytes() and m.alpha().tobytes() == clean.alpha().tobytes()
    m.close()
    clean.close()


def test_a_repeated_point_flags_its_group_and_no_other(bohip):
    """Two identical points at jitter_rel = 0: pivot > 0, value -Inf, a zero gradient; the neighbours keep their bytes.  And tau above
    every sample: the value 0 and an exactly zero gradient."""
    ref = qj.reference(BASE)
    m = model_of(bohip, ref)
    q, Xs = ref["q"], ref["Xs"].copy()
    v, g, p = call(m, ref, jitter_rel=0.0)
    Xs[q + 3] = Xs[q + 1]                                         # group 1
    vf, gf, pf = call(m, ref, Xs, jitter_rel=0.0)
    assert pf[1] > 0 and vf[1] == -np.inf and not gf[:, q:2 * q].any() and not np.delete(pf, 1).any()
    keep = np.delete(np.arange(len(v)), 1)
    assert vf[keep].tobytes() == v[keep].tobytes() and np.delete(gf, np.s_[q:2 * q], axis=1).tobytes() == np.delete(g, np.s_[q:2 * q], axis=1).tobytes()
    v0, g0, p0 = call(m, ref, tau=1e6)
    assert not v0.any() and not g0.any() and not p0.any()
    m.close()


def test_errors_leave_the_handle_usable(bohip):
    from bohip import _lib

    lib = _lib.load()
    ref = qj.reference("se-n129-q2-B1-S70")
    m = model_of(bohip, ref)
    d = ref["Xs"].shape[1]
    before = m.score("UCB", [2.0], ref["Xs"].T)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    val, Xs = np.empty(4), np.ascontiguousarray(np.random.default_rng(0).random((64, d)))

    def rc(B=1, q=2, S=8, tau=0.0, jit=1e-8, xs=Xs, value=val, h=None):
        return lib.bohip_gp_qei_joint(h or m._h, ptr(xs) if xs is not None else None, B, q, S, 1, tau, jit,
                                      ptr(value) if value is not None else None, None, None, None)

    assert rc(xs=None) == _lib.E_ARG and rc(value=None) == _lib.E_ARG and rc(B=0) == _lib.E_ARG
    assert rc(q=0) == _lib.E_ARG and rc(q=_lib.QEIJ_QMAX + 1) == _lib.E_ARG and rc(S=0) == _lib.E_ARG and rc(S=_lib.QEIJ_SMAX + 1) == _lib.E_ARG
    assert rc(tau=np.inf) == _lib.E_ARG and rc(jit=-1.0) == _lib.E_ARG and rc(jit=np.nan) == _lib.E_ARG
    assert rc(B=2 ** 40) == _lib.E_UNSUPPORTED and b"largest B" in lib.bohip_last_error()
    empty = bohip.ElasticGPE(d, kernel=bohip.SEArd(np.zeros(d), 0.0))
    assert rc(h=empty._h) == _lib.E_STATE
    empty.close()
    sites = bohip.ElasticGPE(d, kernel=bohip.SEArd(np.zeros(d), 0.0), collapse=True)
    sites.append_sites_(ref["X"][:8].T, ref["y"][:8], np.full(8, 2), np.ones(8))
    assert rc(h=sites._h) == _lib.E_UNSUPPORTED
    sites.close()
    assert rc() == 0
    after = m.score("UCB", [2.0], ref["Xs"].T)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(before, after))
    m.close()


def test_ascent(bohip):
    """refine = 4 on a small model: a batch inside the bounds whose joint value, on the climb's seed, is at least the greedy batch's;
    refine = 0 returns the bytes of a call without the key."""
    X, y, _ = qj.synth(60, 2, 1, 3)
    m = make_model(bohip, "SEArd", X, y)
    a, lb, ub, q = bohip.ExpectedImprovement(float(y.max())), np.zeros(2), np.ones(2), 3
    opts = {"method": "qei", "draws": 128, "candidates": 200}
    run = lambda o: bohip.acquire_batch(a, m, lb, ub, q, o, rng=np.random.default_rng(7), setparams=False)   # noqa: E731
    (v0, X0), (vz, Xz), (v4, X4) = run(opts), run(dict(opts, refine=0)), run(dict(opts, refine=4))
    assert v0.tobytes() == vz.tobytes() and X0.tobytes() == Xz.tobytes()
    assert X4.shape == (2, q) and np.all((X4 >= 0) & (X4 <= 1))
    rng = np.random.default_rng(7)                                # the generator's draws, replayed up to the climb's seed
    bohip.utils.latin_hypercube_sampling(lb, ub, 200, rng)
    rng.integers(0, 2 ** 63 - 1)
    for _ in range(3):
        rng.choice(200, size=q, replace=False)
    seed = int(rng.integers(0, 2 ** 63 - 1))
    greedy, climbed = (m.qei_joint(Z, q, 128, seed, tau=a.tau, grad=False)[0][0] for Z in (X0, X4))
    print(f"greedy batch {greedy!r}, climbed {climbed!r} (returned {v4[0]!r})")
    assert X0.shape == (2, q) and climbed == v4[0] and climbed >= greedy
    m.close()
