"""Joint posterior draws without a GPU: the NumPy twin of bohip_gp_sample_joint (tests/joint_reference.py) against an explicit
eigen-decomposition, and the host layer -- acquire_thompson_batch, the "joint" acquisition option, myrand(..., seed=), the 62nd
ABI symbol -- against a fake model."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, synth   # noqa: E402
from joint_reference import (distinct_picks, draw_identity_bound, factor_with_jitter, first_argmax_rows, joint_draws,   # noqa: E402
                             normals, np_thompson_normal)
from matern_reference import MaternGP   # noqa: E402


@pytest.fixture(scope="module")
def bo():
    import bohip

    return bohip


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def test_twin_against_an_eigen_decomposition():
    """Tiny case (N = 40, R = 7): with Sigma = Q diag(w) Q', a draw f = mu + C z has the Mahalanobis length
    (f - mu)' Sigma^-1 (f - mu) = z'z and C C' rebuilds Sigma; the arg-max records are the first maxima."""
    X, y, Xs = synth(40, 2, 7, seed=5)
    gp = MaternGP("Mat52Ard", X, y, np.full(2, -0.4), 0.2, -1.0, 0.1)
    mu, Sigma = gp.predict_cov(Xs)
    F, bv, bi, C, jitter, tries = joint_draws(mu, Sigma, 3, 50)
    assert (jitter, tries) == (0.0, 0) and F.shape == (50, 7)
    w, Q = np.linalg.eigh(Sigma)
    assert w[0] > 0
    np.testing.assert_allclose(C @ C.T, (Q * w) @ Q.T, rtol=0, atol=1e-13 * w[-1])
    Z = normals(3, 50, 7)
    dev = (F - mu) @ Q                                                  # coordinates in the eigenbasis
    np.testing.assert_allclose(np.sum(dev * dev / w, axis=1), np.sum(Z * Z, axis=1), rtol=1e-9 * w[-1] / w[0])
    assert np.all(np.abs(F - (mu + Z @ C.T)) <= draw_identity_bound(mu, C, Z))
    for s in range(50):
        assert bi[s] == int(np.argmax(F[s])) and bv[s] == F[s].max()
    # the generator is keyed by (seed, s, j): rows do not depend on how many are drawn
    np.testing.assert_array_equal(normals(3, 4, 7), Z[:4])
    assert np_thompson_normal(3, 2, np.array([5]))[0] == Z[2, 5]
    z = normals(1, 40, 250).ravel()
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05


def test_twin_jitter_rule():
    Sigma = np.ones((3, 3))                                             # rank one
    with pytest.raises(np.linalg.LinAlgError):
        factor_with_jitter(Sigma, 1e-12, 0)
    with pytest.raises(np.linalg.LinAlgError):
        factor_with_jitter(Sigma - 2 * np.eye(3), 0.0, 40)              # jitter_rel = 0 never makes progress
    C, jitter, tries = factor_with_jitter(Sigma, 1e-12, 40)
    assert tries >= 1 and jitter == pytest.approx(1e-12 * 10.0 ** (tries - 1))
    np.testing.assert_allclose(C @ C.T, Sigma + jitter * np.eye(3), atol=1e-15)
    assert first_argmax_rows(np.array([[1.0, np.nan, 1.0], [np.nan, np.nan, np.nan], [-np.inf, 2.0, 2.0]]))[1].tolist() == [0, -1, 1]


# ---- the greedy distinct-picks rule -----------------------------------------------------------------------------------------
def test_distinct_picks_rule(bo):
    from bohip.acquisition import _distinct_picks

    F = np.array([[1.0, 5.0, 5.0, 0.0],        # tie: the smallest index, 1
                  [0.0, 9.0, 3.0, 3.0],        # 1 is taken -> tie of 2 and 3 -> 2
                  [0.0, 9.0, 8.0, 7.0],        # 1, 2 taken -> 3
                  [np.nan, 9.0, 8.0, 7.0],     # only 0 is left and it is NaN -> nothing
                  [-1.0, 9.0, 8.0, 7.0]])      # 0
    assert _distinct_picks(F).tolist() == [1, 2, 3, -1, 0]
    assert distinct_picks(F).tolist() == [1, 2, 3, -1, 0]
    rng = np.random.default_rng(0)
    G = rng.integers(0, 4, size=(6, 9)).astype(float)                   # many ties
    np.testing.assert_array_equal(_distinct_picks(G), distinct_picks(G))
    assert len(set(_distinct_picks(G).tolist())) == 6
    assert _distinct_picks(np.empty((0, 5))).size == 0


# ---- the host layer against a fake model ------------------------------------------------------------------------------------
class FakeModel:
    """Records the calls; sample_joint hands out draws that all favour candidate 1, then 0, then 2, ... so that the raw winners
    repeat; thompson hands out index 0."""

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

    def predict_cov(self, xs):
        self.calls.append(("predict_cov", np.asarray(xs).shape))
        R = np.asarray(xs).shape[1]
        return np.zeros(R), np.eye(R)

    def score(self, acq, params, xs, want_scores=True):
        self.calls.append(("score", acq, xs.shape))
        return np.zeros(xs.shape[1]), 0.0, 0

    def append_(self, x, y):
        y = np.atleast_1d(y)
        self.calls.append(("append_", y.size))
        self.x = np.asfortranarray(np.concatenate([self.x, np.asarray(x).reshape(self.dim, -1)], axis=1))
        self.y = np.concatenate([self.y, y])

    def thompson(self, xs, S, seed=0, j0=0):
        self.calls.append(("thompson", xs.shape, S, seed))
        return np.zeros(S), np.zeros(S, dtype=np.int64)

    def sample_joint(self, xs, S=1, seed=0, jitter=1e-12, max_tries=40, want_samples=True, want_factor=False):
        from bohip.model import JointSample

        self.calls.append(("sample_joint", xs.shape, S, seed, want_samples))
        R = xs.shape[1]
        pref = np.array([1, 0] + list(range(2, R)))[:R] if R > 1 else np.array([0])
        row = np.empty(R)
        row[pref] = -np.arange(R, dtype=float)                          # the same ranking in every draw
        F = np.tile(row, (S, 1))
        bv, bi = first_argmax_rows(F)
        return JointSample(F if want_samples else None, bv, bi, np.zeros(R), 0.0, 0, None)


def test_acquire_thompson_batch_validation_and_picks(bo):
    m = FakeModel()
    lb, ub = [0.0, 0.0], [1.0, 2.0]
    with pytest.raises(ValueError, match="unknown Thompson batch option"):
        bo.acquire_thompson_batch(m, lb, ub, 2, {"fantasy": "believer"})
    with pytest.raises(ValueError, match="batch size"):
        bo.acquire_thompson_batch(m, lb, ub, 0)
    with pytest.raises(ValueError, match="lowerbounds"):
        bo.acquire_thompson_batch(m, [0.0], ub, 2)
    with pytest.raises(ValueError, match="candidates"):
        bo.acquire_thompson_batch(m, lb, ub, 2, {"candidates": 0})
    with pytest.raises(ValueError, match="must be 2 x R"):
        bo.acquire_thompson_batch(m, lb, ub, 2, {"xs": np.zeros((3, 5))})
    with pytest.raises(ValueError, match="exceeds the 5 candidates"):
        bo.acquire_thompson_batch(m, lb, ub, 6, {"xs": np.zeros((2, 5))})
    with pytest.raises(RuntimeError, match="empty model"):
        bo.acquire_thompson_batch(FakeModel(n=0), lb, ub, 2, {"candidates": 8})

    class NoJoint:
        nobs = 3

    with pytest.raises(NotImplementedError):
        bo.acquire_thompson_batch(NoJoint(), lb, ub, 2, {"candidates": 8})
    assert m.calls == []
    xs = np.asfortranarray(np.random.default_rng(1).random((2, 7)))
    vals, X = bo.acquire_thompson_batch(m, lb, ub, 3, {"xs": xs}, rng=np.random.default_rng(2))
    assert len(m.calls) == 1                                            # ONE sample_joint call with S = q
    kind, shape, S, seed, want = m.calls[0]
    assert (kind, shape, S, want) == ("sample_joint", (2, 7), 3, True) and 0 <= seed < 2 ** 63
    assert np.array_equal(X, xs[:, [1, 0, 2]])                          # every draw prefers 1: the later ones take what is left
    assert vals.tolist() == [0.0, -1.0, -2.0]
    vals, X = bo.acquire_thompson_batch(m, lb, ub, 2, rng=np.random.default_rng(2))     # default: 4096 Latin-hypercube candidates
    assert m.calls[-1][1] == (2, 4096) and X.shape == (2, 2)
    assert np.all(X[1] <= 2.0) and np.all(X >= 0.0)
    # acquire_batch keeps refusing the sampled acquisition
    with pytest.raises(ValueError, match="draws its own batch"):
        bo.acquire_batch(bo.ThompsonSamplingSimple(), m, lb, ub, 2)


def test_joint_option_routes_acquire_max(bo):
    from bohip.acquisition import _check_options

    _check_options({"joint": True, "method": "LN_COBYLA"})
    with pytest.raises(ValueError, match="unknown acquisition option"):
        _check_options({"jointt": True})
    ac = bo.ThompsonSamplingSimple()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = FakeModel()
        f, x = bo.acquire_max(ac, m, [0.0, 0.0], [1.0, 1.0], {"method": "LN_COBYLA", "restarts": 2, "maxeval": 16, "joint": True},
                              rng=np.random.default_rng(0))
        assert [c[0] for c in m.calls] == ["sample_joint", "sample_joint"]
        assert all(c[1] == (2, 16) and c[2] == 1 and c[4] is False for c in m.calls)     # one draw, the winner only
        assert f == 0.0 and x.shape == (2,)
        m = FakeModel()
        bo.acquire_max(ac, m, [0.0, 0.0], [1.0, 1.0], {"method": "LN_COBYLA", "restarts": 2, "maxeval": 16},
                       rng=np.random.default_rng(0))
        assert [c[0] for c in m.calls] == ["thompson", "thompson"]                       # the default is unchanged
        m = FakeModel()
        bo.acquire_max(ac, m, [0.0, 0.0], [1.0, 1.0], {"method": "LN_COBYLA", "restarts": 1, "maxeval": 16, "joint": False},
                       rng=np.random.default_rng(0))
        assert [c[0] for c in m.calls] == ["thompson"]


def test_bopt_batches_route_thompson_to_the_joint_draw(bo):
    m = FakeModel()
    o = bo.BOpt(lambda x: float(np.sum(x)), m, bo.ThompsonSamplingSimple(), bo.NoModelOptimizer(), [0.0, 0.0], [1.0, 1.0],
                maxiterations=2, initializer_iterations=0, verbosity=bo.Silent, rng=np.random.default_rng(0), batchsize=3,
                repetitions=2, batchoptions={"candidates": 32})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bo.boptimize_(o)
    kinds = [c[0] for c in m.calls]
    assert kinds[:4] == ["sample_joint", "append_", "sample_joint", "append_"]
    assert [c[1] for c in m.calls if c[0] == "append_"] == [6, 6]       # 3 points x 2 repetitions, ONE update per iteration
    assert m.calls[0][1:3] == ((2, 32), 3)
    new = m.x[:, 3:9:2]
    assert len({tuple(c) for c in new.T}) == 3                          # distinct points


def test_myrand_seed_routes_to_the_device_draw(bo):
    m = FakeModel()
    X = np.asfortranarray(np.random.default_rng(0).random((2, 5)))
    out = bo.myrand(m, X, seed=7)
    assert m.calls == [("sample_joint", (2, 5), 1, 7, True)] and out.shape == (5,)
    m.calls.clear()
    out = bo.myrand(m, X, np.random.default_rng(0))                     # without a seed: today's host path
    assert m.calls == [("predict_cov", (2, 5))] and out.shape == (5,)
    np.testing.assert_array_equal(out, np.random.default_rng(0).standard_normal(5))      # mu = 0, Sigma = I
    assert isinstance(bo.myrand(m, X[:, 0], np.random.default_rng(0), seed=7), float)    # a vector is one marginal draw, seed or not
    assert m.calls == [("predict_cov", (2, 5))]


# ---- the 62nd symbol ----------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_julia_carry_the_symbol(bo):
    from bohip import _lib

    assert len(_lib.SIGNATURES) == 62 and "bohip_gp_sample_joint" in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "bohip.h")).read()
    decls = set(re.findall(r"\b(bohip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert decls == set(_lib.SIGNATURES)
    jl = open(os.path.join(ROOT, "julia", "BOHip.jl")).read()
    assert "(:bohip_gp_sample_joint, libbohip)" in jl and "function sample_joint(m::AbstractBOHipModel" in jl
    assert "function acquire_thompson_batch(m::AbstractBOHipModel" in jl
