"""Pruned arg-max (value-only scoring, kernels_score.hip "pruned arg-max"): the record of a call that returns no scores must equal,
bit for bit, the arg-max record of the same call with scores -- which runs the full pass.  Covers every functor (UCB also with a
negative kappa), 1 ... 4 row tiles with N off the 128 grid, duplicated candidates (index tie-break), candidates on observations
(sigma^2 = 0), a problem where nothing can be pruned (d = 16, unit length scales) and the bench's own shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def problem(N, d, seed=0, ll=np.log(0.5)):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    return X, y, np.full(d, ll)


def model(bohip, X, y, ll):
    m = bohip.ElasticGPE(X.shape[1], mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(ll, 0.0), logNoise=-2.0, capacity=len(y))
    m.append_(X.T, y)
    return m


def assert_same_record(m, acq, params, Xs):
    sc, v_full, i_full = m.score(acq, params, Xs.T, want_scores=True)
    _, v, i = m.score(acq, params, Xs.T, want_scores=False)
    assert i == i_full, (acq, i, i_full)
    assert np.float64(v).tobytes() == np.float64(v_full).tobytes(), (acq, v, v_full)
    assert i == int(np.nanargmax(np.where(np.isnan(sc), -np.inf, sc)))   # first maximum: the reference's strict '>'


@pytest.fixture(scope="module")
def bench_model(bohip):
    X, y, ll = problem(3000, 8)
    return model(bohip, X, y, ll), X, y


ACQS = [("EI", None), ("PI", None), ("UCB", [2.0]), ("UCB", [-1.5]), ("MI", [2.0, 0.3]), ("MaxMean", [0.0])]


@pytest.mark.parametrize("acq,params", ACQS)
def test_functors_bench_shape(bench_model, acq, params):
    m, X, y = bench_model
    rng = np.random.default_rng(1)
    Xs = rng.random((4096, 8))
    assert_same_record(m, acq, params if params is not None else [y.max()], Xs)


@pytest.mark.parametrize("N", [100, 200, 300, 450])
@pytest.mark.parametrize("acq", ["EI", "UCB"])
def test_row_tiles_1_to_4(bohip, N, acq):
    X, y, ll = problem(N, 4, seed=N)
    m = model(bohip, X, y, ll)
    Xs = np.random.default_rng(N + 1).random((3000, 4))
    assert_same_record(m, acq, [y.max()] if acq == "EI" else [1.0], Xs)


def test_duplicates_and_observations(bench_model):
    m, X, y = bench_model
    rng = np.random.default_rng(2)
    Xs = rng.random((4096, 8))
    Xs[100:4096:37] = Xs[99]           # many copies of one candidate: the lowest index must win a tie
    Xs[2000:2100] = X[:100]            # candidates on observations: sigma^2 clamps to 0
    for acq, p in [("EI", [y.max()]), ("UCB", [2.0]), ("MaxMean", [0.0]), ("PI", [y.max() - 0.5])]:
        assert_same_record(m, acq, p, Xs)
    # the winner itself duplicated ahead of its first position
    _, _, i = m.score("EI", [y.max()], Xs.T, want_scores=False)
    Xs2 = Xs.copy()
    Xs2[i + 1:] = Xs[i]
    assert_same_record(m, "EI", [y.max()], Xs2)


def test_no_prune_problem(bohip):
    X, y, ll = problem(3000, 16, seed=3, ll=0.0)
    m = model(bohip, X, y, ll)
    Xs = np.random.default_rng(4).random((4096, 16))
    assert_same_record(m, "EI", [y.max()], Xs)


@pytest.mark.parametrize("seed", [5, 7])
def test_other_seeds(bohip, seed):
    X, y, ll = problem(3000, 8, seed=seed)
    m = model(bohip, X, y, ll)
    Xs = np.random.default_rng(seed + 100).random((4096, 8))
    assert_same_record(m, "EI", [y.max()], Xs)
    assert_same_record(m, "UCB", [2.0], Xs)


def test_batch_size_changes_between_calls(bench_model):
    # the scratch layout follows the batch: consecutive calls of different sizes on one handle (as logical shards do)
    m, X, y = bench_model
    Xs = np.random.default_rng(6).random((4099, 8))
    for R in (4099, 4096, 513, 512, 3000, 4099):
        assert_same_record(m, "EI", [y.max()], Xs[:R])


def bounds(m, acq, params, Xs):
    """the pruned pass's upper bounds of the scores (tests-only export of libbohip)"""
    import ctypes as C
    from bohip import _lib

    lib = _lib.load()
    f = lib.bohip_debug_prune_bounds
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    p = np.zeros(2)
    p[:len(params)] = params
    xs = np.ascontiguousarray(Xs, dtype=np.float64)   # [R][d]: the layout bohip_gp_score takes
    ub = np.empty(len(xs))
    assert f(m._h, _lib.ACQ[acq], p.ctypes.data, xs.ctypes.data, len(xs), ub.ctypes.data) == 0
    return ub


BOUND_CASES = ACQS + [("EI", [10.0]), ("PI", [10.0]), ("PI", [-10.0]), ("MI", [-1.0, 0.5])]


@pytest.mark.parametrize("acq,params", BOUND_CASES)
def test_bound_holds_for_every_candidate(bench_model, acq, params):
    # exactness rests on bound >= the full pass's computed score for EVERY candidate, not only the winner
    m, X, y = bench_model
    rng = np.random.default_rng(8)
    Xs = rng.random((4096, 8))
    Xs[:64] = X[:64]                          # sigma^2 = 0 candidates
    Xs[64:128] = X[:64] + 1e-3 * rng.standard_normal((64, 8))
    p = params if params is not None else [y.max()]
    sc, _, _ = m.score(acq, p, Xs.T, want_scores=True)
    ub = bounds(m, acq, p, Xs)
    bad = np.flatnonzero(ub < sc)
    assert bad.size == 0, (acq, bad[:5], ub[bad[:5]], sc[bad[:5]])
    assert np.isfinite(ub).all()


def test_bound_holds_when_the_winner_is_not_first_by_bound(bohip):
    # many candidates far from the data: large variance, high bound, low mean -- the winner need not rank first by bound, and
    # every candidate whose bound reaches the best score must be scored
    X, y, ll = problem(3000, 8, seed=11)
    m = model(bohip, X, y, ll)
    rng = np.random.default_rng(12)
    Xs = np.concatenate([rng.random((2048, 8)) * 0.2 + 0.8, rng.random((2048, 8))])
    for acq, p in [("EI", [y.max()]), ("UCB", [3.0]), ("PI", [y.max()])]:
        sc, _, _ = m.score(acq, p, Xs.T, want_scores=True)
        ub = bounds(m, acq, p, Xs)
        assert not (ub < sc).any(), acq
        assert_same_record(m, acq, p, Xs)


def test_problem_that_prunes_nothing_repeated(bohip):
    # tau far above the data: every EI is 0 (or nearly), nothing prunes; after one pruned call the handle keeps the full pass for a
    # while and then tries again -- the record is the full pass's on every call
    X, y, ll = problem(3000, 8, seed=13)
    m = model(bohip, X, y, ll)
    Xs = np.random.default_rng(14).random((4096, 8))
    for _ in range(20):
        assert_same_record(m, "EI", [y.max() + 100.0], Xs)
        assert_same_record(m, "EI", [y.max() + 2.0], Xs)
