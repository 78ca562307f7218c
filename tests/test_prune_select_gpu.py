"""Pruned arg-max, the bound's inputs and round 1's list (kernels_score.hip "pruned arg-max"): k_kstar's per-wave partial sums of
alpha_j K*'_j that k_prune_bound adds up, k_prune_select (radix select of the 64 highest bounds, ties by ascending index) and the
tail of round 1's finish that lists round 2.

The shapes are the smallest that prune: N = 300 gives 3 row tiles and a bounding prefix of 2 (2 row tiles do not prune); R > 256, or
the small-batch path takes the call.  Every value-only call is followed by bohip_debug_prune_stat >= 0, so no test passes on the
full pass by accident.  A handle that saw more than R / 8 survivors takes the full pass for its next calls: the cases that count
survivors use a handle of their own."""
import ctypes as C

import numpy as np
import pytest

from matern_reference import cov

pytestmark = pytest.mark.gpu

K1 = 64   # round 1's list length (PRUNE_K1)


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def problem(N, d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    return X, y


def model(bohip, X, y, kern="SEArd", ll=np.log(0.5)):
    d = X.shape[1]
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=getattr(bohip, kern)(np.full(d, ll), 0.0), logNoise=-2.0, capacity=len(y))
    m.append_(X.T, y)
    return m


def bounds(m, acq, params, Xs):
    """the pruned pass's upper bounds of the scores (tests-only export of libbohip)"""
    from bohip import _lib

    f = _lib.load().bohip_debug_prune_bounds
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    p = np.zeros(2)
    p[:len(params)] = params
    xs = np.ascontiguousarray(Xs, dtype=np.float64)   # [R][d]: the layout bohip_gp_score takes
    ub = np.empty(len(xs))
    assert f(m._h, _lib.ACQ[acq], p.ctypes.data, xs.ctypes.data, len(xs), ub.ctypes.data) == 0
    return ub


def prune_stat(m):
    """round 2's list length of the handle's last pruned call"""
    from bohip import _lib

    f = _lib.load().bohip_debug_prune_stat
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p]
    return f(m._h)


def value_only(m, acq, params, Xs):
    _, v, i = m.score(acq, params, Xs.T, want_scores=False)
    n2 = prune_stat(m)
    assert n2 >= 0, "the call did not take the pruned pass"
    return v, i, n2


def assert_record(v, i, v_full, i_full, what=None):
    assert i == i_full, (what, i, i_full)
    assert np.float64(v).tobytes() == np.float64(v_full).tobytes(), (what, v, v_full)


# ---- the partial sums out of k_kstar -------------------------------------------------------------------------------------------
# d = 3, 8, 20: k_kstar's dimension buckets 4, 8 and 32; both N have Npad > N (padded columns must add nothing); R = 700 is no multiple
# of 16 or 64: the last k_kstar block and the last bound block are partial
@pytest.mark.parametrize("kern", ["SEArd", "Mat32Ard"])
@pytest.mark.parametrize("N,d", [(300, 3), (300, 8), (300, 20), (450, 4)])
def test_bounds_from_partials_hold_and_repeat(bohip, N, d, kern):
    X, y = problem(N, d, seed=N + d)
    m = model(bohip, X, y, kern)
    rng = np.random.default_rng(N + d + 1)
    Xs = rng.random((700, d))
    Xs[:8] = X[:8]   # sigma^2 = 0 candidates
    for acq, p in [("EI", [y.max()]), ("UCB", [2.0]), ("UCB", [-1.5]), ("MaxMean", [0.0])]:
        sc, v_full, i_full = m.score(acq, p, Xs.T, want_scores=True)
        ub = bounds(m, acq, p, Xs)
        ub2 = bounds(m, acq, p, Xs)
        assert np.isfinite(ub).all(), (acq, p)
        bad = np.flatnonzero(ub < sc)
        assert bad.size == 0, (acq, p, bad[:5], ub[bad[:5]], sc[bad[:5]])
        assert ub.tobytes() == ub2.tobytes(), (acq, p)   # one writer per partial, a fixed order of additions
        v, i, _ = value_only(m, acq, p, Xs)
        assert_record(v, i, v_full, i_full, (acq, p))


@pytest.mark.parametrize("kern", ["SEArd", "Mat32Ard"])
@pytest.mark.parametrize("N,d", [(300, 3), (300, 8), (300, 20), (450, 4)])
def test_mu_tilde_is_the_alpha_dot_product(bohip, N, d, kern):
    # MaxMean with a zero mean: score = the contraction's mu, bound = mu~ + 4 gamma_n S rounded up (n = Npad + 64, S = sum |alpha_j K*'_j|).
    # Both sums lie within gamma_n S of the exact dot product, so 0 <= ub - score <= (4 + 2) gamma_n S + two roundings; 64 n u S caps
    # that with head-room.  A missing or misplaced partial is off by a term of the sum: orders of magnitude more.
    X, y = problem(N, d, seed=N + d)
    m = model(bohip, X, y, kern)
    Xs = np.random.default_rng(N + d + 1).random((700, d))
    sc, _, _ = m.score("MaxMean", [0.0], Xs.T, want_scores=True)
    ub = bounds(m, "MaxMean", [0.0], Xs)
    S = np.abs(m.alpha()) @ np.abs(cov(kern, X, Xs, np.full(d, np.log(0.5)), 0.0))
    n = (N + 1 + 127) // 128 * 128 + 64
    gap = ub - sc
    print(f"N={N} d={d} {kern}: max (ub - score) / (n u S) = {(gap / (n * 2.0 ** -53 * S)).max():.2f}, min gap = {gap.min():.3e}")
    assert (gap >= 0.0).all(), gap.min()
    assert (gap <= 64 * n * 2.0 ** -53 * S).all(), (gap / (n * 2.0 ** -53 * S)).max()


# ---- the selection against a NumPy model ----------------------------------------------------------------------------------------
def expected_round2(ub, sc):
    """(round 1's set, the survivors outside it): the first min(64, R) in (bound desc, index asc), L = the best score among them"""
    R = len(ub)
    order = np.lexsort((np.arange(R), -np.where(np.isnan(ub), np.inf, ub)))
    first = order[:min(K1, R)]
    L = sc[first].max()
    outside = np.ones(R, bool)
    outside[first] = False
    return first, int(np.count_nonzero(outside & ~(ub < L)))


def check_selection(m, acq, p, Xs):
    sc, v_full, i_full = m.score(acq, p, Xs.T, want_scores=True)
    ub = bounds(m, acq, p, Xs)
    assert np.isfinite(ub).all() and not (ub < sc).any()
    first, n2 = expected_round2(ub, sc)
    v, i, n2_dev = value_only(m, acq, p, Xs)
    print(f"R={len(Xs)} {acq}: round 2 lists {n2_dev}, the model {n2}")
    assert n2_dev == n2, (acq, len(Xs), n2_dev, n2)
    assert_record(v, i, v_full, i_full, (acq, len(Xs)))
    assert i == int(np.argmax(sc))   # first maximum
    return first


@pytest.fixture(scope="module")
def small(bohip):
    return problem(300, 4, seed=21)


@pytest.mark.parametrize("R", [257, 700, 4099, 8192])   # 1 to 8 keys a thread; 8192 is the select kernel's limit
@pytest.mark.parametrize("acq", ["EI", "UCB"])
def test_selection_small(bohip, small, R, acq):
    X, y = small
    Xs = np.random.default_rng(R).random((R, 4))
    check_selection(model(bohip, X, y), acq, [y.max()] if acq == "EI" else [2.0], Xs)


def test_selection_bench_shape(bohip):
    X, y = problem(3000, 8)
    Xs = np.random.default_rng(1).random((4096, 8))
    check_selection(model(bohip, X, y), "EI", [y.max()], Xs)


@pytest.mark.parametrize("R", [700, 4099])
def test_ties_through_the_threshold(bohip, small, R):
    X, y = small
    rng = np.random.default_rng(R + 1)
    Xs = rng.random((R, 4))
    # the highest bound shared by 200 copies of one point: round 1's list ends inside the tie.  There is no export of the device's
    # list: `first` below is the NumPy model's, and its assertion checks the model (the 64 lowest indices of the tie).  What the
    # device is held to is a full list of 64 (an overfull or underfull one changes the survivor count), the survivor count and
    # the record with the lowest index as the winner; the tied candidates share bound and score, so WHICH 64 of the tie the device
    # lists does not show here.
    m = model(bohip, X, y)
    ub = bounds(m, "UCB", [2.0], Xs)
    top = int(np.argmax(ub))
    copies = np.sort(rng.choice(np.setdiff1d(np.arange(R), [top]), 199, replace=False))
    Xs[copies] = Xs[top]
    first = check_selection(model(bohip, X, y), "UCB", [2.0], Xs)
    tie = np.sort(np.append(copies, top))
    assert np.array_equal(np.sort(first), tie[:K1])
    # all but 10 candidates identical: whichever way the threshold falls, the winner is the lowest index of its value
    Xs2 = np.tile(Xs[5], (R, 1))
    other = np.sort(rng.choice(np.arange(1, R), 10, replace=False))
    Xs2[other] = rng.random((10, 4))
    for acq, p in [("UCB", [2.0]), ("EI", [y.max()])]:
        check_selection(model(bohip, X, y), acq, p, Xs2)


def test_batch_size_changes_between_calls(bohip, small):
    # the scratch layout follows the batch and now holds the partials: consecutive calls of different sizes on one handle
    X, y = small
    m = model(bohip, X, y)
    Xs = np.random.default_rng(6).random((8192, 4))
    for R in (8192, 300, 4099):
        _, v_full, i_full = m.score("EI", [y.max()], Xs[:R].T, want_scores=True)
        v, i, _ = value_only(m, "EI", [y.max()], Xs[:R])
        assert_record(v, i, v_full, i_full, R)
