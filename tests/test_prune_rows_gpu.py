"""Row-split exact rounds of the pruned arg-max (k_trigemm_rows, kernels_score.hip): the kernel must reproduce k_trigemm_sq's partial
sums q[2t + h][r] and mu_raw[r] bit for bit -- the pruning proof rests on round 1's best being a score the full pass computes.  Checked
over every row tile (tests-only export bohip_debug_trigemm_partials) for whole last tiles, the solo upper half, T = 2 ... 79 and an
ill-conditioned model; and the record of calls whose round 2 runs on the new kernel (1 ... 256 survivors) against the full pass."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def model(bohip, N, d, seed, ll=np.log(0.5), lsig=0.0, lnoise=-2.0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, ll), lsig), logNoise=lnoise, capacity=N)
    m.append_(X.T, y)
    return m, X, y


def run_partials(m, N, Xs, path):
    from bohip import _lib

    lib = _lib.load()
    f = lib.bohip_debug_trigemm_partials
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    xs = np.ascontiguousarray(Xs, dtype=np.float64)   # [R][d]
    T = (N + 1 + 127) // 128
    q = np.full((2 * T, len(xs)), np.nan)
    mu = np.full(len(xs), np.nan)
    assert f(m._h, xs.ctypes.data, len(xs), path, q.ctypes.data, mu.ctypes.data) == 0
    return q, mu


def assert_bits(a, b):
    bad = np.flatnonzero(a.view(np.uint64).ravel() != b.view(np.uint64).ravel())
    assert bad.size == 0, (bad.size, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])


@pytest.mark.parametrize("N,d", [(200, 8), (1000, 8), (2943, 8), (2999, 8), (3000, 8), (3050, 8), (4900, 8), (6000, 8),
                                 (10000, 16)])
def test_partials_bit_exact(bohip, N, d):
    m, X, y = model(bohip, N, d, seed=N)
    Xs = np.random.default_rng(N + 1).random((1000, d))
    Xs[:50] = X[:50]                                      # candidates on observations
    q0, mu0 = run_partials(m, N, Xs, 0)
    q1, mu1 = run_partials(m, N, Xs, 1)
    assert np.isfinite(q0).all() and np.isfinite(mu0).all()
    assert_bits(q1, q0)
    assert_bits(mu1, mu0)


@pytest.mark.parametrize("lsig,lnoise", [(5.0, 0.0), (0.0, -7.0)])
def test_partials_bit_exact_stress(bohip, lsig, lnoise):
    m, X, y = model(bohip, 2000, 2, seed=5, ll=np.log(0.3), lsig=lsig, lnoise=lnoise)
    Xs = np.random.default_rng(6).random((777, 2))
    q0, mu0 = run_partials(m, 2000, Xs, 0)
    q1, mu1 = run_partials(m, 2000, Xs, 1)
    assert_bits(q1, q0)
    assert_bits(mu1, mu0)


def prune_stat(m):
    from bohip import _lib

    f = _lib.load().bohip_debug_prune_stat
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p]
    return f(m._h)


def test_round2_on_the_row_split_kernel(bohip):
    # tau sweeps from below the data to far above it: the number of candidates that survive outside round 1 grows from none to
    # most of the batch; the record must be the full pass's at every step, and some steps must run round 2 on k_trigemm_rows
    # (1 ... 256 survivors) and some on k_trigemm_sq (more)
    m, X, y = model(bohip, 3000, 8, seed=21)
    Xs = np.random.default_rng(22).random((4096, 8))
    seen = []
    for dt in [-0.5, -0.2, 0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.2, 2.0]:
        p = [y.max() + dt]
        sc, v_full, i_full = m.score("EI", p, Xs.T, want_scores=True)
        _, v, i = m.score("EI", p, Xs.T, want_scores=False)
        n2 = prune_stat(m)
        seen.append(n2)
        assert i == i_full, (dt, n2, i, i_full)
        assert np.float64(v).tobytes() == np.float64(v_full).tobytes(), (dt, n2, v, v_full)
    for kappa in [0.5, 1.0, 2.0, 4.0, 8.0]:
        _, v_full, i_full = m.score("UCB", [kappa], Xs.T, want_scores=True)
        _, v, i = m.score("UCB", [kappa], Xs.T, want_scores=False)
        n2 = prune_stat(m)
        seen.append(n2)
        assert (i, np.float64(v).tobytes()) == (i_full, np.float64(v_full).tobytes()), (kappa, n2)
    print("round-2 survivors per call:", seen)
    assert any(1 <= n <= 256 for n in seen), seen
