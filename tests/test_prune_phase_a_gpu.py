"""Phase A of the pruned arg-max as 64-row jobs (k_trigemm_sq_pa, kernels_score.hip): every whole row piece with rt < m is cut into
its two 64-row halves, each a workgroup of its own in the loop's whole mode.  The partial sums q[2t + h][r], t < m, must be
k_trigemm_sq's bit for bit -- the bounds, the select and both exact rounds read them.  Path 3 of the tests-only export
bohip_debug_trigemm_partials is the phase-A launch exactly as pruned_pass enqueues it (same table, grid and m); path 0 is the full
pass's k_trigemm_sq.  Compared as uint64 views.  The records of value-only calls that take the pruned pass are compared with the full
pass's, value and index, and the length of round 2's list (bohip_debug_prune_stat) with the figure the whole-tile phase A left for
the same inputs (PARENT_STAT: recorded on the commit before the 64-row jobs, same seeds)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_models = {}

# (N, d) -> (T, m): m = the smallest m >= 2 with m (m + 1) >= 0.02 T (T + 1)  (prune_tiles in bohip.hip)
SHAPES = {(300, 2): (3, 2), (1100, 3): (9, 2), (3000, 8): (24, 3), (5000, 16): (40, 6)}
# R = 64: one candidate tile; 200: a last tile of 8 live columns, 4 tiles < 8 XCD slots; 520: 9 tiles, one XCD owns two; 1000
CASES = [(N, d, R) for (N, d) in SHAPES for R in (64, 200, 520, 1000)] + [(3000, 8, 4096)]


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    yield b
    _models.clear()


def make_model(bohip, N, d, seed, kernel=None, ll=np.log(0.5), lsig=0.0, lnoise=-2.0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    k = (kernel or bohip.SEArd)(np.full(d, ll), lsig)
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=k, logNoise=lnoise, capacity=N)
    m.append_(X.T, y)
    return m, X, y


def model(bohip, N, d):
    """One model per shape for the tests that only read q (the export does not touch the handle's pruning history)."""
    if (N, d) not in _models:
        _models[(N, d)] = make_model(bohip, N, d, 500 + N)
    return _models[(N, d)]


def candidates(N, d, R, X):
    Xs = np.random.default_rng(11 * N + R).random((R, d))
    Xs[: min(3, R)] = X[: min(3, R)]   # candidates on observations
    return Xs


def run_partials(m, N, Xs, path):
    from bohip import _lib

    f = _lib.load().bohip_debug_trigemm_partials
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    xs = np.ascontiguousarray(Xs, dtype=np.float64)   # [R][d]
    T = (N + 1 + 127) // 128
    q = np.full((2 * T, len(xs)), np.nan)
    mu = np.full(len(xs), np.nan)
    assert f(m._h, xs.ctypes.data, len(xs), path, q.ctypes.data, mu.ctypes.data) == 0
    return q, mu


def prune_stat(m):
    from bohip import _lib

    f = _lib.load().bohip_debug_prune_stat
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p]
    return f(m._h)


def assert_bits(a, b):
    bad = np.flatnonzero(a.view(np.uint64).ravel() != b.view(np.uint64).ravel())
    assert bad.size == 0, (bad.size, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])


def check_phase_a(m, N, Xs, m_tiles):
    q0, _ = run_partials(m, N, Xs, 0)
    q3, _ = run_partials(m, N, Xs, 3)
    assert np.isfinite(q0).all()
    assert (q0[: 2 * m_tiles] > 0.0).all()          # every half of the prefix holds live rows: a slot left unwritten would show
    assert_bits(q3[: 2 * m_tiles], q0[: 2 * m_tiles])
    assert not q3[2 * m_tiles:].view(np.uint64).any()   # the rows phase A does not own come back as zeros


@pytest.mark.parametrize("N,d,R", CASES)
def test_phase_a_partials_bit_exact(bohip, N, d, R):
    T, m_tiles = SHAPES[(N, d)]
    assert T == (N + 1 + 127) // 128
    m, X, y = model(bohip, N, d)
    check_phase_a(m, N, candidates(N, d, R, X), m_tiles)


@pytest.mark.parametrize("lsig,lnoise", [(5.0, 0.0), (0.0, -7.0)])
def test_phase_a_partials_bit_exact_stress(bohip, lsig, lnoise):
    # the ill-conditioned models of test_prune_rows_gpu.py: T = 16, m = 2
    m, X, y = make_model(bohip, 2000, 2, seed=5, ll=np.log(0.3), lsig=lsig, lnoise=lnoise)
    check_phase_a(m, 2000, np.random.default_rng(6).random((777, 2)), 2)


def test_phase_a_partials_bit_exact_matern32(bohip):
    m, X, y = make_model(bohip, 1100, 3, seed=77, kernel=bohip.Mat32Ard)
    check_phase_a(m, 1100, candidates(1100, 3, 1000, X), 2)


# round 2's list length of the first value-only call of a fresh handle, with whole-tile phase-A jobs (the parent commit)
PARENT_STAT = {
    (300, 2, "EI"): 4032, (300, 2, "UCB"): 0,      # (EI ~ 1e-17 at tau = max y: below the bound's slack, everybody survives)
    (1100, 3, "EI"): 4032, (1100, 3, "UCB"): 0,
    (3000, 8, "EI"): 0, (3000, 8, "UCB"): 0,
}
RECORD_R = 4096


@pytest.mark.parametrize("acq", ["EI", "UCB"])
@pytest.mark.parametrize("N,d", [(300, 2), (1100, 3), (3000, 8)])
def test_value_only_record_is_the_full_pass(bohip, N, d, acq):
    m, X, y = make_model(bohip, N, d, 500 + N)      # a handle of its own: no pruning history, the first value-only call prunes
    Xs = candidates(N, d, RECORD_R, X)
    p = [y.max()] if acq == "EI" else [2.0]
    _, v, i = m.score(acq, p, Xs.T, want_scores=False)
    stat = prune_stat(m)
    print(f"N={N} d={d} R={len(Xs)} {acq}: round-2 list {stat}, best {v!r} @ {i}")
    assert stat >= 0                                # the pruned pass ran (it owns the word)
    assert stat == PARENT_STAT[(N, d, acq)]
    _, v_full, i_full = m.score(acq, p, Xs.T, want_scores=True)
    assert int(i) == int(i_full)
    assert np.float64(v).tobytes() == np.float64(v_full).tobytes()
