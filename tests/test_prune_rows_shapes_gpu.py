"""Shapes of the row-split exact rounds (k_trigemm_rows) and of their finish (k_prune_finish) that the other pruning tests do not reach:
candidate lists that end inside a column group of 8, contraction extents shorter than the operand ring and than the fragment
prefetch (T = 2: halves of 4 and 8 chunks), the solo upper half at T = 3, value-only records of small and odd batches against the
full pass, repeated calls on one handle, and a tau sweep whose round 2 is once empty, once short (row-split) and once long.

Everything is compared bit for bit: path 1 of the tests-only export bohip_debug_trigemm_partials (k_trigemm_rows over every row
tile) against path 0 (k_trigemm_sq), and the record of a value-only call against the record of the full pass.  Which path a
value-only call takes is the library's choice: at N = 450 batches of up to 256 candidates take the small-batch pass, R = 300 prunes
with a round-2 launch sized for 236 candidates (the row-split kernel alone) and R = 321 with both round-2 launches enqueued; at
N = 3000 batches below 1345 candidates take the split-K pass, so the cases that must prune there use 1400 candidates or more."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_models = {}


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    yield b
    _models.clear()


def make_model(bohip, N, seed, d=8):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
    m.append_(X.T, y)
    return m, X, y


def model(bohip, N):
    """One model per N for the tests that only read it (a handle remembers how its last pruned call went and may answer the next
    value-only calls with the full pass: tests that must prune build their own)."""
    if N not in _models:
        _models[N] = make_model(bohip, N, 1000 + N)
    return _models[N]


def candidates(N, R, X, d=8):
    Xs = np.random.default_rng(7 * N + R).random((R, d))
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


def record(m, acq, p, Xs, want_scores):
    _, v, i = m.score(acq, p, Xs.T, want_scores=want_scores)
    return int(i), np.float64(v).tobytes()


@pytest.mark.parametrize("N,R", [(N, R) for N in (200, 300, 450) for R in (1, 7, 8, 9, 15, 17, 63, 65)] + [(3000, 65)])
def test_partial_column_groups_bit_exact(bohip, N, R):
    m, X, y = model(bohip, N)
    Xs = candidates(N, R, X)
    q0, mu0 = run_partials(m, N, Xs, 0)
    q1, mu1 = run_partials(m, N, Xs, 1)
    assert np.isfinite(q0).all() and np.isfinite(mu0).all()
    assert_bits(q1, q0)
    assert_bits(mu1, mu0)


def fresh(bohip, N):
    """A handle of its own: its first value-only call cannot be answered by the back-off (see model())."""
    return make_model(bohip, N, 1000 + N)


def prunes(N, R):
    return (N == 450 and R > 256) or (N == 3000 and R >= 1400)


@pytest.mark.parametrize("acq", ["EI", "UCB"])
@pytest.mark.parametrize("N,R", [(450, 1), (450, 63), (450, 64), (450, 65), (450, 100), (450, 321), (450, 300), (3000, 1400)])
def test_value_only_record_is_the_full_pass(bohip, N, R, acq):
    m, X, y = fresh(bohip, N)
    Xs = candidates(N, R, X)
    p = [y.max()] if acq == "EI" else [2.0]
    got = record(m, acq, p, Xs, False)          # first: the handle has no history
    if prunes(N, R):
        assert prune_stat(m) >= 0               # the pruned pass ran (it owns the word); the smaller batches take the small-batch pass
    assert got == record(m, acq, p, Xs, True)


@pytest.mark.parametrize("N,R", [(450, 321), (450, 300), (3000, 1400)])
def test_duplicated_candidates_lowest_index_wins(bohip, N, R):
    # the winner 69 times over: the same bound and the same score bits at 69 indices.  Round 1 holds at most 64 of them and every
    # copy outside it has bound >= score = L, so at least 5 go through round 2; the lowest index must come out of the finishes
    m, X, y = fresh(bohip, N)
    Xs = candidates(N, R, X)
    p = [y.max()]
    i_best, _ = record(m, "EI", p, Xs, True)
    dup = sorted(set(np.random.default_rng(R).choice(R, 68, replace=False).tolist()) | {i_best})
    Xs[dup] = Xs[i_best]
    got = record(m, "EI", p, Xs, False)
    n2 = prune_stat(m)
    print("round-2 survivors:", n2)
    assert n2 >= len(dup) - 64, n2
    full = record(m, "EI", p, Xs, True)
    assert full[0] == dup[0]
    assert got == full


def test_repeated_calls_carry_nothing_over(bohip):
    m, X, y = make_model(bohip, 3000, 31)
    p = [y.max()]
    A, B = candidates(3000, 2048, X), candidates(3000, 1400, X)
    a_full, b_full = record(m, "EI", p, A, True), record(m, "EI", p, B, True)
    for Xs, full in ((A, a_full), (A, a_full), (B, b_full), (A, a_full)):
        assert record(m, "EI", p, Xs, False) == full
        assert 0 <= prune_stat(m) <= len(Xs) // 8   # pruned, and few enough survivors that the next call prunes too
    qa, mua = run_partials(m, 3000, A[:65], 1)
    qb, mub = run_partials(m, 3000, B[:9], 1)
    qa2, mua2 = run_partials(m, 3000, A[:65], 1)
    qb0, mub0 = run_partials(m, 3000, B[:9], 0)
    assert_bits(qa2, qa)
    assert_bits(mua2, mua)
    assert_bits(qb, qb0)
    assert_bits(mub, mub0)


def test_tau_sweep_empty_short_and_long_round2(bohip):
    # the model, candidates and tau values of test_prune_rows_gpu.py's sweep, known to leave 1 ... 256 survivors outside round 1 at
    # some steps.  tau rises, so the long lists come last: after a list longer than R / 8 the handle answers the next value-only
    # calls with the full pass and clears the word, so what is read after that says nothing about round 2
    m, X, y = make_model(bohip, 3000, 21)
    Xs = np.random.default_rng(22).random((4096, 8))
    seen = []
    for dt in [-0.5, -0.2, 0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.2, 2.0]:
        p = [y.max() + dt]
        full = record(m, "EI", p, Xs, True)
        got = record(m, "EI", p, Xs, False)
        if not seen or seen[-1] <= 4096 // 8:
            seen.append(prune_stat(m))
        assert got == full, (dt, seen)
    print("round-2 survivors per pruned call:", seen)
    assert any(n == 0 for n in seen), seen
    assert any(1 <= n <= 256 for n in seen), seen
    assert any(n > 256 for n in seen), seen
