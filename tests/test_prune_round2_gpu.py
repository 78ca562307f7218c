"""Pruned arg-max with the rounds finished inside k_trigemm_rows (its last arriver runs the finish) and round 2 as ONE launch whose
workgroups loop over the column groups (the steady form), against the long form (gather, k_trigemm_sq, k_trigemm_rows up to 256
candidates, k_prune_finish) -- tests-only export bohip_debug_prune_round2_form: -1 the library's rule, 0 steady, 1 long.

Everything is compared bit for bit with the full pass (the record of the same call with want_scores=True), and after every value-only
call that must prune the pinned word (bohip_debug_prune_stat: round 2's list length) is >= 0, so no test passes on the full pass.
Every model is on a handle of its own: a handle that saw a long list answers its next value-only calls with the full pass.

Round-2 lists of a wanted length come from duplicating the winner: k copies share one bound and one score, round 1 holds at most 64
of them and every copy outside it has bound >= score = L, so the list has at least k - 64 entries.  One pass of the steady
form's grid is 8 column groups of 8 candidates = 64 entries.  Shapes: N = 450 (T = 4, m = 2) with 300 and 321 candidates -- the sizes
at which a value-only call prunes there -- and N = 3000 with 1400."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID_PASS = 64   # candidates in one pass of the steady form's grid
ROWS_CAP = 256   # the long form's k_trigemm_rows takes lists up to this length


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def fresh(bohip, N, seed=None, d=8):
    rng = np.random.default_rng(1000 + N if seed is None else seed)
    X = rng.random((N, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
    m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=bohip.SEArd(np.full(d, np.log(0.5)), 0.0), logNoise=-2.0, capacity=N)
    m.append_(X.T, y)
    return m, X, y


def candidates(N, R, X, d=8):
    Xs = np.random.default_rng(7 * N + R).random((R, d))
    Xs[: min(3, R)] = X[: min(3, R)]   # candidates on observations
    return Xs


def _lib():
    from bohip import _lib as L

    return L.load()


def prune_stat(m):
    f = _lib().bohip_debug_prune_stat
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p]
    return f(m._h)


def set_form(m, form):
    f = _lib().bohip_debug_prune_round2_form
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int]
    assert f(m._h, form) == 0


def prune_bounds(m, p, Xs):
    f = _lib().bohip_debug_prune_bounds
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    par = np.asarray(p, dtype=np.float64)
    ub = np.full(len(xs), np.nan)
    assert f(m._h, 0, par.ctypes.data, xs.ctypes.data, len(xs), ub.ctypes.data) == 0   # (0: EI)
    return ub


def run_partials(m, N, Xs, path):
    f = _lib().bohip_debug_trigemm_partials
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    xs = np.ascontiguousarray(Xs, dtype=np.float64)
    T = (N + 1 + 127) // 128
    q = np.full((2 * T, len(xs)), np.nan)
    mu = np.full(len(xs), np.nan)
    assert f(m._h, xs.ctypes.data, len(xs), path, q.ctypes.data, mu.ctypes.data) == 0
    return q, mu


def assert_bits(a, b):
    bad = np.flatnonzero(a.view(np.uint64).ravel() != b.view(np.uint64).ravel())
    assert bad.size == 0, (bad.size, bad[:5], a.ravel()[bad[:5]], b.ravel()[bad[:5]])


def record(m, acq, p, Xs, want_scores):
    _, v, i = m.score(acq, p, Xs.T, want_scores=want_scores)
    return int(i), np.float64(v).tobytes()


def params(acq, y, dt=0.0):
    return [y.max() + dt] if acq == "EI" else [2.0]


def with_copies(bohip, N, R, acq, k):
    """Candidates with the winner of the call at k indices (the winner's own among them), the parameters, the indices."""
    m, X, y = fresh(bohip, N)
    Xs = candidates(N, R, X)
    p = params(acq, y)
    i_best, _ = record(m, acq, p, Xs, True)
    dup = sorted(set(np.random.default_rng(R + k).choice(R, k - 1, replace=False).tolist()) | {i_best})
    while len(dup) < k:   # (the draw held the winner's index)
        dup = sorted(set(dup) | {next(i for i in range(R) if i not in dup)})
    Xs[dup] = Xs[i_best]
    return Xs, p, dup


def both_forms(bohip, N, acq, p, Xs):
    """The value-only record under either form, each on a handle of its own, against the full pass; returns the words."""
    words = []
    for form in (0, 1):
        m, X, y = fresh(bohip, N)
        set_form(m, form)
        full = record(m, acq, p, Xs, True)
        got = record(m, acq, p, Xs, False)
        w = prune_stat(m)
        assert w >= 0, (form, w)
        assert got == full, (form, w, got, full)
        words.append(w)
    print(f"N={N} R={len(Xs)} {acq}: round 2's list length under the forms 0 / 1: {words}")
    assert words[0] == words[1], words
    return words[0], full


# k copies of the winner: the list ends inside the first column group (>= 1), crosses a group boundary (>= 9), is longer than one
# pass of the grid (>= 65)
@pytest.mark.parametrize("acq", ["EI", "UCB"])
@pytest.mark.parametrize("k", [65, 73, 64 + GRID_PASS + 1])
@pytest.mark.parametrize("N,R", [(450, 300), (450, 321)])
def test_lists_of_intermediate_length(bohip, N, R, acq, k):
    Xs, p, dup = with_copies(bohip, N, R, acq, k)
    w, full = both_forms(bohip, N, acq, p, Xs)
    assert w >= k - 64, (w, k)
    assert full[0] == dup[0]          # the lowest index wins


# above the long form's cap: the one case at N = 3000
@pytest.mark.parametrize("acq", ["EI", "UCB"])
def test_list_above_the_rows_cap(bohip, acq):
    k = 64 + ROWS_CAP + 9
    Xs, p, dup = with_copies(bohip, 3000, 1400, acq, k)
    w, full = both_forms(bohip, 3000, acq, p, Xs)
    assert w > ROWS_CAP and w >= k - 64, (w, k)
    assert full[0] == dup[0]


# every candidate outside round 1 is listed: EI with tau = max y + 100 (every score and every bound is 0 or its slack: nothing is
# pruned); UCB on a batch of copies of one point (one bound, one score)
@pytest.mark.parametrize("acq", ["EI", "UCB"])
@pytest.mark.parametrize("N,R", [(450, 300), (450, 321)])
def test_everything_outside_round_1_listed(bohip, N, R, acq):
    m, X, y = fresh(bohip, N)
    Xs = candidates(N, R, X)
    if acq == "UCB":
        Xs[:] = Xs[5]
    p = params(acq, y, 100.0)
    w, full = both_forms(bohip, N, acq, p, Xs)
    assert w == R - min(64, R), w


# empty: the sweep's model and candidates (tests/test_prune_rows_gpu.py) at tau = max y, and on the small shapes a batch whose round 1
# holds every candidate that can win
@pytest.mark.parametrize("acq", ["EI", "UCB"])
def test_empty_list(bohip, acq):
    for form in (0, 1):
        m, X, y = fresh(bohip, 3000, seed=21)
        Xs = np.random.default_rng(22).random((4096, 8))
        set_form(m, form)
        p = [y.max()] if acq == "EI" else [0.5]
        full = record(m, acq, p, Xs, True)
        got = record(m, acq, p, Xs, False)
        w = prune_stat(m)
        print(f"sweep model, {acq}, form {form}: round 2's list length {w}")
        assert w == 0, (form, w)
        assert got == full, (form, got, full)


def test_order_of_the_list_does_not_show(bohip):
    # round 2's list is written with an LDS atomic: its order varies from call to call, the record must not
    for form in (0, 1):
        Xs, p, dup = with_copies(bohip, 450, 321, "EI", 73)
        m, X, y = fresh(bohip, 450)
        set_form(m, form)
        full = record(m, "EI", p, Xs, True)
        recs, words = [], []
        for _ in range(5):
            recs.append(record(m, "EI", p, Xs, False))
            words.append(prune_stat(m))
        print("form", form, "words", words)
        assert all(r == full for r in recs), (recs, full)
        assert all(w == words[0] and w >= 9 for w in words), words


def test_counters_over_forms_and_batch_sizes(bohip):
    # one handle: the arrival counters must come out of every call at zero, whatever the form, the batch and a call that stops
    # after the bounds in between
    A, pa, _ = with_copies(bohip, 450, 321, "EI", 73)
    B, pb, _ = with_copies(bohip, 450, 300, "EI", 70)
    m, X, y = fresh(bohip, 450)
    full = {321: record(m, "EI", pa, A, True), 300: record(m, "EI", pb, B, True)}
    seq = [(0, A, pa), (1, B, pb), (-1, A, pa), ("bounds", B, pb), (1, A, pa), (0, B, pb), (-1, A, pa), (0, A, pa), ("bounds", A, pa),
           (-1, B, pb), (1, A, pa), (0, A, pa)]
    words = []
    for form, Xs, p in seq:
        if form == "bounds":
            assert np.isfinite(prune_bounds(m, p, Xs)).all()
            continue
        set_form(m, form)
        got = record(m, "EI", p, Xs, False)
        w = prune_stat(m)
        words.append(w)
        assert got == full[len(Xs)], (form, len(Xs), w)
        assert 6 <= w <= len(Xs) // 8, (form, len(Xs), w)   # pruned (>= k - 64), and short enough that the next call prunes too
    print("words:", words)


def test_the_librarys_rule(bohip):
    # form -1.  The first call of a handle has no figure: a long list goes through the steady form.  It is longer than R / 8, so the
    # next 31 value-only calls are the full pass's (the back-off); the call after them is the retry, which takes the long form.
    m, X, y = fresh(bohip, 450)
    long_Xs = candidates(450, 321, X)
    p_long = [y.max() + 100.0]
    short_Xs, p_short, _ = with_copies(bohip, 450, 321, "EI", 73)
    full_long, full_short = record(m, "EI", p_long, long_Xs, True), record(m, "EI", p_short, short_Xs, True)
    assert record(m, "EI", p_long, long_Xs, False) == full_long
    assert prune_stat(m) == 321 - 64
    assert record(m, "EI", p_short, short_Xs, False) == full_short
    assert record(m, "EI", p_long, long_Xs, False) == full_long
    for _ in range(29):
        assert record(m, "EI", p_short, short_Xs, False) == full_short
    assert prune_stat(m) == 0                                  # (cleared by the back-off: none of these calls pruned)
    assert record(m, "EI", p_long, long_Xs, False) == full_long   # the retry
    assert prune_stat(m) == 321 - 64
    # a second handle: long, short, long with lists that stay below R / 8 is not possible at these sizes (R / 8 < 256), so the
    # stale figure is exercised with short lists: steady after a short list, whatever the list then is
    m2, X, y = fresh(bohip, 450)
    assert record(m2, "EI", p_short, short_Xs, False) == full_short
    w = prune_stat(m2)
    assert 9 <= w <= 321 // 8, w
    assert record(m2, "EI", p_long, long_Xs, False) == full_long
    assert prune_stat(m2) == 321 - 64


@pytest.mark.parametrize("N,R", [(N, R) for N in (200, 450) for R in (1, 8, 9, 17, 65, 130)] + [(3000, 65)])
def test_group_loop_bit_exact(bohip, N, R):
    # path 2: ONE column group in the grid, every further group from the kernel's loop (N = 200: T = 2, the solo half and contraction
    # extents shorter than the ring)
    m, X, y = fresh(bohip, N)
    Xs = candidates(N, R, X)
    q0, mu0 = run_partials(m, N, Xs, 0)
    q2, mu2 = run_partials(m, N, Xs, 2)
    assert np.isfinite(q0).all() and np.isfinite(mu0).all()
    assert_bits(q2, q0)
    assert_bits(mu2, mu0)
