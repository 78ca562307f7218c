"""Records of the pruned pass through poisoned buffers: a value-only call may read of K*' and of the packed rows only what its own
launches wrote.

A full-pass call (want_scores=True) gives the record and leaves the right K*' behind, which hides a launch that reads an element no
launch of the value-only call filled: the existing pruning tests would pass on such a read.  Here the tests-only export
bohip_debug_kstar_poison overwrites the handle's K*' buffer and the pruned pass's packed rows with all-ones bytes (NaNs) between the
two calls; the value-only call on the same handle must still give the full pass's record (index and value bytes).
bohip_debug_prune_stat >= 0 shows that the pruned pass ran, and its value is the length of round 2's list: every case asserts the
class of list it is meant to hit.  (Written for a pruned pass that stores K*' only where a later launch reads it; that form
measured slower and is not in the library -- profiles/prune_kstar_store_ab.txt -- but the property holds for any form.)

Lists of a wanted length come from tests/test_prune_round2_gpu.py's recipe (k copies of the winner: >= k - 64 entries).  The empty
list on the small shapes is built, not hoped for: every candidate past the first 60 lies at distance >= 49 from the unit cube, where
K*' is exactly 0, the bound is the prior's score exactly, and that is far below the best exact score of round 1."""
import ctypes as C

import numpy as np
import pytest

from test_prune_round2_gpu import ROWS_CAP, candidates, fresh, params, prune_stat, record, set_form, with_copies

pytestmark = pytest.mark.gpu

FORMS = [0, 1]   # round 2's steady and long form (bohip_debug_prune_round2_form)


@pytest.fixture(scope="module")
def bohip():
    import bohip as b
    from bohip import _lib

    assert _lib.load().bohip_device_count() > 0, "GPU tests need an MI355X; libbohip has no CPU fallback"
    return b


def poison(m):
    from bohip import _lib

    f = _lib.load().bohip_debug_kstar_poison
    f.restype = C.c_int
    f.argtypes = [C.c_void_p]
    assert f(m._h) == 0


def through_the_poison(m, acq, p, Xs):
    """Full pass, poison, value-only call on the same handle: the records agree; returns the pinned word."""
    full = record(m, acq, p, Xs, True)
    poison(m)
    got = record(m, acq, p, Xs, False)
    w = prune_stat(m)
    assert w >= 0, w
    assert got == full, (w, got, full)
    return w


def far_tail(Xs, keep=60):
    """Every candidate past the first `keep` moved >= 49 away from the unit cube: K*' is exactly 0 there."""
    Xs = Xs.copy()
    Xs[keep:] += 50.0
    return Xs


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("acq", ["EI", "UCB"])
@pytest.mark.parametrize("k", [1, 65, 73, 129])
@pytest.mark.parametrize("N,R", [(450, 300), (450, 321)])
def test_lists_of_every_class(bohip, N, R, k, acq, form):
    m, X, y = fresh(bohip, N)
    if k == 1:
        Xs, p = far_tail(candidates(N, R, X)), params(acq, y)
    else:
        Xs, p, _ = with_copies(bohip, N, R, acq, k)
    set_form(m, form)
    w = through_the_poison(m, acq, p, Xs)
    print(f"N={N} R={R} {acq} k={k} form={form}: round 2's list length {w}")
    if k == 1:
        assert w == 0, w         # the empty list: round 2 leaves at once
    else:
        assert w >= k - 64, (w, k)   # k = 65: >= 1 entry; 73: past a column group; 129: past one pass of the steady form's grid


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("acq", ["EI", "UCB"])
def test_list_above_the_rows_cap(bohip, acq, form):
    k = 64 + ROWS_CAP + 9
    Xs, p, _ = with_copies(bohip, 3000, 1400, acq, k)
    m, X, y = fresh(bohip, 3000)
    set_form(m, form)
    w = through_the_poison(m, acq, p, Xs)
    assert w > ROWS_CAP and w >= k - 64, (w, k)


@pytest.mark.parametrize("N,R", [(450, 300), (450, 321)])
def test_everything_outside_round_1_listed(bohip, N, R):
    # tau = max y + 100 under the steady form: every row outside round 1 is read by round 2
    m, X, y = fresh(bohip, N)
    set_form(m, 0)
    w = through_the_poison(m, "EI", params("EI", y, 100.0), candidates(N, R, X))
    assert w == R - 64, w


def test_the_librarys_rule_on_a_first_call(bohip):
    # form -1 on a fresh handle: no figure yet, so the steady form whatever the list will be
    for k, dt in ((73, 0.0), (None, 100.0)):
        m, X, y = fresh(bohip, 450)
        if k:
            Xs, p, _ = with_copies(bohip, 450, 321, "EI", k)
        else:
            Xs, p = candidates(450, 321, X), params("EI", y, dt)
        set_form(m, -1)
        w = through_the_poison(m, "EI", p, Xs)
        assert (w >= k - 64) if k else (w == 321 - 64), (k, w)


@pytest.mark.parametrize("which", ["Mat32Ard", "d16"])
@pytest.mark.parametrize("acq", ["EI", "UCB"])
def test_other_models(bohip, which, acq):
    d = 16 if which == "d16" else 8
    ll = np.log(np.sqrt(d) * np.linspace(0.35, 0.7, d))
    N, R, k = 450, 321, 73
    for form in FORMS:
        rng = np.random.default_rng(77 + N + d)
        X = rng.random((N, d))
        y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(N)
        m = bohip.ElasticGPE(d, mean=bohip.MeanConst(0.0), kernel=(bohip.SEArd if which == "d16" else bohip.Mat32Ard)(ll, 0.0),
                             logNoise=-2.0, capacity=N)
        m.append_(X.T, y)
        Xs = np.random.default_rng(3).random((R, d))
        p = params(acq, y)
        i_best, _ = record(m, acq, p, Xs, True)
        dup = sorted(set(range(k - 1)) | {i_best})
        Xs[dup] = Xs[i_best]
        set_form(m, form)
        w = through_the_poison(m, acq, p, Xs)
        assert w >= len(dup) - 64 >= 8, (form, w)


def test_one_handle_three_candidate_sets(bohip):
    # one poison, then six value-only calls with no full pass in between: each call finds the call before's K*' and packed rows
    N = 450
    m, X, y = fresh(bohip, N)
    sets = [with_copies(bohip, N, 321, "EI", 73)[:2], with_copies(bohip, N, 300, "EI", 70)[:2],
            (far_tail(candidates(N, 321, X)), params("EI", y))]
    set_form(m, 0)
    full = [record(m, "EI", p, Xs, True) for Xs, p in sets]
    poison(m)
    words = []
    for rnd in range(2):
        for (Xs, p), want in zip(sets, full):
            got = record(m, "EI", p, Xs, False)
            words.append(prune_stat(m))
            assert got == want, (rnd, words)
    print("words:", words)
    assert words[0] >= 9 and words[1] >= 6 and words[2] == 0 and words[3:] == words[:3], words
