"""The CPU-side conditions of the life-cycle tests (tests/test_lifecycle_gpu.py): the history takes the routes it was written for,
the bound of Part A is attainable by a plain float64 inversion with room to spare, and Part C's checks are not vacuous (a twin that
lacks the jitter differs from the one that has it by more than 100 x the tolerance the device is held to)."""
import math

import numpy as np
import pytest

import lifecycle_inputs as li
import path_reference as pr
from matern_reference import MaternGP
from oracle.oracle import fit_with_jitter


def test_the_history_takes_the_routes_of_its_table():
    p = li.plan()
    appends = [s for s in p if s["action"] == "append"]
    assert [s["n"] for s in appends] == [90, 95, 127, 128, 130, 133, 165, 197, 198, 203, 206]
    assert [s["route"] for s in appends] == ["refit", "incremental", "refit"] + ["incremental"] * 6 + ["refit", "incremental"]
    assert [s["ld"] for s in appends] == [144, 144] + [272] * 7 + [528, 528]
    assert [s["cap"] for s in appends] == [100, 100] + [200] * 7 + [400, 400]
    calls = {s["arg"]: s for s in p if s["action"] == "call"}
    assert {k: (v["n"], v["ld"]) for k, v in calls.items()} == {"warm": (90, 144), "A": (127, 272), "B": (165, 272), "C": (165, 272),
                                                                "D": (206, 528)}
    assert (calls["B"]["refits"], calls["C"]["refits"], calls["D"]["refits"]) == (2, 3, 4)      # C: the stale handle is factored again
    assert (calls["A"]["appends"], calls["B"]["appends"], calls["D"]["appends"]) == (1, 5, 8)
    # N0 = 127 -> 128: Npad = round_up(N + 1, 128) goes from 128 to 256, the alpha row (row N of W) into the second tile
    assert -(-(127 + 1) // li.TILE) * li.TILE == 128 and -(-(128 + 1) // li.TILE) * li.TILE == 256
    # a feature that never reads the resident model leaves the handle stale: the next append is then a refit, so the device test
    # freshens such a handle itself after the call at C (one refit, as if the feature had)
    lazy = {s["arg"]: s for s in li.plan(reads_model=False) if s["action"] == "call"}
    assert lazy["C"]["refits"] == 2 and lazy["C"]["freshen"] and lazy["D"]["refits"] == 4 and lazy["D"]["appends"] == 8
    assert li.N_AT == {k: v["n"] for k, v in calls.items()}
    for ck, lo in li.APPENDED_FROM.items():                                 # the rows appends wrote since the last refit
        last_refit = max(s["n"] for s in p if s["route"] == "refit" and s["n"] <= li.N_AT[ck])
        assert lo == (li.N_AT[ck] if ck == "C" else last_refit), ck


@pytest.mark.parametrize("kern,d", li.PAIRS)
def test_the_inverse_bound_is_attainable(kern, d):
    """float64 substitution (LAPACK dtrtri's arithmetic through solve_triangular) stays within a tenth of the componentwise bound
    of Part A on every model of the history, so a device inverse that misses the bound is wrong, not unlucky."""
    for name in li.CHECKPOINTS:
        ck = li.checkpoint(kern, d, name)
        L = ck.ref.L
        Wref = li.inv_lower_ld(L)
        resid = np.abs(np.asarray(L, dtype=np.longdouble) @ Wref - np.eye(ck.n)).max()
        assert resid < 1e-17 * ck.n, resid                                  # the reference is an inverse to extended precision
        comp, norm = li.inverse_bounds(L, Wref)
        W64 = li.solve_inverse(L)
        share = li.inverse_share(W64, Wref, comp)
        kappa = norm / (ck.n * li.EPS * float(np.abs(Wref).max()))
        print(f"{ck}: float64 substitution uses {share:.3f} of the componentwise bound; kappa_inf(L) = {kappa:.3g}")
        assert share <= 0.1
        assert li.inverse_share(W64, Wref, norm) <= share                   # the normwise form is the weaker one
        # the bound can tell a wrong entry: a relative error of 1e-9 in the last diagonal entry is far outside
        bad = W64.copy()
        bad[ck.n - 1, ck.n - 1] *= 1.0 + 1e-9
        assert li.inverse_share(bad, Wref, comp) > 100.0


def jittered():
    X, y, Xa, ya = li.jitter_data()
    mean_diag = math.exp(2.0 * li.JIT_LSIG) + math.exp(2.0 * li.JIT_LNOISE)
    return X, y, Xa, ya, li.JIT_REL * mean_diag


def test_the_jittered_model_takes_one_try_and_is_well_conditioned(orc):
    X, y, _, _, J = jittered()
    with pytest.raises(np.linalg.LinAlgError):
        orc.fit(X, y, li.JIT_LL, li.JIT_LSIG, li.JIT_LNOISE, li.JIT_BETA)
    L, alpha, tries, added = fit_with_jitter(orc, X, y, li.JIT_LL, li.JIT_LSIG, li.JIT_LNOISE, li.JIT_BETA, li.JIT_REL, li.JIT_TRIES)
    assert tries == 1 and added == J
    ref = MaternGP("SEArd", X, y, li.JIT_LL, li.JIT_LSIG, li.lognoise_with(li.JIT_LNOISE, J), li.JIT_BETA)
    np.testing.assert_allclose(ref.L, L, rtol=1e-9, atol=1e-12 * math.exp(li.JIT_LSIG))   # the twin with logNoise' IS the jittered model
    kappa = np.linalg.cond(ref.cK)
    print(f"J = {J:.6g}, kappa_2(cK + J I) = {kappa:.3g}")
    assert 1e3 < kappa < 1e6                                                # (measured 2.3e4: the families' bounds stay meaningful)


def test_the_twins_without_the_jitter_are_far_away():
    """Non-vacuity of Part C on the CPU: a twin whose fantasy noise (select_batch) or whose sqrt(noise) (the paths' right-hand side)
    lacks J differs from the twin that has it by more than 100 x the tolerance the device is held to."""
    X, y, _, _, J = jittered()
    Xs = li.jitter_candidates(li.JIT_R)
    s2f = math.exp(2.0 * li.JIT_LSIG)
    for acq, p, fantasy in li.JIT_BATCH:
        with_j = li.jitter_batch_twin(X, y, Xs, acq, p, fantasy, J)
        without = li.jitter_batch_twin(X, y, Xs, acq, p, fantasy, J, fantasy_noise_has_j=False)
        assert all(r[4] > 1e-7 for r in with_j), "choose another JIT_SEED: a near tie among the twin's picks"
        moved = li.batch_moved(with_j, without, len(y), s2f)
        print(f"select_batch {acq} {fantasy}: the twin without J in the fantasy's noise differs by {moved:.3g} x the tolerance")
        assert moved > 100.0
    tw = li.jitter_path_twin(X, y, J)
    nu0 = math.exp(2.0 * li.JIT_LNOISE) + li.EPS
    for s in (0, 2):
        w, ze = tw.w(s), pr.noise_normals(tw.seed, s, tw.M, tw.N)
        rhs, u = tw.rhs(s), tw.u(s)
        without = (y - tw.beta) - tw.PhiX @ w - math.sqrt(nu0) * ze
        moved = float(np.max(np.abs(rhs - without) / li.path_solve_bound(tw, u, w, rhs, ze)))
        print(f"paths, path {s}: the right-hand side without J differs by {moved:.3g} x the bound of K u = rhs")
        assert moved > 100.0
