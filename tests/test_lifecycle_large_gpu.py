"""Lived-in models past 256 rows: the pruned arg-max, split-K and the whole-K passes with W' on a handle that has a history.

tests/test_lifecycle_gpu.py stops at 206 observations, two row tiles: no call there can prune (prune_tiles needs three) or split the
contraction (split_applicable needs eight), and every pruning test of the suite builds a fresh handle and compares the value-only
record with the full pass of the SAME handle.  Here one scripted history per handle (tests/lifecycle_large_inputs.py) runs ONCE in a
module-scoped driver that records what the device returned at the checkpoints A (N = 256, the first pruned call), B0 (383), B (384,
incremental factor), C (stale hyper-parameters), D (896, split-K) and E (1041, after the third re-allocation); the tests assert on the
record, against the checkpoint's independent twin.  Three handles live the history: SEArd d = 3, Mat32Iso d = 9, and a SEArd d = 3
handle of weighted sites (bohip_gp_append_sites) whose twin is rep_reference.RepTwin in float64.

The driver asserts INFO_REFITS, INFO_APPENDS, INFO_CAPACITY and the stage labels after every step against plan(), and at every
checkpoint the value-only call comes first: at C it is that call which must raise INFO_REFITS by one (test_lifecycle_gpu.Own).

Every numeric bound is an existing one of the suite, named where it is used.  Every test prints its worst share of its bound
(profiles/lifecycle_large_tests.txt holds the output of a run on an MI355X)."""
import math

import numpy as np
import pytest

import lifecycle_inputs as li
import lifecycle_large_inputs as ll
import rep_reference as rr
from conftest import var_tol
from high_dim_inputs import score_floor
from matern_reference import first_argmax
from test_high_dim_gpu import SMALL, SPLIT, WHOLE, assert_route, labels
from test_lifecycle_gpu import Own, Shares, new_handle, read_w, sub_of
from test_parity_gpu import bohip  # noqa: F401  (fixture)
from test_prune_poison_gpu import poison, through_the_poison
from test_prune_round2_gpu import prune_stat, set_form
from test_prune_select_gpu import bounds as prune_bounds
from test_prune_select_gpu import expected_round2

pytestmark = pytest.mark.gpu

GRAD_ACQS = ("UCB", "EI")
WHOLE_HINT = 1 << 20                                                        # test_split_k_path_vs_oracle_and_whole_k's: the whole-K schedule


def xs_of(ck, R):
    return np.asfortranarray(ck.Xs[:R].T)


def value_only(m, acq, p, xs):
    _, v, i = m.score(acq, p, xs, want_scores=False)
    return int(i), np.float64(v).tobytes()


def pruned(m, acq, p, xs, next_R, what, log):
    """A value-only call that must take the pruned pass: (record, round 2's list length).  next_R: the smallest batch the handle's
    next value-only call may have; a list longer than an eighth of it would send that call to the full pass (prune_wanted's
    back-off), where bohip_debug_prune_stat reads 0 and proves nothing: logged here, asserted by test_pruned_records_are_the_scored_calls."""
    rec = value_only(m, acq, p, xs)
    w = prune_stat(m)
    assert_route(m, ["kstar", "trigemm_sq"], SMALL + SPLIT)
    assert w >= 0, (what, w)
    log.append((what, w, next_R))
    return rec, w


# ==== the driver ======================================================================================================================
def append_step(m, ck_data, step, weighted):
    """One append of the history; the labels say which route it took (and, on a weighted handle, that rep_diag followed the covariance)."""
    n, arg = step["n"], step["arg"]
    lo = n - arg
    if weighted:
        pos, evals, _ = ck_data
        x, ybar, reps, ss, ymax = rr.sites_of(pos, evals, lo, n)
        if lo < ll.N_PLAIN:
            assert n == ll.N_PLAIN and np.all(reps == 1)
            m.append_(x, ybar)
        else:
            m.append_sites_(x, ybar, reps, ss, ymax)
    else:
        X, y, _ = ck_data
        m.append_(X[lo:n].T, y[lo:n])
    lab = labels(m)
    if step["route"] == "incremental":
        assert "append_cov_rows" in lab and "append_W21" in lab and "build_cov" not in lab, (step, lab)
    else:
        assert "build_cov" in lab and "append_W21" not in lab, (step, lab)
    is_weighted = weighted and n > ll.N_PLAIN
    assert ("rep_diag" in lab) == is_weighted and m.weighted == is_weighted, (step, lab)
    if is_weighted:
        assert lab[lab.index("rep_diag") - 1] == ("append_cov_rows" if step["route"] == "incremental" else "build_cov"), (step, lab)
    if step["route"] == "refit" and ll.row_tiles(n) >= 4:                   # a dataflow Cholesky with a factorisation task
        assert "cholesky+inverse" in lab or "cholesky" in lab, (step, lab)


def at_checkpoint(m, ck, own, out):
    """Every device call of one checkpoint, the entry point under test first; the results go to `out`, the route assertions are made here."""
    n, name = ck.n, ck.name
    Rb, Rs = ll.R_PRUNE.get(name, (ll.R_MID, ll.R_MID))
    xb, xs_small, x40, x700 = xs_of(ck, Rb), xs_of(ck, Rs), xs_of(ck, ll.R_SMALL), xs_of(ck, ll.R_MID)
    p_ei = ck.params("EI")
    if name == "warm":                                                      # T = 2: nothing prunes; the scratch of every route comes to exist at ld = 400
        assert ll.route_of(n, Rb, value_only=True) == "whole" and prune_stat(m) == -1
        out["first"] = own(value_only, m, "EI", p_ei, xb)
        assert prune_stat(m) == -1
        sc, bv, bi = m.score("EI", p_ei, xb)
        assert out["first"] == (int(bi), np.float64(bv).tobytes())
        m.score_grad("UCB", ck.params("UCB"), xb)
        assert_route(m, ["trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT)
        m.score("EI", p_ei, x40)
        assert_route(m, ["small_V"], WHOLE + SPLIT)
        return
    assert ll.route_of(n, Rb, value_only=True) == ll.route_of(n, Rs, value_only=True) == "pruned"
    log = out["lists"] = []
    set_form(m, -1)
    out["first"] = own(pruned, m, "EI", p_ei, xb, Rs, (ck, "first"), log)           # C: the reader that factors the stale handle
    out["mu"], out["var"] = m.predict_f(xb)
    for acq in ll.ACQS:
        p = ck.params(acq)
        o = out[acq] = {}
        sc, bv, bi = m.score(acq, p, xb)
        assert_route(m, ["kstar", "trigemm_sq"], SMALL + SPLIT)
        o["scores"], o["full"] = sc, (int(bi), np.float64(bv).tobytes())
        for form in (0, 1) + ((-1,) if acq == "EI" else ()):                # both round-2 forms, and once the library's own rule
            poison(m)
            set_form(m, form)
            o["form", form] = pruned(m, acq, p, xb, Rs, (ck, acq, form), log)
        set_form(m, -1)
        o["ub"] = prune_bounds(m, acq, p, ck.Xs[:Rb])
        scs, bvs, bis = m.score(acq, p, xs_small)
        o["scores_small"], o["full_small"] = scs, (int(bis), np.float64(bvs).tobytes())
        poison(m)
        o["small"] = pruned(m, acq, p, xs_small, Rs, (ck, acq, "smaller batch"), log)     # dpr does not grow: only its offsets move
        o["again"] = pruned(m, acq, p, xb, Rs, (ck, acq, "larger batch again"), log)
        Xd, _ = ll.dup_set(ck, acq, Rb)                                     # a round-2 list that is not empty: the forms differ only then
        xd = np.asfortranarray(Xd.T)
        scd, bvd, bid = m.score(acq, p, xd)
        o["dup_full"] = (int(bid), np.float64(bvd).tobytes())
        for form in (0, 1):
            poison(m)
            set_form(m, form)
            # (the value-only call after this one has the larger batch, here or at the next checkpoint: up to DUP_K - 1 entries may be listed)
            o["dup", form] = pruned(m, acq, p, xd, ll.R_MID, (ck, acq, "copies of the winner", form), log)
        set_form(m, -1)
    # ---- routes by label ----
    mid = ll.route_of(n, ll.R_MID)
    assert ll.route_of(n, ll.R_SMALL) == "small" and mid == ("split" if name in ("D", "E") else "whole")
    p_ucb = ck.params("UCB")
    out["small40"] = m.score("UCB", p_ucb, x40)
    assert_route(m, ["small_V"], WHOLE + SPLIT + ("kstar",))
    out["mid"] = m.score("UCB", p_ucb, x700)
    if mid == "split":
        assert_route(m, ["kstar", "split_V", "score"], SMALL + WHOLE)
        m.set_batch_hint(WHOLE_HINT)
        out["mid_whole"] = m.score("UCB", p_ucb, x700)
        assert_route(m, ["kstar", "trigemm_sq"], SMALL + SPLIT)
        m.set_batch_hint(0)
    else:
        assert_route(m, ["kstar", "trigemm_sq"], SMALL + SPLIT + ("score",))
    # ---- score_grad reads W' ----
    if name in ("B", "D", "E"):
        for acq in GRAD_ACQS:
            p = ck.params(acq)
            sc, g = m.score_grad(acq, p, x700)
            if mid == "split":
                assert_route(m, ["kstar", "split_V", "split_U", "score+grad"], SMALL + WHOLE)
            else:
                assert_route(m, ["trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT)
            out["grad", acq] = (sc, g, m.score(acq, p, x700)[0])
            if mid == "split":
                m.set_batch_hint(WHOLE_HINT)
                scw, gw = m.score_grad(acq, p, x700)
                assert_route(m, ["trigemm_sq+V", "gemm_U", "score+grad"], SMALL + SPLIT)
                out["grad_whole", acq] = (scw, gw, m.score(acq, p, x700)[0])
                m.set_batch_hint(0)
    # ---- the resident state ----
    out["L"], out["alpha"] = m.factor(), m.alpha()
    if name in ("B", "E"):
        out["W"], out["WT"] = np.tril(read_w(m, 0)), np.triu(read_w(m, 1))
    if name in ("C", "E"):
        out["mll_grad"], out["mll"] = m.mll_grad(), m.mll()
        if ck.weighted:
            out["sites"] = (m.nobs, m.nevals, m.get_reps().copy())


def run_history(bohip, kern, d, weighted):
    from bohip import _lib

    src = ll.weighted_data() if weighted else ll.data(kern, d)
    m = new_handle(bohip, kern, d, ll.hyper(kern, "A", weighted), ll.CAPACITY)
    base = (m.info(_lib.INFO_REFITS), m.info(_lib.INFO_APPENDS))
    own = Own(m)
    record = {}
    try:
        for step in ll.plan():
            action, arg = step["action"], step["arg"]
            if action == "append":
                append_step(m, src, step, weighted)
            elif action == "hyper":
                ll_, lsig, lnoise, beta = ll.hyper(kern, "C", weighted)
                m.set_params_(ll=ll_, lsigma=lsig, logNoise=lnoise, beta=beta)    # no fit_(): the next reader has to factor again
                own.stale = True
            else:
                ck = ll.checkpoint(kern, d, arg, weighted)
                assert m.nobs == ck.n == step["n"] and ll.CAP_AT[arg] == step["cap"]
                record[arg] = {}
                at_checkpoint(m, ck, own, record[arg])
                if arg == "C":
                    assert own.met_stale == 1 and not own.stale, (ck, own.met_stale)
            got = (m.info(_lib.INFO_REFITS) - base[0], m.info(_lib.INFO_APPENDS) - base[1], m.info(_lib.INFO_CAPACITY))
            assert got == (step["refits"], step["appends"], step["cap"]), (step, got)
    finally:
        m.close()
    return record


@pytest.fixture(scope="module", params=ll.HANDLES, ids=lambda h: f"{h[0]}-d{h[1]}{'-weighted' if h[2] else ''}")
def lived(request, bohip):  # noqa: F811
    kern, d, weighted = request.param
    return kern, d, weighted, run_history(bohip, kern, d, weighted)


def checkpoints(lived):
    kern, d, weighted, record = lived
    for name in ll.CHECKPOINTS:
        yield ll.checkpoint(kern, d, name, weighted), record[name]


# ==== the pruned route ==================================================================================================================
def test_pruned_records_are_the_scored_calls(lived):
    """A to E: for EI, UCB and PI the value-only record (index and value bytes) is the scored call's on the same handle, through
    bohip_debug_kstar_poison, in both round-2 forms and under the library's rule, for the larger batch, the smaller one and the larger
    again; every such call pruned (bohip_debug_prune_stat >= 0 and the pass's labels, asserted by the driver; no list long enough to
    send the next call into the back-off, asserted here)
    and round 2's list length is test_prune_select_gpu.expected_round2's on the device's own bounds and scores.  Those lists are
    empty on these inputs, so both forms run once more on candidates that hold DUP_K copies of the twin's winner
    (test_prune_round2_gpu's recipe): at least DUP_K - 64 entries, and the lowest index of the tie wins."""
    n_calls, lists = 0, []
    for ck, o in checkpoints(lived):
        for what, w, next_R in o["lists"]:                                  # no call sent the next one into the back-off
            assert w <= next_R // 8, (what, w, next_R)
        assert o["first"][0] == o["EI"]["full"], (ck, "the first reader")
        for acq in ll.ACQS:
            a = o[acq]
            sc = a["scores"]
            assert a["full"] == (first_argmax(sc)[1], np.float64(first_argmax(sc)[0]).tobytes())
            _, n2 = expected_round2(a["ub"], sc)
            for key in [("form", 0), ("form", 1), "again"] + ([("form", -1)] if acq == "EI" else []):
                rec, w = a[key]
                assert rec == a["full"], (ck, acq, key, rec, a["full"])
                assert w == n2, (ck, acq, key, w, n2)
                n_calls += 1
            rec, w = a["small"]
            assert rec == a["full_small"], (ck, acq, "smaller batch", rec, a["full_small"])
            _, dup = ll.dup_set(ck, acq, ll.R_PRUNE[ck.name][0])
            for form in (0, 1):                                             # DUP_K copies of the winner: round 2 has a list to work on
                rec, w = a["dup", form]
                assert rec == a["dup_full"] and rec[0] == dup[0], (ck, acq, form, rec, a["dup_full"], dup[0])
                assert w >= ll.DUP_K - ll.SELECT_K1 and w == a["dup", 0][1], (ck, acq, form, w)
                lists.append(w)
                n_calls += 1
            np.testing.assert_array_equal(a["scores_small"], sc[:len(a["scores_small"])])      # a score does not depend on its batch
            n_calls += 1
    print(f"  {lived[0]} d={lived[1]}{' weighted' if lived[2] else ''}: {n_calls} pruned calls gave the scored call's record; "
          f"round-2 lists of the calls with {ll.DUP_K} copies of the winner: {min(lists)} to {max(lists)} entries")


def test_scores_and_winners_against_the_twin(lived):
    """mu, sigma^2 and the scores of the scored call against the checkpoint's twin at test_seeded_vs_oracle's bounds (1e-6 relative
    plus mu_floor / var_tol / the score floor; rep_reference.mu_bound, var_tol and score_bound on the weighted handle are the same
    expressions); the index is the twin's first arg-max unless the twin's top two are closer than 4 max(floor) (the rule of
    test_seeded_vs_oracle; tests/test_lifecycle_large_host.py caps the exemptions at a tenth of the cases -- none is taken)."""
    kern, d, weighted, _ = lived
    exempt = 0
    for ck, o in checkpoints(lived):
        Rb, Rs = ll.R_PRUNE[ck.name]
        sh = Shares(f"{ck} R={Rb}")
        mu_r, var_r = ll.moments(kern, d, ck.name, weighted, Rb)
        sh.note("mu", np.abs(o["mu"] - mu_r), 1e-6 * np.abs(mu_r) + ck.floor)
        sh.note("var", np.abs(o["var"] - var_r), var_tol(var_r, ck.n, ck.s2f))
        for acq in ll.ACQS:
            sc_r, fl = ll.twin_scores(ck, acq, Rb)
            sh.note(acq, np.abs(o[acq]["scores"] - sc_r), 1e-6 * np.abs(sc_r) + fl)
            for R, rec in ((Rb, o[acq]["full"]), (Rs, o[acq]["full_small"])):
                if ll.exempt((kern, d, weighted, ck.name, acq, R)):
                    exempt += 1
                else:
                    assert rec[0] == first_argmax(ll.twin_scores(ck, acq, R)[0])[1], (ck, acq, R)
        for key, R in (("small40", ll.R_SMALL), ("mid", ll.R_MID), ("mid_whole", ll.R_MID)):      # the small route, whole-K / split-K
            if key in o:
                mu_k, var_k = ll.moments(kern, d, ck.name, weighted, R)
                p = ck.params("UCB")
                sc_k = ck.ref.score("UCB", p, ck.Xs[:R])
                sc, bv, bi = o[key]
                sh.note(f"UCB R={R} {key}", np.abs(sc - sc_k), 1e-6 * np.abs(sc_k) + score_floor("UCB", p, ck.floor, var_k, ck.n, ck.s2f))
                assert (bv, bi) == first_argmax(sc)
        if "mid_whole" in o:                                                # test_split_k_path_vs_oracle_and_whole_k: rtol 1e-10, atol 1e-13
            sh.note("split-K vs whole-K", np.abs(o["mid"][0] - o["mid_whole"][0]), 1e-10 * np.abs(o["mid_whole"][0]) + 1e-13)
        sh.done()
    print(f"  arg-max exemptions taken: {exempt}")


def test_prune_bounds_cover_the_twins_scores(lived):
    """bohip_debug_prune_bounds on the lived-in handle: no bound below the device's own score of the scored call (what exactness rests
    on: test_bound_holds_for_every_candidate), and none below the TWIN's exact score minus the score's floor."""
    for ck, o in checkpoints(lived):
        Rb = ll.R_PRUNE[ck.name][0]
        worst = {}
        for acq in ll.ACQS:
            ub, sc = o[acq]["ub"], o[acq]["scores"]
            assert np.isfinite(ub).all() and not (ub < sc).any(), (ck, acq, np.flatnonzero(ub < sc)[:5])
            sc_r, fl = ll.twin_scores(ck, acq, Rb)
            tol = 1e-6 * np.abs(sc_r) + fl
            worst[acq] = float(np.max((sc_r - ub) / tol))
            assert np.all(ub >= sc_r - tol), (ck, acq, worst[acq])
        print(f"  {ck} R={Rb}: worst (twin's score - bound) / floor (<= 1 holds; negative: the bound lies above): "
              + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ==== score_grad ========================================================================================================================
def test_score_grad_on_whole_k_and_split_k(lived):
    """B (whole-K: gemm_U on rows of W' that appends wrote), D and E (split-K: split_U, and whole-K forced through the batch hint):
    values and gradients against the twin's analytic gradient at test_score_grad_vs_oracle's bounds (rtol 1e-6; atol mu_floor + 1e-12
    and 1e-9 max|g| + 1e-12), the value path and the gradient path bit for bit, split-K against whole-K at
    test_split_k_path_vs_oracle_and_whole_k's (rtol 1e-7, atol 1e-10 max|g|)."""
    sub = sub_of(ll.R_MID, 48)
    for ck, o in checkpoints(lived):
        if ck.name not in ("B", "D", "E"):
            continue
        sh = Shares(f"{ck} score_grad R={ll.R_MID}")
        for acq in GRAD_ACQS:
            sc_r, g_r = ck.ref.score_grad(acq, ck.params(acq), ck.Xs[:ll.R_MID][sub])
            assert np.abs(g_r).max() > 0
            for key in ("grad", "grad_whole"):
                if (key, acq) not in o:
                    continue
                sc, g, sv = o[key, acq]
                route = "whole-K" if key == "grad_whole" or ck.name == "B" else "split-K"
                sh.note(f"{acq} value, {route}", np.abs(sc[sub] - sc_r), 1e-6 * np.abs(sc_r) + ck.floor + 1e-12)
                sh.note(f"{acq} grad, {route}", np.abs(g.T[sub] - g_r), 1e-6 * np.abs(g_r) + 1e-9 * np.abs(g_r).max() + 1e-12)
                np.testing.assert_array_equal(sc, sv)                       # value path == gradient path, bit for bit
            if ("grad_whole", acq) in o:
                (sc, g, _), (scw, gw, _) = o["grad", acq], o["grad_whole", acq]
                sh.note(f"{acq} value, split-K vs whole-K", np.abs(sc - scw), 1e-10 * np.abs(scw) + 1e-13)
                sh.note(f"{acq} grad, split-K vs whole-K", np.abs(g - gw), 1e-7 * np.abs(gw) + 1e-10 * np.abs(gw).max())
        sh.done()


# ==== the resident state ================================================================================================================
def test_factor_and_alpha_against_the_twin(lived, orc):
    """L and alpha at every checkpoint against the twin at test_seeded_vs_oracle's bounds (rtol 1e-9 / atol 1e-11 s_f, rtol 1e-6 /
    atol 1e-9 max|alpha|: test_rep_gpu.check_state's too); the plain SEArd handle against the C oracle as well."""
    kern, d, weighted, _ = lived
    for ck, o in checkpoints(lived):
        refs = [(ck.ref.L, ck.ref.alpha)]
        if kern == "SEArd" and not weighted:
            refs.append(orc.fit(ck.X, ck.y, ck.ll, ck.lsig, ck.lnoise, ck.beta))
        sL = sa = 0.0
        for Lr, ar in refs:
            sL = max(sL, float(np.max(np.abs(o["L"] - Lr) / (1e-9 * np.abs(Lr) + 1e-11 * math.sqrt(ck.s2f)))))
            sa = max(sa, float(np.max(np.abs(o["alpha"] - ar) / (1e-6 * np.abs(ar) + 1e-9 * np.abs(ar).max()))))
        print(f"  {ck}: worst share of the bounds: L {sL:.2e}, alpha {sa:.2e}")
        assert sL <= 1 and sa <= 1 and not np.any(np.triu(o["L"], 1)), (ck, sL, sa)


def test_resident_inverse_and_its_transpose(lived):
    """B (rows 261 ... 383 written by appends at ld = 656) and E (everything by the refit at ld = 2192): tril(W) and triu(W') against
    the np.longdouble inverse of the device's own L within lifecycle_inputs.inverse_bounds (N eps |W| |L| |W| entry by entry, and
    its normwise form), and W'[c, i] == W[i, c] bit for bit."""
    for ck, o in checkpoints(lived):
        if ck.name not in ("B", "E"):
            continue
        n, lo = ck.n, ll.APPENDED_FROM[ck.name]
        L, W, WT = o["L"], o["W"], o["WT"]
        Wref = li.inv_lower_ld(L)
        comp, norm = li.inverse_bounds(L, Wref)
        refit_rows, app_rows = slice(0, lo), slice(lo, n)
        s = {"W refit rows": li.inverse_share(W, Wref, comp, refit_rows), "W append rows": li.inverse_share(W, Wref, comp, app_rows),
             "W' refit rows": li.inverse_share(WT.T, Wref, comp, refit_rows), "W' append rows": li.inverse_share(WT.T, Wref, comp, app_rows),
             "W normwise": li.inverse_share(W, Wref, norm)}
        same_app, same_all = np.array_equal(WT.T[app_rows], W[app_rows]), np.array_equal(WT.T, W)
        print(f"  {ck}: rows [{lo}, {n}) written by appends; share of N eps |W||L||W|: " + ", ".join(f"{k} {v:.2e}" for k, v in s.items())
              + f"; W' == W.T bit for bit: append rows {same_app}, all rows {same_all}")
        assert same_app, (ck, "W' lags W on the rows appends wrote")
        assert same_all, (ck, "W' differs from W.T on rows a refit wrote")
        assert all(v <= 1.0 for v in s.values()), (ck, s)


# ==== the marginal likelihood, and jitter on a weighted handle =============================================================================
def test_likelihood_behind_a_large_inverse(lived):
    """mll and mll_grad at C and E (cK^-1 = W'W behind a T >= 4 inverse; on the weighted handle k_rep_noise_sum and the site constant,
    for the first time at this size) against the twin -- RepTwin on the weighted handle -- at test_rep_gpu.check_state's bounds: 1e-9
    relative (rep_reference.MLL_RTOL, every mll check of the suite) and rep_reference.grad_bound (test_mll_gradient_vs_oracle's)."""
    kern, d, weighted, _ = lived
    for ck, o in checkpoints(lived):
        if ck.name not in ("C", "E"):
            continue
        if weighted:
            ns, ne, reps = o["sites"]
            assert (ns, ne) == (ck.n, int(ck.reps.sum())) and np.array_equal(reps, ck.reps)
        mll_r, dn, dm, dk = ck.tw.mll_grad() if weighted else ck.ref.mll_grad()
        g_r = np.concatenate([[dn, dm], np.ravel(dk)]).astype(np.float64)
        mll, gn, gm, gk = o["mll_grad"]
        g = np.concatenate([[gn, gm], gk])
        s_m, s_g = abs(mll - float(mll_r)) / (rr.MLL_RTOL * abs(float(mll_r))), float(np.max(np.abs(g - g_r) / rr.grad_bound(g_r)))
        print(f"  {ck}: worst share of the bounds: mll {s_m:.2e}, mll_grad {s_g:.2e}")
        assert s_m <= 1 and s_g <= 1 and mll == o["mll"], (ck, mll, float(mll_r), g, g_r)


def test_jitter_on_a_weighted_handle(bohip, orc):  # noqa: F811
    """test_hardening_gpu's singular model as 300 sites of 1 to 5 evaluations under set_jitter(1e-3, 3): refit_once puts (nu + J) / r_i
    on the diagonal and site_constant reads nu + jitter_last.  L, alpha, predict_f, mll and mll_grad against RepTwin(jitter=J), J what
    oracle.fit_with_jitter reports; then an incremental append of three sites, whose diagonal carries J / r_i too.  Bounds:
    test_jitter_escalation_switch_against_its_oracle_twin's (L L' to 1e-9 max|cK|; mu rtol 1e-5 / atol 1e-5 max|mu|; sigma^2 rtol 1e-5 /
    atol 1e-6 s_f^2), test_rep_gpu.check_state's for alpha, mll (1e-9) and its gradient (rep_reference.grad_bound)."""
    from bohip import _lib
    from oracle.oracle import fit_with_jitter

    X, ybar, reps, ss, Xa, ya, ra, sa = ll.jitter_sites()
    _, _, tries, J = fit_with_jitter(orc, X, ybar, li.JIT_LL, li.JIT_LSIG, li.JIT_LNOISE, li.JIT_BETA, li.JIT_REL, li.JIT_TRIES)
    m = bohip.ElasticGPE(2, mean=bohip.MeanConst(li.JIT_BETA), kernel=bohip.SEArd(li.JIT_LL, li.JIT_LSIG), logNoise=li.JIT_LNOISE,
                         capacity=len(ybar) + 8)
    m.enable_timing(True)
    Xs = li.jitter_candidates(64)
    s2f = math.exp(2.0 * li.JIT_LSIG)
    try:
        m.set_jitter(li.JIT_REL, li.JIT_TRIES)
        m.append_sites_(np.asfortranarray(X.T), ybar, reps, ss)
        assert m.weighted and "rep_diag" in labels(m) and m.info(_lib.INFO_JITTER_STEPS) == tries == 1
        for with_append in (False, True):
            if with_append:
                n_app = m.info(_lib.INFO_APPENDS)
                m.append_sites_(np.asfortranarray(Xa.T), ya, ra, sa)
                lab = labels(m)
                assert m.info(_lib.INFO_APPENDS) == n_app + 1 and "rep_diag" in lab and "build_cov" not in lab, lab
            tw = ll.jitter_twin(J, with_append)
            L, alpha = m.factor(), m.alpha()
            mu, var = m.predict_f(np.asfortranarray(Xs.T))
            mll, gn, gm, gk = m.mll_grad()
            mu_r, var_r = tw.predict(Xs)
            mll_r, dn, dm, dk = tw.mll_grad()
            g, g_r = np.concatenate([[gn, gm], gk]), np.concatenate([[dn, dm], dk])
            s = {"L L' - cK_w": float(np.max(np.abs(L @ L.T - tw.cK)) / (1e-9 * np.abs(tw.cK).max())),
                 "alpha": float(np.max(np.abs(alpha - tw.alpha) / (1e-6 * np.abs(tw.alpha) + 1e-9 * np.abs(tw.alpha).max()))),
                 "mu": float(np.max(np.abs(mu - mu_r) / (1e-5 * np.abs(mu_r) + 1e-5 * np.abs(mu_r).max()))),
                 "var": float(np.max(np.abs(var - var_r) / (1e-5 * np.abs(var_r) + 1e-6 * s2f))),
                 "mll": abs(mll - mll_r) / (rr.MLL_RTOL * abs(mll_r)), "mll_grad": float(np.max(np.abs(g - g_r) / rr.grad_bound(g_r)))}
            print(f"  jittered weighted handle, J = {J:.6g}, {tw.n} sites{' (three appended)' if with_append else ''}: worst share of each bound: "
                  + ", ".join(f"{k} {v:.2e}" for k, v in s.items()))
            assert all(v <= 1.0 for v in s.values()), s
            assert mll == m.mll()
    finally:
        m.close()


# ==== fresh handles at the edge sizes ===================================================================================================
@pytest.mark.parametrize("acq", ["EI", "UCB"])
@pytest.mark.parametrize("N", [256, 383, 384, 385])
def test_fresh_handles_where_the_alpha_row_is_alone(bohip, N, acq):  # noqa: F811
    """The sizes test_prune_gpu.test_row_tiles_1_to_4 (100, 200, 300, 450) steps over: at N = 256 and 384 round 1's last row tile holds
    nothing but the alpha row, 383 fills the tile before it, 385 is the first observation beside it.  R = 700: the value-only record
    is the full pass's through the poison, and the call pruned."""
    from test_prune_gpu import model, problem

    X, y, ll_ = problem(N, 4, seed=N)
    m = model(bohip, X, y, ll_)
    Xs = np.random.default_rng(N + 1).random((700, 4))
    try:
        w = through_the_poison(m, acq, [y.max()] if acq == "EI" else [1.0], Xs)
        print(f"  fresh N={N} {acq}: round 2's list length {w}")
    finally:
        m.close()
