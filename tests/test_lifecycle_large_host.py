"""The CPU-side conditions of the large life-cycle tests (tests/test_lifecycle_large_gpu.py): the history takes the routes it was
written for (checked against constants read from the sources), the twins are held to the C oracle and to np.longdouble, the arg-max
exemption stays the exception, the history's pruned calls do not start the back-off, and the weighted checks are not vacuous."""
import math
import os
import re

import numpy as np
import pytest

import lifecycle_inputs as li
import lifecycle_large_inputs as ll
import rep_reference as rr
from conftest import var_tol
from matern_reference import acq_value
from oracle.oracle import fit_with_jitter

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bayesianoptimization.jl_amd", "csrc")


def constant(file, name):
    with open(os.path.join(CSRC, file)) as f:
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", f.read())
    assert m, (file, name)
    return int(m.group(1))


def test_the_history_takes_the_routes_of_its_table():
    assert constant("common.h", "TILE") == ll.TILE == 128 and constant("common.h", "CTILE") == 64
    assert constant("kernels_linalg.hip", "APPEND_PMAX") == ll.APPEND_PMAX
    assert constant("bohip.hip", "PRUNE_R_MAX") == ll.PRUNE_R_MAX and constant("bohip.hip", "PRUNE_K1") == ll.SELECT_K1
    assert constant("bohip.hip", "SMALL_MAX") == 256
    with open(os.path.join(CSRC, "bohip.hip")) as f:
        src = f.read()
    assert "return g_split && row_tiles(g) >= 8;" in src and "if (CT64 * T >= 512) return sp;" in src          # split_applicable, split_plan
    assert "while ((double)m * (m + 1) < 0.02 * T * (T + 1)) ++m;" in src                                        # prune_tiles
    assert "(20 + 260000 / std::max<int64_t>(g->n, 1)) / 16 * 16" in src and "90 + 300000 / std::max<int64_t>(g->n, 1)" in src

    p = ll.plan()
    appends = [s for s in p if s["action"] == "append"]
    refits = [(s["n"], s["cap"], s["ld"]) for s in appends if s["route"] == "refit"]
    assert refits == [(250, 260, 400), (261, 520, 656), (521, 1040, 1168), (1041, 2080, 2192)]
    assert all(s["arg"] <= ll.APPEND_PMAX for s in appends if s["route"] == "incremental")
    calls = {s["arg"]: s for s in p if s["action"] == "call"}
    assert {k: v["n"] for k, v in calls.items()} == ll.N_AT and {k: v["cap"] for k, v in calls.items()} == ll.CAP_AT
    assert [calls[k]["ld"] for k in ("warm", "A", "B0", "B", "C", "D", "E")] == [400, 400, 656, 656, 656, 1168, 2192]
    assert [calls[k]["refits"] for k in ("warm", "A", "B0", "B", "C", "D", "E")] == [1, 1, 2, 2, 3, 4, 5]       # C: the stale handle is factored again
    assert [calls[k]["appends"] for k in ("warm", "A", "B0", "B", "C", "D", "E")] == [0, 2, 6, 7, 7, 19, 24]
    # the steps 255 -> 256, 383 -> 384 and 1040 -> 1041 are single rows; the first two are incremental, the last one grows the handle
    ones = [(s["n"], s["route"]) for s in appends if s["arg"] == 1]
    assert ones == [(256, "incremental"), (384, "incremental"), (1041, "refit")]
    for ck, lo in ll.APPENDED_FROM.items():                                 # the rows appends wrote since the last refit
        last_refit = max(s["n"] for s in p if s["route"] == "refit" and s["n"] <= ll.N_AT[ck])
        assert lo == (ll.N_AT[ck] if ck == "C" else last_refit), ck
    # row tiles, the bounding prefix, and where the alpha row sits: alone in the last tile at A, B, C and D
    T = {k: ll.row_tiles(n) for k, n in ll.N_AT.items()}
    assert T == {"warm": 2, "A": 3, "B0": 3, "B": 4, "C": 4, "D": 8, "E": 9}
    assert ll.prune_tiles(2) == 0 and all(ll.prune_tiles(T[k]) == 2 for k in ll.CHECKPOINTS)
    assert all(ll.N_AT[k] % ll.TILE == 0 for k in ("A", "B", "C", "D")) and ll.N_AT["B0"] % ll.TILE == ll.TILE - 1
    # the row pieces (trigemm_pieces): the last tile is a half piece when its live rows fit the upper half -- at A, not at B0, same T
    live = {k: ll.N_AT[k] + 1 - (T[k] - 1) * ll.TILE for k in ll.CHECKPOINTS}
    assert live["A"] == 1 and live["B0"] == ll.TILE and T["A"] == T["B0"]
    # routes: the small one at R = 40 everywhere, whole-K at 700 up to C, split-K at 700 at D and E, pruned for both value-only batches
    assert ll.small_limit(896) == 256 and (20 + 260000 // 896) // 16 * 16 == 304
    for k in ll.CHECKPOINTS:
        n = ll.N_AT[k]
        assert ll.route_of(n, ll.R_SMALL) == "small"
        assert ll.route_of(n, ll.R_MID) == ("split" if k in ("D", "E") else "whole")
        assert ll.route_of(n, ll.R_MID, hint=1 << 20) == "whole"
        Rb, Rs = ll.R_PRUNE[k]
        assert Rs < Rb <= ll.PRUNE_R_MAX and Rb % 64 and Rs % 64
        assert ll.route_of(n, Rb, value_only=True) == ll.route_of(n, Rs, value_only=True) == "pruned"
        assert ll.route_of(n, Rb) == "whole"
    assert ll.route_of(250, 700, value_only=True) == "whole"                # warm: two row tiles do not prune
    assert ll.R_PRUNE["D"][0] >= 4096 and ll.route_of(896, 4032, value_only=True) == "split"


def test_the_weighted_history_turns_weighted_where_it_says():
    pos, evals, _ = ll.weighted_data()
    reps = np.array([v.size for v in evals])
    assert np.all(reps[:ll.N_PLAIN] == 1) and np.any(reps[ll.N_PLAIN:ll.N_PLAIN + 5] > 1)      # the first sites append turns the handle
    assert np.all(reps[[255, 383, 1040]] == 3) and reps.max() == 5 and np.count_nonzero(reps[ll.N_PLAIN:] == 1) >= (ll.N_END - ll.N_PLAIN) / 5


# ---- the twins ---------------------------------------------------------------------------------------------------------------------------
def test_the_plain_twins_against_the_oracle_and_longdouble(orc):
    """Checkpoint B: the SEArd twin against the C oracle, the Mat32Iso twin (a family the C oracle does not have) against RepTwin in
    np.longdouble with every weight 1 -- mu, sigma^2 and the scores within a thousandth of the bounds the device is held to."""
    for kern, d in ll.PAIRS:
        ck = ll.checkpoint(kern, d, "B")
        R = ll.R_MID
        mu, var = ll.moments(kern, d, "B", False, R)
        if kern == "SEArd":
            L, alpha = orc.fit(ck.X, ck.y, ck.ll, ck.lsig, ck.lnoise, ck.beta)
            mu_q, var_q = orc.predict(ck.X, ck.ll, ck.lsig, ck.beta, L, alpha, ck.Xs[:R])
        else:
            tq = rr.RepTwin(kern, ck.X, ck.y, np.ones(ck.n, dtype=np.int64), np.zeros(ck.n), ck.ll, ck.lsig, ck.lnoise, ck.beta, dtype=np.longdouble)
            mu_q, var_q = (np.asarray(a, dtype=np.float64) for a in tq.predict(ck.Xs[:R]))
        s_mu = float(np.max(np.abs(mu - mu_q) / (1e-6 * np.abs(mu_q) + ck.floor)))
        s_var = float(np.max(np.abs(var - var_q) / var_tol(var_q, ck.n, ck.s2f)))
        worst = {"mu": s_mu, "var": s_var}
        for acq in ll.ACQS:
            p = ck.params(acq)
            sc, fl = ll.twin_scores(ck, acq, R)
            sc_q = acq_value(acq, p, mu_q, var_q)
            worst[acq] = float(np.max(np.abs(sc - sc_q) / (1e-6 * np.abs(sc_q) + fl)))
        print(f"{ck}: the twin against {'the C oracle' if kern == 'SEArd' else 'np.longdouble'}, shares of the device's bounds: "
              + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        assert max(worst.values()) <= 1e-3, worst


def test_the_weighted_twin_against_the_expanded_oracle(orc):
    """Checkpoint B of the weighted handle: RepTwin's MaternGP shell is RepTwin (its own substitutions), and both are the model with
    every evaluation as a row of its own (the C oracle) within a thousandth of the device's bounds, as tests/test_rep_host.py holds
    the twin at its sizes."""
    kern, d = ll.WEIGHTED
    ck = ll.checkpoint(kern, d, "B", True)
    R = ll.R_MID
    mu, var = ll.moments(kern, d, "B", True, R)
    mu_t, var_t = ck.tw.predict(ck.Xs[:R])
    pos, evals, _ = ll.weighted_data()
    X, y = rr.expand(pos, evals, 0, ck.n)
    ex = rr.Expanded(kern, X, y, ck.ll, ck.lsig, ck.lnoise, ck.beta, orc)
    mu_o, var_o = ex.predict(ck.Xs[:R])
    worst = {}
    for what, (a, b) in {"shell vs twin": ((mu, var), (mu_t, var_t)), "twin vs expanded": ((mu_t, var_t), (mu_o, var_o))}.items():
        worst[what + " mu"] = float(np.max(np.abs(a[0] - b[0]) / (1e-6 * np.abs(b[0]) + ck.floor)))
        worst[what + " var"] = float(np.max(np.abs(a[1] - b[1]) / var_tol(b[1], ck.n, ck.s2f)))
    print(f"{ck} ({len(y)} evaluations): shares of the device's bounds: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-3, worst


# ---- the arg-max exemption and the back-off -------------------------------------------------------------------------------------------------
def test_argmax_exemptions_are_rare_and_no_pruned_call_backs_off():
    """test_seeded_vs_oracle's near-tie rule recomputed from the reference alone over every (handle, checkpoint, acquisition, R) of the
    device test: at most one case in ten may take it.  And the model of round 2's list (prefix_survivors) stays below R / 8 in every
    case, so that no value-only call of the history sends its handle into prune_wanted's back-off."""
    cases = ll.argmax_cases()
    exempt = [c for c in cases if ll.exempt(c)]
    worst = 0
    for k, d, w, name, acq, R in cases:
        n2 = ll.prefix_survivors(ll.checkpoint(k, d, name, w), acq, R)
        worst = max(worst, n2)
        assert 8 * n2 <= min(r for rs in ll.R_PRUNE.values() for r in rs), ((k, d, w, name, acq, R), n2)
    print(f"arg-max exemptions: {len(exempt)} of {len(cases)}: {exempt}; longest modelled round-2 list: {worst}")
    assert len(cases) == 3 * 6 * 3 * 2 and 10 * len(exempt) <= len(cases), exempt
    # the calls with DUP_K copies of the winner list DUP_K - 64 ... DUP_K - 1 candidates (other candidates may have higher bounds and take
    # places of round 1); the value-only call that follows one of them has the larger batch, at least R_MID: still no back-off
    assert 8 * (ll.DUP_K - 1 + worst) <= ll.R_MID == min(rs[0] for rs in ll.R_PRUNE.values()) and ll.DUP_K - ll.SELECT_K1 > 8
    Xd, dup = ll.dup_set(ll.checkpoint("SEArd", 3, "A"), "EI", 700)
    assert len(dup) == ll.DUP_K == len(set(dup.tolist())) and np.all(Xd[dup] == Xd[dup[0]])


# ---- non-vacuity of the weighted history ----------------------------------------------------------------------------------------------------
def test_ignoring_the_weights_misses_by_a_wide_factor():
    """At E, the largest checkpoint: a twin with ignore_weights=True (what a library computes that stores the sites and forgets
    1 / r_i) misses the device's bounds on mu, on mll and on the logNoise gradient a hundred times over, as tests/test_rep_host.py
    shows at its sizes; and at D, where the factor is incremental, so does one whose diagonal lacks the weights of the rows that appends
    wrote (append_incremental without its k_rep_diag launch)."""
    kern, d = ll.WEIGHTED
    R = 512
    for name, what, lo in (("E", "every weight", None), ("D", "the weights of the appended rows 521 ... 895", ll.APPENDED_FROM["D"])):
        ck = ll.checkpoint(kern, d, name, True)
        Xs = ck.Xs[:R]
        mu, _ = ck.tw.predict(Xs)
        m, dn, _, _ = ck.tw.mll_grad()
        bad = (rr.RepTwin(kern, ck.X, ck.y, ck.reps, ck.ss, ck.ll, ck.lsig, ck.lnoise, ck.beta, ignore_weights=True) if lo is None
               else BadDiag(kern, ck, np.where(np.arange(ck.n) >= lo, 1, ck.reps)))
        mu_b, _ = bad.predict(Xs)
        m_b, dn_b, _, _ = bad.mll_grad()
        s_mu = float(np.max(np.abs(mu_b - mu) / rr.mu_bound(mu, ck.tw.alpha, ck.s2f)))
        s_mll = float(abs(m_b - m) / (rr.MLL_RTOL * abs(m)))
        s_g = float(abs(dn_b - dn) / rr.grad_bound(np.array([dn, 0.0]))[0])
        print(f"{ck}: {what} ignored: mu {s_mu:.1e} mll {s_mll:.1e} logNoise gradient {s_g:.1e} bounds away")
        assert min(s_mu, s_mll, s_g) >= 100.0


class BadDiag(rr.RepTwin):
    """RepTwin whose DIAGONAL uses other repetition counts than its site constant: a factor whose appended rows missed k_rep_diag."""

    def __init__(self, kern, ck, diag_reps):
        super().__init__(kern, ck.X, ck.y, diag_reps, ck.ss, ck.ll, ck.lsig, ck.lnoise, ck.beta)
        self.reps = np.asarray(ck.reps, dtype=np.int64)                     # (site_constant and the noise gradient keep the true counts)


# ---- jitter on a weighted handle --------------------------------------------------------------------------------------------------------------
def test_the_jittered_weighted_model(orc):
    """The 300 sites are singular without jitter whatever the weights; with J = 1e-3 mean(diag) -- what oracle.fit_with_jitter adds on
    its first try -- cK_w factors, and a twin without J or without the weights is far outside the bounds the device is held to."""
    X, ybar, reps, ss, Xa, ya, ra, sa = ll.jitter_sites()
    assert reps.min() == 1 and reps.max() == 5 and np.any(ra > 1)
    _, _, tries, J = fit_with_jitter(orc, X, ybar, li.JIT_LL, li.JIT_LSIG, li.JIT_LNOISE, li.JIT_BETA, li.JIT_REL, li.JIT_TRIES)
    assert tries == 1 and J == li.JIT_REL * (math.exp(2.0 * li.JIT_LSIG) + math.exp(2.0 * li.JIT_LNOISE))
    with pytest.raises(np.linalg.LinAlgError):
        ll.jitter_twin(0.0)
    tw = ll.jitter_twin(J)
    tq = ll.jitter_twin(J, dtype=np.longdouble)
    Xs = li.jitter_candidates(64)
    s2f = math.exp(2.0 * li.JIT_LSIG)
    mu, var = tw.predict(Xs)
    mu_q, var_q = tq.predict(Xs)
    tol_mu, tol_var = 1e-5 * np.abs(mu) + 1e-5 * np.abs(mu).max(), 1e-5 * np.abs(var) + 1e-6 * s2f
    share = max(float(np.max(np.abs(mu - mu_q) / tol_mu)), float(np.max(np.abs(var - var_q) / tol_var)),
                float(abs(tw.mll() - tq.mll()) / (rr.MLL_RTOL * abs(tw.mll()))))
    print(f"J = {J:.6g}, kappa_2(cK_w + J / r) = {np.linalg.cond(tw.cK):.3g}; float64 twin against np.longdouble: {share:.1e} of the device's bounds")
    assert share <= 1e-1
    for what, bad in (("the weights", ll.jitter_twin(J, ignore_weights=True)), ("a tenth of J", ll.jitter_twin(0.9 * J))):
        mu_b, var_b = bad.predict(Xs)
        moved = max(float(np.max(np.abs(mu_b - mu) / tol_mu)), float(np.max(np.abs(var_b - var) / tol_var)))
        moved_mll = float(abs(bad.mll() - tw.mll()) / (rr.MLL_RTOL * abs(tw.mll())))
        print(f"a twin without {what}: posterior {moved:.3g}, mll {moved_mll:.3g} x the bounds away")
        assert moved_mll > 100.0
