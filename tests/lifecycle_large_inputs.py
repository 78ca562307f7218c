"""Inputs of the large life-cycle tests (tests/test_lifecycle_large_gpu.py, tests/test_lifecycle_large_host.py).  No device.  A helper,
not a test module.

tests/lifecycle_inputs.py ends at 206 observations: two row tiles, where a handle can take neither the pruned arg-max (prune_tiles
needs three) nor split-K (split_applicable needs eight).  The history here is the smallest that takes a handle through both, with the
same ingredients -- incremental appends, capacity growth (a re-allocation with another leading dimension), a change of every
hyper-parameter with no fit_() behind it -- and through the sizes at which the alpha row (row N of W) sits alone in the last row tile:

    warm  N = 250, capacity 260 (ld = 400), T = 2: value-only and scored calls, so that the score scratch and K*' exist before any pruning
    A     255 -> 256 by an incremental append of ONE row: T = 3, the bounding prefix m = 2, tile 2 holds the alpha row alone; the
          handle's first pruned call
    B0    261 rows pass the capacity (520, ld = 656, a refit), incremental appends to 383: T = 3 still, but the alpha row now ends a
          FULL last tile -- the row pieces change (a whole tile where A had a half piece) while T does not (ensure_pieces' key)
    B     383 -> 384: T = 4, the alpha row alone again; the factor is incremental, refit rows and appended rows both in the prefix
    C     every hyper-parameter changed, no fit_(): the first reader refits (a dataflow Cholesky with a factorisation task, T = 4)
    D     137 rows (past APPEND_PMAX and past the capacity: 1040, ld = 1168, a refit), incremental appends to 896: T = 8, split-K
    E     incremental appends to 1040, one more row: capacity 2080, ld = 2192, T = 9; every buffer sized by ld is made again

`plan` is lifecycle_inputs.plan on this history.  Three handles live it: the two pairs of lifecycle_inputs.PAIRS, and a SEArd d = 3
handle that turns weighted (replicated sites, bohip_gp_append_sites) with its first append after the plain fill; its twin is
rep_reference.RepTwin in float64, carried by a MaternGP shell (the twin's L and alpha under MaternGP's posterior and gradient formulas)."""
import functools
import math

import numpy as np

import lifecycle_inputs as li
import rep_reference as rr
from conftest import synth
from high_dim_inputs import near_tie, score_floor
from matern_reference import MaternGP, acq_value, first_argmax

EPS = li.EPS
TILE, APPEND_PMAX = li.TILE, li.APPEND_PMAX
PAIRS = li.PAIRS
WEIGHTED = ("SEArd", 3)                                                     # the pair of the weighted handle
HANDLES = tuple((k, d, False) for k, d in PAIRS) + ((WEIGHTED[0], WEIGHTED[1], True),)
CAPACITY = 260
N_END = 1041
PRUNE_R_MAX, SELECT_K1 = 8192, 64                                           # csrc/bohip.hip PRUNE_R_MAX, PRUNE_K1


def _appends(n_from, n_to, step=APPEND_PMAX):
    out, n = [], n_from
    while n < n_to:
        out.append(("append", min(step, n_to - n)))
        n += out[-1][1]
    return out


HISTORY = tuple([("append", 250), ("call", "warm"), ("append", 5), ("append", 1), ("call", "A"), ("append", 5)]
                + _appends(261, 383) + [("call", "B0"), ("append", 1), ("call", "B"), ("hyper", None), ("call", "C"), ("append", 137)]
                + _appends(521, 896) + [("call", "D")] + _appends(896, 1040) + [("append", 1), ("call", "E")])
N_AT = {"warm": 250, "A": 256, "B0": 383, "B": 384, "C": 384, "D": 896, "E": 1041}
CAP_AT = {"warm": 260, "A": 260, "B0": 520, "B": 520, "C": 520, "D": 1040, "E": 2080}
CHECKPOINTS = ("A", "B0", "B", "C", "D", "E")
APPENDED_FROM = {"A": 250, "B0": 261, "B": 261, "C": 384, "D": 521, "E": 1041}      # rows [lo, n): written by appends since the last refit
N_PLAIN = 250                                                               # the weighted handle's first fill: rows of one evaluation

# candidate counts: the pruned route's larger batch (no multiple of 64), then the smaller; the small route; the whole-K / split-K one
R_SMALL, R_MID = 40, 700
R_PRUNE = {"A": (700, 321), "B0": (700, 321), "B": (700, 321), "C": (700, 321), "D": (4100, 4037), "E": (4100, 4037)}
R_MAX = 4100
ACQS = ("EI", "UCB", "PI")
UCB_KAPPA = 2.0
DUP_K = 73                                                                  # copies of the winner: round 1 holds 64, round 2 lists >= 9 (past a column group of 8)


def row_tiles(n):
    """csrc/bohip.hip row_tiles: the observations and the alpha row."""
    return -(-(n + 1) // TILE)


def prune_tiles(T):
    """csrc/bohip.hip prune_tiles: the smallest m >= 2 whose triangle holds 2 % of the contraction's; 0: no pruning."""
    m = 2
    while m * (m + 1) < 0.02 * T * (T + 1):
        m += 1
    return m if m < T else 0


def split_applicable(n):
    return row_tiles(n) >= 8


def small_limit(n):
    """csrc/bohip.hip small_limit (SMALL_MAX = 256)."""
    if split_applicable(n):
        return min(256, max(16, (20 + 260000 // max(n, 1)) // 16 * 16))
    return min(256, 90 + 300000 // max(n, 1))


def route_of(n, R, value_only=False, hint=0):
    """choose_route restated: "small", "split", "pruned" or "whole" (a value-only call whose handle has not backed off)."""
    Rp = max(R, hint)
    if Rp <= small_limit(n) and R <= 256:
        return "small"
    if split_applicable(n) and -(-Rp // 64) * row_tiles(n) < 512:
        return "split"
    if value_only and hint == 0 and prune_tiles(row_tiles(n)) > 0 and R <= PRUNE_R_MAX:
        return "pruned"
    return "whole"


def plan(reads_model=True):
    return li.plan(HISTORY, CAPACITY, reads_model)


# ---- data ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data(kern, d):
    """(X[1041, d], y, Xs[4100, d]) of a plain pair, read-only."""
    X, y, Xs = synth(N_END, d, R_MAX, seed=5000 + 3 * d)
    for a in (X, y, Xs):
        a.setflags(write=False)
    return X, y, Xs


W_LNOISE, W_LSIG = rr.HYPERS[0]
W_SEED = 7300


@functools.lru_cache(maxsize=None)
def weighted_data():
    """(pos[1041, 3], evals, Xs[4100, 3]) of the weighted handle, rep_reference.raw's recipe: r_i from draw_reps, the first N_PLAIN
    sites cut to one evaluation (the plain fill), and the three sites that arrive alone (rows 255, 383, 1040: each lands as the last
    row before the alpha row moves into a tile of its own) given three evaluations, so that a missed weight there cannot hide."""
    rng = np.random.default_rng(W_SEED)
    pos = rng.random((N_END, rr.D))
    reps = rr.draw_reps(N_END, rng)
    reps[:N_PLAIN] = 1
    reps[[255, 383, 1040]] = 3
    f = math.exp(W_LSIG) * np.sin(3 * pos).sum(1)
    evals = tuple(f[i] + math.exp(W_LNOISE) * rng.standard_normal(int(reps[i])) for i in range(N_END))
    Xs = rng.random((R_MAX, rr.D))
    for a in (pos, Xs) + evals:
        a.setflags(write=False)
    return pos, evals, Xs


def hyper(kern, name, weighted=False):
    after = name in ("C", "D", "E")
    if weighted:
        return rr.hyper_after(kern, W_LNOISE, W_LSIG) if after else (rr.LL[kern], W_LSIG, W_LNOISE, rr.BETA)
    return li.HYPER[kern][1 if after else 0]


class WeightedGP(MaternGP):
    """rep_reference.RepTwin (float64) under MaternGP's formulas: cK_w = K + nu diag(1 / r), the twin's own L and alpha."""

    def __init__(self, tw, kern, X, ybar, ll, lsig, lnoise, beta):
        self.kern, self.fam = kern, tw.fam
        self.X, self.y = np.array(X, dtype=np.float64), np.array(ybar, dtype=np.float64)
        self.N, self.d = self.X.shape
        self.loglen = np.atleast_1d(np.asarray(ll, dtype=np.float64)).copy()
        self.logsig, self.lognoise, self.beta = float(lsig), float(lnoise), float(beta)
        self.s2f, self.il2, self.noise = float(tw.s2f), np.asarray(tw.il2, dtype=np.float64), float(tw.nu)
        self.cK, self.L, self.alpha = tw.cK, tw.L, tw.alpha

    def mll(self):
        raise NotImplementedError("the weighted likelihood is the twin's (site_constant)")

    mll_grad = mll


class Checkpoint(li.Checkpoint):
    """lifecycle_inputs.Checkpoint on this history; weighted: X the sites, y their means, tw the RepTwin, ref its MaternGP shell."""

    def __init__(self, kern, d, name, weighted=False):
        self.kern, self.d, self.name, self.n, self.weighted = kern, d, name, N_AT[name], weighted
        self.hyp = hyper(kern, name, weighted)
        self.ll, self.lsig, self.lnoise, self.beta = self.hyp
        if weighted:
            pos, evals, Xs = weighted_data()
            _, ybar, reps, ss, _ = rr.sites_of(pos, evals, 0, self.n)
            self.X, self.y, self.Xs, self.reps, self.ss = pos[:self.n], ybar, Xs, reps, ss
            self.tw = rr.RepTwin(kern, self.X, ybar, reps, ss, self.ll, self.lsig, self.lnoise, self.beta)
            self.ref = WeightedGP(self.tw, kern, self.X, ybar, self.ll, self.lsig, self.lnoise, self.beta)
            # the best single evaluation lies ten posterior deviations above this model's mean (five evaluations a site, noise e^-2):
            # EI and PI underflow to a tie at 0 there.  The 98th percentile of the site means is an incumbent the mean exceeds somewhere
            self.tau = float(np.quantile(ybar, 0.98))
        else:
            X, y, Xs = data(kern, d)
            self.X, self.y, self.Xs = X[:self.n], y[:self.n], Xs
            self.ref = MaternGP(kern, self.X, self.y, self.ll, self.lsig, self.lnoise, self.beta)
            self.tau = float(self.y.max())                                  # test_seeded_vs_oracle's incumbent
        self.s2f = self.ref.s2f
        self.floor = 64 * EPS * self.s2f * np.abs(self.ref.alpha).sum()     # test_parity_gpu.mu_floor

    def __repr__(self):
        return f"{self.kern} d={self.d}{' weighted' if self.weighted else ''} checkpoint {self.name} (N = {self.n})"

    def params(self, acq):
        return [UCB_KAPPA] if acq == "UCB" else [self.tau]


@functools.lru_cache(maxsize=None)
def checkpoint(kern, d, name, weighted=False):
    return Checkpoint(kern, d, name, weighted)


@functools.lru_cache(maxsize=None)
def moments(kern, d, name, weighted, R):
    """(mu, sigma^2) of the twin over the first R candidates, read-only."""
    ck = checkpoint(kern, d, name, weighted)
    mu, var = ck.ref.predict(ck.Xs[:R])
    mu.setflags(write=False)
    var.setflags(write=False)
    return mu, var


def twin_scores(ck, acq, R):
    """(scores, floor) of the twin: test_seeded_vs_oracle's floor of a score (high_dim_inputs.score_floor)."""
    mu, var = moments(ck.kern, ck.d, ck.name, ck.weighted, R)
    p = ck.params(acq)
    return acq_value(acq, p, mu, var), score_floor(acq, p, ck.floor, var, ck.n, ck.s2f)


def dup_set(ck, acq, R):
    """test_prune_round2_gpu's recipe for a round-2 list of a wanted length, on the twin: the twin's winner among the first R candidates
    copied to DUP_K indices.  The copies share one bound and one score, round 1 holds at most SELECT_K1 of them and every copy outside
    it has bound >= score = round 1's best: the list has at least DUP_K - SELECT_K1 entries, and the lowest index of the tie must win.
    -> (Xs[R, d], the indices in ascending order)."""
    i_best = first_argmax(twin_scores(ck, acq, R)[0])[1]
    rng = np.random.default_rng(R + DUP_K + ck.n)
    dup = np.sort(np.append(rng.choice(np.setdiff1d(np.arange(R), [i_best]), DUP_K - 1, replace=False), i_best))
    Xs = ck.Xs[:R].copy()
    Xs[dup] = Xs[i_best]
    return Xs, dup


def argmax_cases():
    """Every (kern, d, weighted, checkpoint, acquisition, R) whose winner the device test compares with the twin's."""
    return [(k, d, w, name, acq, R) for k, d, w in HANDLES for name in CHECKPOINTS for acq in ACQS for R in R_PRUNE[name]]


def exempt(case):
    """test_seeded_vs_oracle's near-tie rule, from the reference alone."""
    k, d, w, name, acq, R = case
    sc, fl = twin_scores(checkpoint(k, d, name, w), acq, R)
    return near_tie(sc, fl)


def prefix_survivors(ck, acq, R):
    """A model of round 2's list length from the twin alone: the bound of a candidate is its score with the variance of the first
    m row tiles' contraction only (sigma^2 <= s_f^2 - |V[:128 m]|^2); round 1 scores the SELECT_K1 highest bounds exactly, and every
    other candidate whose bound is not below round 1's best survives.  The device's bounds carry rounding slack on top, so its list
    is at least this long; the model shows that the history's pruned calls stay far below the back-off's R / 8."""
    import scipy.linalg as sl

    m = prune_tiles(row_tiles(ck.n))
    Ks = ck.ref.kstar(ck.Xs[:R])[:TILE * m]
    V = sl.solve_triangular(ck.ref.L[:TILE * m, :TILE * m], Ks, lower=True)
    mu, _ = moments(ck.kern, ck.d, ck.name, ck.weighted, R)
    p = ck.params(acq)
    ub = acq_value(acq, p, mu, np.maximum(ck.s2f - np.sum(V * V, axis=0), 0.0))
    sc, _ = twin_scores(ck, acq, R)
    order = np.lexsort((np.arange(R), -ub))
    first = order[:SELECT_K1]
    outside = np.ones(R, bool)
    outside[first] = False
    return int(np.count_nonzero(outside & ~(ub < sc[first].max())))


# ---- jitter on a weighted handle ---------------------------------------------------------------------------------------------------------
JIT_SEED = 23


@functools.lru_cache(maxsize=None)
def jitter_sites():
    """lifecycle_inputs.jitter_data's singular model (test_hardening_gpu's: 60 positions, each five times) as 300 SITES of 1 to 5
    evaluations: (X, ybar, reps, ss, Xa, ya, reps_a, ss_a).  The repeated positions keep K singular whatever the weights are."""
    X, y, Xa, ya = li.jitter_data()
    rng = np.random.default_rng(JIT_SEED)
    reps = rr.draw_reps(len(y) + len(ya), rng)
    ss = np.where(reps > 1, rng.random(len(reps)) * (reps - 1), 0.0)
    n = len(y)
    return X, y, reps[:n], ss[:n], Xa, ya, reps[n:], ss[n:]


def jitter_twin(J, with_append=False, dtype=np.float64, ignore_weights=False):
    X, y, reps, ss, Xa, ya, ra, sa = jitter_sites()
    if with_append:
        X, y, reps, ss = np.vstack([X, Xa]), np.concatenate([y, ya]), np.concatenate([reps, ra]), np.concatenate([ss, sa])
    return rr.RepTwin("SEArd", X, y, reps, ss, li.JIT_LL, li.JIT_LSIG, li.JIT_LNOISE, li.JIT_BETA, dtype=dtype, jitter=J,
                      ignore_weights=ignore_weights)
