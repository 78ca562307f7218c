"""NumPy references of optimisation with two to four objectives (include/bohip_mom.h).  No device.  A helper, not a
test module.

The float64 twin follows the library operation for operation (the device differs from it in exp and erfc -- libm's here):
  front(Y, ref)                        the observed front [M, n_front], lexicographic ascending, and its hypervolume -- bohip_mom_front
  boxes(fr, ref)                       the level arrays and the boxes [2M, n_boxes] of the slab recursion -- bohip_mom_boxes
  ehvi(fr, ref, mu, var)               value[R], dmu[M, R], dvar[M, R] in k_ehvi_boxes' product and summation order
  gradient(pm, pv, var, jmu, jvar)     the d gradient entries from the M models' Jacobians, ascending m from +0.0
  record(values)                       the arg-max record of bohip_gp_score
  score_mom(models, front, ref, Xs)    the whole call on the members' twins (matern_reference.MaternGP)
  propagate(models, tw)                mo_reference.propagate for M members
  hvi(fr, ref, y)                      the hypervolume improvement of points y [M, S], from the boxes
The extended-precision evaluator (mpmath, 50 digits): mp_ehvi, mp_table (cached under tests/golden/ where it is slow).
"""
import hashlib
import math
import os

import numpy as np

import con_reference as cr
import mo_reference as mr

OBJ_MAX, FRONT_MAX, BOX_MAX, LANES = 4, 256, 65536, 64     # BOHIP_MOM_OBJ_MAX, _FRONT_MAX, _BOX_MAX, _LANES
EPS = np.finfo(np.float64).eps
GOLDEN = mr.GOLDEN
REF4 = np.array([-2.25, -2.125, -2.5, -2.375])


def keys(M):
    return ("value",) + tuple(f"dmu{m + 1}" for m in range(M)) + tuple(f"dvar{m + 1}" for m in range(M))


# The twin's worst error against the 50-digit evaluator over the crafted grid of tests/test_mom_host.py (GRID below, seeds
# grid_seed(M, n_front, R)), measured on the CPU with glibc's exp and SciPy's erfc as |twin - ref| / max(S, 1e-300), S the box sum with
# prod_m (Psi(l) + Psi(u)) in place of the differences (mp_ehvi), over the value and the 2M partials, rounded up to two digits:
# 1.5172e-10 -> 1.6e-10, set by d/ds2_2 at M = 2, n_front = 1, column 127 (S = 5.9e-299); the worst of the other cases is 1.46e-10
# (M = 2), 1.13e-10 (M = 3), 1.2e-11 (M = 4), and away from the tails (S > 1e-30) the M = 2, n_front = 1 case gives 1.87e-12.  As in mo_reference.WORST the maximum sits where every box is deep in a tail of one
# objective: Psi = sd phi + D Phi cancels to z^-2 of its terms while exp(-z^2 / 2) carries z^2 eps / 2.  The host test bounds the twin
# by 2 x WORST (another libm), the device tests bound the kernel by 16 x WORST, mo_reference.WORST's factors.
GRID = tuple((M, n, 257) for M in (2, 3, 4) for n in (0, 1, 2, 8, 17)) + ((3, 150, 40), (4, 24, 40))
WORST = 1.6e-10


# ---- the front and its boxes ---------------------------------------------------------------------------------------------------------
def _nondominated(P, dim):
    """The non-dominated subset of the projections of P (tuples) on the first dim coordinates: weak dominance, of equal ones one."""
    Q = sorted({p[:dim] for p in P})
    return [p for p in Q if not any(q != p and all(a >= b for a, b in zip(q, p)) for q in Q)]


def _slabs(P, dim, nl):
    return [0] + sorted({p[dim - 1] for p in P}) + [nl - 1]


def levels_of(fr, ref):
    return [np.concatenate([[ref[m]], np.unique(fr[m]), [np.inf]]) for m in range(fr.shape[0])]


def _index(fr, L):
    """The points as tuples of level indices (1 .. n_levels - 2)."""
    M, n = fr.shape
    return [tuple(int(np.searchsorted(L[m][1:-1], fr[m, i])) + 1 for m in range(M)) for i in range(n)]


def _decomp(P, dim, nls, hi_tail, lo_tail, out):
    if dim == 1:
        out.append(((max([0] + [p[0] for p in P]),) + lo_tail, (nls[0] - 1,) + hi_tail))
        return
    z = _slabs(P, dim, nls[dim - 1])
    for j in range(len(z) - 1):
        Q = _nondominated([p for p in P if p[dim - 1] > z[j]], dim - 1)
        _decomp(Q, dim - 1, nls, (z[j + 1],) + hi_tail, (z[j],) + lo_tail, out)


def _hv(P, dim, L):
    if dim == 1:
        return L[0][max([0] + [p[0] for p in P])] - L[0][0]
    z = _slabs(P, dim, len(L[dim - 1]))
    a = 0.0
    for j in range(len(z) - 2):
        Q = _nondominated([p for p in P if p[dim - 1] > z[j]], dim - 1)
        a += (L[dim - 1][z[j + 1]] - L[dim - 1][z[j]]) * _hv(Q, dim - 1, L)
    return a


def boxes(fr, ref):
    """-> (levels: list of M arrays, B: int32 [2M, n_boxes]) of bohip_mom_boxes."""
    fr = np.asarray(fr, dtype=np.float64)
    M = fr.shape[0]
    L = levels_of(fr, ref)
    out = []
    _decomp(_index(fr, L), M, [len(l) for l in L], (), (), out)
    B = np.array([lo + hi for lo, hi in out], dtype=np.int32).reshape(-1, 2 * M).T.copy()
    return L, B


def front(Y, ref):
    """-> (front[M, n_front], hv) of bohip_mom_front."""
    Y = np.asarray(Y, dtype=np.float64)
    M = Y.shape[0]
    ref = np.asarray(ref, dtype=np.float64)
    if not np.all(np.isfinite(Y)) or not np.all(np.isfinite(ref)):
        raise ValueError("not finite")
    A = Y[:, np.all(Y > ref[:, None], axis=0)]
    keep = _nondominated([tuple(c) for c in A.T], M)
    fr = np.array(keep, dtype=np.float64).reshape(-1, M).T.copy()
    L = levels_of(fr, ref)
    return fr, _hv(_index(fr, L), M, L)


def hvi(fr, ref, y):
    """The hypervolume improvement of each column of y [M, S] over the front: the volume of the box below y (above ref) that no front
    point dominates, box by box."""
    L, B = boxes(fr, ref)
    y = np.asarray(y, dtype=np.float64)
    M = y.shape[0]
    out = np.ones((y.shape[1], B.shape[1]))
    for m in range(M):
        lo, hi = L[m][B[m]], L[m][B[M + m]]
        out *= np.clip(np.minimum(y[m][:, None], hi[None, :]) - lo[None, :], 0.0, None)
    return out.sum(axis=1)


# ---- the twin of k_ehvi_boxes ---------------------------------------------------------------------------------------------------------
def lane_sum(terms):
    """The kernel's order over the boxes (last axis): lane g adds boxes g, g + 64, ... in ascending order from +0.0, then the
    butterfly a_g <- a_g + a_{g xor o}, o = 32, 16, 8, 4, 2, 1; lane 0's result."""
    R, K = terms.shape
    acc = np.zeros((R, LANES))
    for s0 in range(0, K, LANES):
        w = min(LANES, K - s0)
        acc[:, :w] = acc[:, :w] + terms[:, s0:s0 + w]
    lanes = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def _product(factors):
    p = factors[0]
    for f in factors[1:]:
        p = p * f
    return p


def ehvi(fr, ref, mu, var):
    """-> (value[R], dmu[M, R], dvar[M, R]) of bohip_mom_ehvi_values."""
    mu, var = np.atleast_2d(np.asarray(mu, dtype=np.float64)), np.atleast_2d(np.asarray(var, dtype=np.float64))
    M = mu.shape[0]
    L, B = boxes(np.asarray(fr, dtype=np.float64).reshape(M, -1), ref)
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(mu).all(axis=0) & np.isfinite(var).all(axis=0) & (var >= 0.0).all(axis=0))
        sd = np.sqrt(var)
        dP, dF, df = [], [], []
        for m in range(M):
            P, F, f = mr.psi(mu[m][:, None], var[m][:, None], sd[m][:, None], L[m][None, :])
            lo, hi = B[m], B[M + m]
            dP.append(P[:, lo] - P[:, hi])
            dF.append(F[:, lo] - F[:, hi])
            df.append(f[:, lo] - f[:, hi])
        v = lane_sum(_product(dP))
        pm = np.stack([lane_sum(_product([dF[l] if l == m else dP[l] for l in range(M)])) for m in range(M)])
        sm = np.stack([lane_sum(_product([df[l] if l == m else dP[l] for l in range(M)])) for m in range(M)])
        pv = np.where(var > 0.0, sm / (2.0 * sd), 0.0)
        v = np.where(bad, np.nan, v)
        pm[:, bad], pv[:, bad] = np.nan, np.nan
    return v, pm, pv


def gradient(pm, pv, var, jmu, jvar):
    """grad[R, d] = sum_m pm[m] jmu[m] + (var[m] > 0) pv[m] jvar[m], ascending m from +0.0; jmu, jvar [M, R, d]."""
    g = np.zeros(jmu.shape[1:])
    with np.errstate(all="ignore"):
        for m in range(jmu.shape[0]):
            g = g + pm[m][:, None] * jmu[m]
            g = np.where((var[m] > 0.0)[:, None], g + pv[m][:, None] * jvar[m], g)
    return g


record = cr.record


def score_mom(models, fr, ref, Xs, want_grad=True):
    """The whole call on the members' twins -> dict(scores, grad[R, d], mu, var, pm, pv, jmu, jvar, best_val, best_idx)."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    R, d = Xs.shape
    M = len(models)
    mu, var, jmu, jvar = np.empty((M, R)), np.empty((M, R)), np.empty((M, R, d)), np.empty((M, R, d))
    for m, gp in enumerate(models):
        mu[m], var[m], jmu[m], jvar[m] = cr.posterior_jac(gp, Xs)
    f, pm, pv = ehvi(fr, ref, mu, var)
    g = gradient(pm, pv, var, jmu, jvar) if want_grad else None
    bv, bi = record(f)
    return dict(scores=f, grad=g, mu=mu, var=var, pm=pm, pv=pv, jmu=jmu, jvar=jvar, best_val=bv, best_idx=bi)


propagate = mr.propagate      # (it walks enumerate(models): M members as they come)


# ---- extended precision ----------------------------------------------------------------------------------------------------------------
def mp_ehvi(fr, ref, mu, var, dps=50, as_float=True, decomposition=None):
    """One candidate at 50 digits from the exact formulas: mu, var of length M (mpmath numbers or floats).
    -> (vals, scales): vals = (EHVI, d/dmu_1 .. d/dmu_M, d/ds2_1 .. d/ds2_M), scales the sums S each of them cancels against (the
    same box sums with + in place of every difference)."""
    import mpmath as mp

    M = len(mu)
    L, B = decomposition if decomposition is not None else boxes(np.asarray(fr, dtype=np.float64).reshape(M, -1), ref)
    with mp.workdps(dps):
        def three(m, v, t):
            if t == np.inf:
                return mp.mpf(0), mp.mpf(0), mp.mpf(0)
            D = m - mp.mpf(float(t))
            if v == 0:
                return (D if D > 0 else mp.mpf(0)), (mp.mpf(1) if D > 0 else mp.mpf(0)), mp.mpf(0)
            sd = mp.sqrt(v)
            z = D / sd
            Phi, phi = mp.ncdf(z), mp.npdf(z)
            return sd * phi + D * Phi, Phi, phi

        ms, vs = [mp.mpf(x) for x in mu], [mp.mpf(x) for x in var]
        h = [1 / (2 * mp.sqrt(v)) if v > 0 else mp.mpf(0) for v in vs]
        tabs = [[three(ms[m], vs[m], t) for t in L[m]] for m in range(M)]
        vals, scales = [mp.mpf(0)] * (1 + 2 * M), [mp.mpf(0)] * (1 + 2 * M)
        one = mp.mpf(1)
        for b in range(B.shape[1]):
            lo = [tabs[m][B[m, b]] for m in range(M)]
            hi = [tabs[m][B[M + m, b]] for m in range(M)]
            d0, s0 = [lo[m][0] - hi[m][0] for m in range(M)], [lo[m][0] + hi[m][0] for m in range(M)]
            for k in range(1 + 2 * M):
                pd, ps = one, one
                for m in range(M):
                    if k == 1 + m:
                        pd, ps = pd * (lo[m][1] - hi[m][1]), ps * (lo[m][1] + hi[m][1])
                    elif k == 1 + M + m:
                        pd, ps = pd * (lo[m][2] - hi[m][2]) * h[m], ps * (lo[m][2] + hi[m][2]) * h[m]
                    else:
                        pd, ps = pd * d0[m], ps * s0[m]
                vals[k], scales[k] = vals[k] + pd, scales[k] + ps
        if as_float:
            return [float(x) for x in vals], [float(x) for x in scales]
        return vals, scales


def _case_file(M, n_front, R, seed):
    return os.path.join(GOLDEN, f"mom_mp_M{M}_n{n_front}_R{R}_s{seed}.npz")


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def mp_table(fr, ref, mu, var, cache=None):
    """mp_ehvi over the columns whose moments are valid -> dict of keys(M) -> [R] and "S_" + key -> [R]; NaN columns elsewhere.
    cache = (M, n_front, R, seed) of `crafted`: the table is read from tests/golden/ when a file recorded for exactly these inputs (by
    their SHA-256) is there, and computed otherwise."""
    digest = _digest(fr, ref, mu, var)
    if cache is not None and os.path.exists(_case_file(*cache)):
        z = np.load(_case_file(*cache))
        if str(z["digest"]) == digest:
            return {k: z[k] for k in z.files if k != "digest"}
    M, R = mu.shape
    K = keys(M)
    out = {k: np.full(R, np.nan) for k in K}
    out.update({"S_" + k: np.full(R, np.nan) for k in K})
    dec = boxes(fr, ref)
    for j in range(R):
        if np.all(np.isfinite(mu[:, j])) and np.all(np.isfinite(var[:, j])) and np.all(var[:, j] >= 0.0):
            vals, scales = mp_ehvi(fr, ref, mu[:, j], var[:, j], decomposition=dec)
            for k, v, s in zip(K, vals, scales):
                out[k][j], out["S_" + k][j] = v, s
    return out


def write_golden(M, n_front, R, seed):
    """Records the 50-digit table of crafted(M, n_front, R, seed) under tests/golden/ (development use: python -c ...)."""
    fr, ref, mu, var = crafted(M, n_front, R, seed)
    tab = mp_table(fr, ref, mu, var)
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez(_case_file(M, n_front, R, seed), digest=_digest(fr, ref, mu, var), **tab)
    return tab


def shares(got, tab, bound):
    """got = (value, dmu[M, R], dvar[M, R]); -> dict key -> max |got - ref| / (bound max(S, 1e-300)) over the valid columns; the
    others must be NaN in every output."""
    f, pm, pv = got
    M = pm.shape[0]
    K = keys(M)
    mine = dict(zip(K, (f,) + tuple(pm) + tuple(pv)))
    ok = np.isfinite(tab["value"])
    out = {}
    for k in K:
        assert np.all(np.isnan(mine[k][~ok])), (k, "a column with a NaN or negative moment must be NaN")
        assert np.all(np.isfinite(mine[k][ok])), k
        out[k] = float(np.max(np.abs(mine[k][ok] - tab[k][ok]) / (bound * np.maximum(tab["S_" + k][ok], 1e-300)))) if ok.any() else 0.0
    return out


# ---- crafted fronts and moments ------------------------------------------------------------------------------------------------------
def grid_seed(M, n_front, R):
    return 100000 * M + 1000 * n_front + R


def sphere_front(M, n, rng, ties=True):
    """n mutually non-dominated points over [-2, 2]^M: -2 + 4 u, u on the unit sphere's positive orthant (of two points on a sphere
    neither dominates the other).  With M >= 3, n >= 4 and ties: points 0 and 1 share their value in the LAST objective (point 1 is
    point 0 turned in the plane of objectives 0 and 1) and points 2 and 3 share theirs in the FIRST (turned in the plane of objectives
    1 and M - 1)."""
    u = rng.uniform(0.2, 1.0, (n, M))

    def turn(p, a, b):
        q = p.copy()
        c, s = math.cos(0.1), math.sin(0.1)
        q[a], q[b] = c * p[a] - s * p[b], s * p[a] + c * p[b]
        return q

    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if ties and M >= 3 and n >= 4:
        u[1] = turn(u[0], 0, 1)
        u[3] = turn(u[2], 1, M - 1)
    return np.ascontiguousarray((-2.0 + 4.0 * u).T)


def staircase(M, n):
    """A front whose box count is known: a two-objective staircase of n points, every further objective at one shared value --
    n + M - 1 boxes (n + 1 strips below the shared value, one box above it per further objective)."""
    k = np.arange(n, dtype=np.float64)
    fr = np.full((M, n), 0.5)
    fr[0], fr[1] = -1.5 + 3.0 * (k + 0.5) / max(n, 1), 1.5 - 3.0 * (k + 0.25) / max(n, 1)
    return fr


def crafted_moments(fr, ref, R, rng):
    """mu, var [M, R] against a front: every objective's z = (mu - t) / sigma against a level t of its own (one of the front's values
    in that objective or ref's) runs over [-12, 8] in an order of its own, sigma over [1e-3, 10].  With R >= 16, columns 0..2 carry
    sigma^2 = 0 in objective 1 (above, below and on a level), 3..5 in the last objective likewise, 6..8 in ALL objectives (above the
    front, below ref, on levels), column 9 a NaN mean, 10 a NaN variance, 11 a negative variance."""
    M, n = fr.shape
    mu, var = np.empty((M, R)), np.empty((M, R))
    for m in range(M):
        pool = np.concatenate([[ref[m]], fr[m]])
        t = pool[rng.integers(0, pool.size, R)]
        sd = 10.0 ** rng.uniform(-3, 1, R)
        z = rng.permutation(np.linspace(-12.0, 8.0, R)) if R > 1 else np.array([0.7 - m])
        mu[m], var[m] = t + z * sd, sd * sd
    if R >= 16:
        t = np.array([fr[m, n // 2] if n else ref[m] for m in range(M)])
        var[0, 0:3] = 0.0
        mu[0, 0:3] = [t[0] + 0.25, t[0] - 0.25, t[0]]
        var[M - 1, 3:6] = 0.0
        mu[M - 1, 3:6] = [t[M - 1] + 0.25, t[M - 1] - 0.25, t[M - 1]]
        var[:, 6:9] = 0.0
        mu[:, 6] = 2.5
        mu[:, 7] = ref - 0.5
        mu[:, 8] = t
        mu[0, 9] = np.nan
        var[M - 1, 10] = np.nan
        var[0, 11] = -1e-3
    return mu, var


def crafted(M, n_front, R, seed=0):
    """(front[M, n], ref[M], mu[M, R], var[M, R]): sphere_front (with its ties where M >= 3 and n >= 4) above ref = REF4[:M], and
    crafted_moments against it."""
    rng = np.random.default_rng(seed)
    ref = REF4[:M].copy()
    fr = sphere_front(M, n_front, rng)
    mu, var = crafted_moments(fr, ref, R, rng)
    return fr, ref, mu, var


def measure_worst(grid=GRID, write=False):
    """The measurement behind WORST (development use): -> (worst share, its case)."""
    worst, case = 0.0, None
    for M, n, R in grid:
        seed = grid_seed(M, n, R)
        fr, ref, mu, var = crafted(M, n, R, seed)
        tab = write_golden(M, n, R, seed) if write else mp_table(fr, ref, mu, var, cache=(M, n, R, seed))
        sh = shares(ehvi(fr, ref, mu, var), tab, 1.0)
        k = max(sh, key=sh.get)
        print(M, n, R, boxes(fr, ref)[1].shape[1], k, sh[k], flush=True)
        if sh[k] > worst:
            worst, case = sh[k], (M, n, R, k)
    return worst, case
