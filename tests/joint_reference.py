"""NumPy model of bohip_gp_sample_joint (joint posterior draws over a candidate set), a helper of the joint-draw tests, not a
test module.

    Sigma = K** - V'V,  C C' = Sigma + jitter I (LAPACK),  f_s = mu + C z_s,  z_sj = thompson_normal(seed, s, j)
    jitter: 0 first; a failed factorisation is repeated with max(10 jitter, jitter_rel max(max diag Sigma, tiny)), max_tries times

The generator is the NumPy twin of bohip_thompson_normal (splitmix64 keyed on (seed, s, j) + Box-Muller), the one
tests/test_full_size_gpu.py checks against the library's host export.
"""
import math

import numpy as np

EPS = np.finfo(np.float64).eps


def np_thompson_normal(seed, s, j):
    """z(seed, s, j) for a scalar s and an int64 array j."""
    M = np.uint64

    def sm(x):
        x = x + M(0x9E3779B97F4A7C15)
        x = (x ^ (x >> M(30))) * M(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> M(27))) * M(0x94D049BB133111EB)
        return x ^ (x >> M(31))

    j = np.asarray(j, dtype=np.int64)
    with np.errstate(over="ignore"):
        key = np.full(j.shape, s, dtype=np.uint64) * M(0xD1B54A32D192ED03) + j.astype(np.uint64)
        h = sm(np.full(j.shape, seed, dtype=np.uint64) ^ sm(key))
        h2 = sm(h)
    u1 = ((h >> M(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)
    u2 = (h2 >> M(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def normals(seed, S, R):
    """Z[s, j] = z(seed, s, j), S x R."""
    j = np.arange(R, dtype=np.int64)
    return np.stack([np_thompson_normal(seed, s, j) for s in range(S)]) if S > 0 else np.empty((0, R))


def factor_with_jitter(Sigma, jitter_rel=1e-12, max_tries=40):
    """(C, jitter, tries) under the library's escalation rule; numpy.linalg.LinAlgError when max_tries retries do not suffice."""
    R = Sigma.shape[0]
    scale = max(float(np.max(np.diag(Sigma))), np.finfo(float).tiny)
    jitter, tries = 0.0, 0
    while True:
        try:
            return np.linalg.cholesky(Sigma + jitter * np.eye(R)), jitter, tries
        except np.linalg.LinAlgError:
            nxt = max(10.0 * jitter, jitter_rel * scale)
            if tries >= max_tries or not nxt > jitter:
                raise
            jitter, tries = nxt, tries + 1


def first_argmax_rows(F):
    """(values, indices) of the first maximum of every row under strict '>' from -Inf; NaN never wins; -1 when nothing wins."""
    F = np.asarray(F, dtype=np.float64)
    G = np.where(np.isnan(F), -math.inf, F)
    idx = np.argmax(G, axis=1).astype(np.int64)
    val = G[np.arange(F.shape[0]), idx]
    idx = np.where(val > -math.inf, idx, -1)
    return np.where(idx >= 0, val, -math.inf), idx


def joint_draws(mu, Sigma, seed, S, jitter_rel=1e-12, max_tries=40):
    """(samples S x R, best values, best indices, C, jitter, tries)."""
    C, jitter, tries = factor_with_jitter(Sigma, jitter_rel, max_tries)
    F = mu[None, :] + normals(seed, S, len(mu)) @ C.T
    bv, bi = first_argmax_rows(F)
    return F, bv, bi, C, jitter, tries


def distinct_picks(F):
    """Draw s takes its best candidate not taken by draws 0..s-1 (ties -> smallest index); -1 when none is left."""
    F = np.asarray(F, dtype=np.float64)
    taken, out = set(), []
    for s in range(F.shape[0]):
        best, idx = -math.inf, -1
        for j in range(F.shape[1]):
            if j not in taken and F[s, j] > best:
                best, idx = F[s, j], j
        out.append(idx)
        if idx >= 0:
            taken.add(idx)
    return np.array(out, dtype=np.int64)


def draw_identity_bound(mu, C, Z):
    """2 (R + 2) eps (|mu_j| + sum_k |C_jk| |z_sk|): a length-R dot product in any summation order plus one addition, doubled
    because the NumPy evaluation it is compared with carries the same error."""
    R = len(mu)
    return 2.0 * (R + 2) * EPS * (np.abs(mu)[None, :] + np.abs(Z) @ np.abs(C).T)
