"""NumPy twin of the batched leave-one-out objective (include/bohip_loo_batch.h).  No device.  A helper, not a test
module.

tests/loo_reference.py states WHAT is computed (cK^-1 from a library solve, G as a full matrix).  This file restates HOW the
one-workgroup kernel computes it, stage by stage, so that the kernel's own choices can be wrong here first:

    pad      M = N rounded up to 16; rows / columns N .. M - 1 of cK are identity, the residual is 0 there
    chol     L, z = L^-1 r (the augmented row), W = L^-1, alpha = W' z, and cK^-1 = W' W kept in its LOWER triangle only -- every
             later read of cK^-1(i, j) goes to (max(i, j), min(i, j)); the strict upper triangle is filled with NaN
    finish   kappa_i = cK^-1_ii, q = alpha / kappa, c = 1/2 (1 / kappa + q^2), logp, total -- rows >= N masked by index (q = c = 0,
             no part in the total); mask=False leaves the mask out, which is the bug the padding invites
    b        b_i = sum_{j < i} cK^-1[i][j] q_j + sum_{j >= i} cK^-1[j][i] q_j
    product  Mm = cK^-1 diag(c) cK^-1 built panel by panel: for each block K of 16 columns, P[i][k] = cK^-1(i, 16 K + k)
             sqrt(c_{16 K + k}), Mm (lower) += P P'
    grad     one walk of the lower triangle with the weight G_ii = alpha_i b_i - Mm_ii, G_ij = (b_i alpha_j + alpha_i b_j) - 2 Mm_ij
             (an off-diagonal entry counts twice), slots [2 e^{2 logNoise} tr G, sum b, ll..., logsig], iso lengths folded

Every array is of `dtype`: float64 for the twin proper, np.longdouble for the extended-precision yardstick of the stress setting.
"""
import numpy as np

from matern_reference import family, is_iso

NB = 16
NOISE_EPS = 2.220446049250313e-16


def _cholesky(A):
    """Lower factor, column by column, in A's dtype (np.linalg has no longdouble)."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        dj = A[j, j] - L[j, :j] @ L[j, :j]
        if not (dj > 0 and np.isfinite(dj)):
            raise np.linalg.LinAlgError(f"pivot {j + 1}")
        L[j, j] = np.sqrt(dj)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _lower_inverse(L):
    n = L.shape[0]
    W = np.zeros_like(L)
    for i in range(n):
        W[i, i] = 1 / L[i, i]
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
    return W


def _k_and_fac(fam, r, s2f, dt):
    """(k, fac) with fac = -2 dk/dr, the factor of the length-scale slots (Matern 1/2: 0 at r = 0)."""
    rho = np.sqrt(r)
    if fam == "SE":
        k = s2f * np.exp(-r / 2)
        return k, k
    if fam == "M12":
        k = s2f * np.exp(-rho)
        safe = np.where(rho > 0, rho, dt(1))
        return k, np.where(rho > 0, k / safe, dt(0))
    if fam == "M32":
        s = np.sqrt(dt(3)) * rho
        return s2f * (1 + s) * np.exp(-s), 3 * s2f * np.exp(-s)
    s = np.sqrt(dt(5)) * rho
    return s2f * (1 + s + dt(5) / 3 * r) * np.exp(-s), dt(5) / 3 * s2f * (1 + s) * np.exp(-s)


def twin(kern, X, y, t, mask=True, dtype=np.float64):
    """(total, grad[P], logp[N]) at t = [logNoise, mean, ll..., lsigma], computed the kernel's way."""
    dt = dtype
    X, y, t = np.asarray(X, dt), np.asarray(y, dt), np.asarray(t, dt)
    N, d = X.shape
    M = (N + NB - 1) // NB * NB
    fam, iso = family(kern), is_iso(kern)
    nl = 1 if iso else d
    assert t.size == 3 + nl
    noise_var, beta, s2f = np.exp(2 * t[0]), t[1], np.exp(2 * t[2 + nl])
    il2 = np.exp(-2 * (np.full(d, t[2], dt) if iso else t[2:2 + d]))
    D2 = (X[:, None, :] - X[None, :, :]) ** 2 * il2
    r = D2.sum(axis=2)
    K, fac = _k_and_fac(fam, r, s2f, dt)
    # ---- pad, factor, invert ---------------------------------------------------------------------------------------------------
    cK = np.eye(M, dtype=dt)
    cK[:N, :N] = K + (noise_var + dt(NOISE_EPS)) * np.eye(N, dtype=dt)
    res = np.zeros(M, dt)
    res[:N] = y - beta
    L = _cholesky(cK)
    W = _lower_inverse(L)
    alpha = W.T @ (W @ res)
    S = np.tril(W.T @ W)
    S[np.triu_indices(M, 1)] = np.nan                             # never read as a number

    def kinv(i, j):
        return S[np.maximum(i, j), np.minimum(i, j)]

    # ---- finish ------------------------------------------------------------------------------------------------------------------
    rows = np.arange(M)
    live = rows < N if mask else np.ones(M, bool)
    kappa = S[rows, rows]
    q = np.where(live, alpha / kappa, dt(0))
    c = np.where(live, (1 / kappa + q * q) / 2, dt(0))
    logp = np.log(kappa) / 2 - alpha * q / 2 - np.log(2 * dt(np.pi)) / 2
    total = logp[live].sum()
    # ---- b ---------------------------------------------------------------------------------------------------------------------
    b = np.zeros(M, dt)
    for i in np.flatnonzero(live):
        b[i] = S[i, :i] @ q[:i] + S[i:, i] @ q[i:]
    # ---- Mm, panel by panel ----------------------------------------------------------------------------------------------------
    sc = np.sqrt(c)
    Mm = np.zeros((M, M), dt)
    for k0 in range(0, M, NB):
        cols = np.arange(k0, k0 + NB)
        P = kinv(rows[:, None], cols[None, :]) * sc[cols][None, :]
        P = np.where(live[:, None] & live[cols][None, :], P, dt(0))
        Mm += np.tril(P @ P.T)
    # ---- gradient: the lower triangle once ---------------------------------------------------------------------------------------
    a, bb = alpha[:N], b[:N]
    G = np.outer(bb, a) + np.outer(a, bb) - 2 * Mm[:N, :N]
    G[np.diag_indices(N)] = a * bb - np.diag(Mm)[:N]
    G = np.tril(G)
    dll = np.einsum("ij,ijk->k", G * fac, D2)
    g = np.concatenate([[np.trace(G) * 2 * noise_var, bb.sum()], [dll.sum()] if iso else dll, [np.sum(G * 2 * K)]]).astype(dt)
    return total, g, logp[:N]
