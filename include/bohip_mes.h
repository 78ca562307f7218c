/*
 * bohip_mes.h -- C ABI of max-value entropy search over a candidate set of libbohip.so.  A header of its own beside
 * bohip.h: the model's ABI (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls, status codes,
 * bohip_last_error) are those of bohip.h.  ctypes: _lib.MES_SIGNATURES; Julia: julia/BOHipMES.jl.
 *
 * Role: an EXTENSION -- the reference has no information-theoretic acquisition.  Max-value entropy search (Wang & Jegelka, ICML
 * 2017) ranks a candidate by the information its observation gives about the VALUE of the optimum; unlike EI with tau = max y it
 * does not lean on a noisy incumbent (the reference's logNoise / repetitions).
 *
 * 1. The functor (the contract; tests/mes_reference.py is the NumPy twin, operation for operation; contraction off).
 *    c = 0.9189385332046728, sqrt 2 = 1.4142135623730951.  For mu, s2 of a candidate and a max value m:
 *      mu, s2 or m not finite, or s2 < 0            u = NaN, both partials NaN
 *      s2 == 0                                      u = 0, both partials 0
 *      otherwise sigma = sqrt(s2), gamma = (m - mu) / sigma, phi = 0.3989422804014327 exp(-0.5 (gamma gamma)) and
 *      gamma > 0        Phic = 0.5 erfc(gamma / sqrt 2),  lambda = phi / (1 - Phic),  u = (gamma lambda) / 2 - log1p(-Phic)
 *                       (both terms are >= 0: a u of 1e-290 keeps its relative accuracy)
 *      -4 < gamma <= 0  Phi = 0.5 erfc(-gamma / sqrt 2),  lambda = phi / Phi,         u = (gamma lambda) / 2 - log(Phi)
 *      gamma <= -4      t = -gamma; r = 2 / (t + 3 / (t + ...)) and c1 = 1 / (t + r) from csrc/acq_log.h's continued fraction at
 *                       depth 40;  lambda = t + c1,  u = (c + log(t + c1)) - (0.5 t) c1   (the two t^2 / 2 terms of gamma lambda / 2
 *                       and -log Phi cancel analytically and are never formed)
 *      du/dgamma        -((lambda / 2) ((1 + gamma gamma) + gamma lambda)) in the first two cases;
 *                       -((lambda / 2) (r c1)) for gamma <= -4  (1 + gamma^2 + gamma lambda = r c1, no subtraction)
 *      du/dmu = (-du/dgamma) / sigma,    du/ds2 = ((-du/dgamma) gamma) / (2 s2)
 *    MES_j = (sum_{k=0}^{K-1} u(mu_j, s2_j, m_k)) / K: added in ascending k from +0.0, ONE IEEE division by K; the two partials are
 *    summed and divided likewise.  The result depends on (mu_j, s2_j, m) alone, bit for bit, not on R or the candidate's position.
 *    best: bohip_gp_score's record -- first maximum under strict '>' from -Inf, NaN never wins, {-Inf, -1} if nothing can win.
 *
 * 2. Max values, mode BOHIP_MES_GUMBEL (0); any R up to BOHIP_MES_RMAX.
 *    S(y) = sum_j log Phi((y - mu_j) / sigma_j), log Phi(g) = log1p(-0.5 erfc(g / sqrt 2)) for g > 0, log(0.5 erfc(-g / sqrt 2)) for
 *    -4 < g <= 0, (-0.5 (g g) - c) - log(t + c1) for g <= -4.  A candidate with s2 == 0 adds 0 when y >= mu_j and -Inf otherwise; a
 *    candidate that is not finite (or has s2 < 0) takes no part.
 *    lo = max_j (mu_j - 5 sigma_j), hi = max_j (mu_j + 5 sigma_j): S(lo) < log 0.25 (one factor is Phi(-5)) and S(hi) > log 0.75
 *    (S >= -R 2.87e-7 > -0.151 for R <= BOHIP_MES_RMAX), so the bracket needs no expansion.
 *    y_p, p = 0.25, 0.5, 0.75: the root of S(y) = log p in [lo, hi] by 14 passes of 16-section -- 15 probes lo + (hi - lo) i / 16, the
 *    first probe with S >= log p is the new hi, its predecessor the new lo -- and lo + 0.5 (hi - lo) of the final bracket.
 *    b = (y75 - y25) / 1.5725335836855193   (log(log 4) - log(log(4/3)));      a = y50 + b (-0.36651292058166435)   (log(log 2))
 *    m_k = max(a - b log(-log u_k), floor_value),  u_k the first uniform of bohip_thompson_normal(seed, k, 0).
 *    hi == lo (every sigma is 0): y_p = lo, b = 0, m_k = max(lo, floor_value).
 *    quantiles[3] = (y25, y50, y75) and maxvals[K] are bit-identical between two calls of one build.
 *
 * 3. Max values, mode BOHIP_MES_JOINT (1); R within one candidate chunk.
 *    K joint draws, exactly bohip_gp_sample_joint's for the same (Xs, R, S = K, seed, jitter_rel, max_tries); they stay on the
 *    device.  m_k = max(max over the finite F_kj, floor_value), the inner maximum -Inf if no F_kj is finite.  Jitter escalation,
 *    jitter_used / tries_used and BOHIP_E_NOTPD follow bohip_gp_sample_joint.  quantiles are NaN.
 *
 *   bohip_gp_mes      posterior -> max values -> values -> record, all on the device; only the named outputs cross.  One host
 *                     synchronisation per call, plus one per jitter retry.  The model is not changed.  floor_value = -Inf: no floor.
 *   bohip_mes_values  the functor alone on the caller's (mu, var, maxvals), with the partials if dmu AND dvar are given.
 *   bohip_mes_gumbel  the max-value sampler of mode 0 alone on the caller's (mu, var).
 *                     Both take the handle for its device and stream only: a model without observations will do.
 * Errors (sizes before null pointers).  BOHIP_E_ARG: R < 1, K < 1, an unknown mode, a null pointer where one is needed, only one
 * of dmu / dvar, a NaN floor.  BOHIP_E_STATE: bohip_gp_mes on a model without observations.  BOHIP_E_UNSUPPORTED: K above
 * BOHIP_MES_KMAX (the max values live in a workgroup's LDS), R above BOHIP_MES_RMAX (the bracket's guarantee), joint mode beyond
 * one candidate chunk; the message names the limit, and nothing is allocated before the check.
 * Scratch lives on the handle, grows on demand and is freed by bohip_gp_destroy.
 */
#ifndef BOHIP_MES_H
#define BOHIP_MES_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_MES_KMAX 1024
#define BOHIP_MES_RMAX 524288
#define BOHIP_MES_GUMBEL 0
#define BOHIP_MES_JOINT 1

int bohip_gp_mes(bohip_gp *gp, const double *Xs, int64_t R, int64_t K, int mode, uint64_t seed, double floor_value,
                 double jitter_rel, int max_tries /* joint mode only, ignored otherwise */, double *mes /* R */,
                 double *maxvals /* K, nullable */, double *quantiles /* 3, nullable; NaN in joint mode */, double *mu /* R, nullable */,
                 double *var /* R, nullable */, bohip_best *best /* nullable */, double *jitter_used /* nullable */,
                 int *tries_used /* nullable */);
int bohip_mes_values(bohip_gp *gp, const double *mu, const double *var, int64_t R, const double *maxvals, int64_t K,
                     double *mes /* R */, double *dmu, double *dvar /* R each, nullable TOGETHER */, bohip_best *best /* nullable */);
int bohip_mes_gumbel(bohip_gp *gp, const double *mu, const double *var, int64_t R, int64_t K, uint64_t seed, double floor_value,
                     double *quantiles /* 3 */, double *maxvals /* K */);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_MES_H */
