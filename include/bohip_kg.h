/*
 * bohip_kg.h -- C ABI of the knowledge gradient over a candidate set of libbohip.so.  A header of its own beside
 * bohip.h: the model's ABI (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls, status codes,
 * bohip_last_error) are those of bohip.h.  ctypes: _lib.KG_SIGNATURES; Julia: julia/BOHipKG.jl.
 *
 * Role: an EXTENSION -- the reference has no such acquisition.  Every acquisition of the reference is a one-point functor of
 * (mu, sigma^2) and ranks a candidate by what its own value might be; the knowledge gradient ranks it by what OBSERVING it would
 * teach the model about the optimum (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011), the one-step look-ahead for a
 * noisy objective (the reference's logNoise / repetitions).
 *
 * Definition (the contract).  Candidates x_0 .. x_{R-1} of one chunk; a_j = mu_j their latent posterior mean, Sigma their
 * posterior covariance (bohip_gp_predict_cov's), nu = exp(2 logNoise) + eps + jitter_last what the model has on the diagonal of
 * cK (the noise of bohip_gp_select_batch's fantasies).  For an evaluation point e < E <= R the lines are
 *     b_j = Sigma_je / sqrt(Sigma_ee + nu)              one IEEE addition, square root and division
 *     KG(e) = E_Z[max_j (a_j + b_j Z)] - max_j a_j,     Z ~ N(0, 1),    KG(e) >= 0
 * computed EXACTLY (no quadrature, no Monte Carlo: the kinks of the envelope defeat Gauss-Hermite) by a march along the upper
 * envelope of the lines.  Lines whose a or b is not finite take no part; KG = 0, nseg = 0 if none is left.
 *     c <- the line of smallest b (ties: largest a, then smallest index);  kg <- +0.0;  nseg <- 0
 *     loop:  U = { i : b_i > b_c };  if U is empty, stop
 *            z_i = (a_c - a_i) / (b_i - b_c)   for i in U        one IEEE subtraction each, one IEEE division; a NaN z_i (the
 *                                                                 subtractions overflowed) takes no part in this step
 *            t   = argmin_i z_i                                   ties: largest b, then largest a, then smallest index
 *            kg += T(b_t - b_c, -|z_t|);   nseg += 1;   c <- t
 * T(db, x) = db h(x), h(x) = phi(x) + x Phi(x), x <= 0, in csrc/acq_log.h's two forms, contraction off:
 *     x > -4    phi = 0.3989422804014327 exp(-0.5 (x x)),  Phi = 0.5 erfc(-x / 1.4142135623730951),  T = db (phi + x Phi)
 *     x <= -4   t = -x, Mills' ratio by its continued fraction at depth 40: r = 2 / (t + 3 / (t + ...)), c1 = 1 / (t + r),
 *               h = phi(x) c1 / (t + c1) with no subtraction.  The exponential is taken in two halves, e = exp(-0.25 (x x)),
 *               T = (db e) ((0.3989422804014327 e) (c1 / (t + c1))), so the term of a steep line in the deep tail does not
 *               underflow before its product does.
 * Every term is >= 0, so nothing cancels against max a (this is Frazier's sum (b_{i+1} - b_i) f(-|c_i|)), and a KG of 1e-30 keeps
 * its relative accuracy.  The arg-min is exact and the terms are added in march order: the sequence of lines, nseg and the order
 * of the additions depend on (a, b) only, not on launch geometry.  tests/kg_reference.py is the NumPy twin, operation for
 * operation (kg_march), next to an independent sorted-hull form (kg_hull).
 * KG(e) = 0 with nseg = 0 also where Sigma_ee + nu <= 0 or is not finite, and for R = 1.
 * best: the arg-max over e < E under bohip_gp_score's rule -- first maximum under strict '>' from -Inf, NaN never wins,
 * {-Inf, -1} if nothing can win.
 *
 *   bohip_gp_kg      the posterior of the R candidates (the stages of bohip_gp_predict_cov: K*', V', V'V, Sigma, mu -- all of it
 *                    stays on the device), then the march for the first E columns of Xs, one workgroup per evaluation point; the
 *                    maximum runs over all R.  kg[E]; nseg[E], mu[R], best: nullable.  Only these cross to the host.  One host
 *                    synchronisation per call.  The model is not changed.
 *   bohip_kg_lines   the march alone on the caller's lines: a[R], B E x R row-major (row e: the slopes of evaluation point e),
 *                    uploaded into scratch on the handle.  The handle supplies the device and the stream only: a model without
 *                    observations will do.
 * BOHIP_E_ARG: null handle or pointers (gp, Xs / a / B, kg); R < 1, E < 1, E > R.  BOHIP_E_STATE: bohip_gp_kg on a model without
 * observations.  BOHIP_E_UNSUPPORTED: R above BOHIP_KG_RMAX (a point's a and b live in the workgroup's LDS: 16 R bytes of the
 * 160 KiB); R beyond one candidate chunk (bohip_gp_predict_cov's limit; bohip_gp_kg only).  Both messages name the limit.
 * Scratch lives on the handle, grows on demand and is freed by bohip_gp_destroy.
 */
#ifndef BOHIP_KG_H
#define BOHIP_KG_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_KG_RMAX 8192

int bohip_gp_kg(bohip_gp *gp, const double *Xs, int64_t R, int64_t E, double *kg /* E */, int32_t *nseg /* E, nullable */,
                double *mu /* R, nullable */, bohip_best *best /* nullable */);
int bohip_kg_lines(bohip_gp *gp, const double *a /* R */, const double *B /* E x R row-major */, int64_t R, int64_t E,
                   double *kg /* E */, int32_t *nseg /* E, nullable */);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_KG_H */
