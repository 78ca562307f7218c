/*
 * bohip_nei_grad.h -- C ABI of the gradient of noisy expected improvement of libbohip.so.  A header of its own beside
 * bohip_nei.h: that header keeps its six symbols, bohip.h its 62.  Conventions (Float64 / Int64, blocking calls, status codes,
 * bohip_last_error) are those of bohip.h.  ctypes: _lib.NEI_GRAD_SIGNATURES; Julia: julia/BOHipNEIGrad.jl.
 *
 * Role: an EXTENSION, as bohip_gp_score_nei is.  With the fantasies drawn once (a fixed seed) NEI is one deterministic function of the
 * candidate, which Letham et al. climb with L-BFGS; this symbol gives it the gradient.  In bohip_nei.h's notation, with
 * u(x) = W_d'W_d k* and S1 = max(S, 1):
 *     grad NEI(x) = sum_n dk(x, X_n)/dx e[n],      e[n] = sum_s omega_s alpha_s[n] - 2 c u[n]
 *     omega_s = (1 / S1) da/dmu(m_s, s^2; tau_s),  c = (1 / S1) sum_s da/dsigma^2(m_s, s^2; tau_s),  c = 0 where s^2 == 0 exactly
 * with bohip_acq_eval's partials (a clamped variance has zero gradient, as in bohip_gp_score_grad) and
 * dk*_n/dx_k = fx(r_n) il2_k (x_k - X_nk), fx = 2 dk/dr (Matern 1/2: 0 at r = 0).  LogEI's score is the max-shifted log-mean-exp of
 * the per-fantasy values v_s, so omega_s = p_s dv_s/dmu and c = sum_s p_s dv_s/dsigma^2, p_s = exp(v_s - v_max) / sum_t exp(v_t - v_max),
 * every sum in the order s = 0, 1, ...; a score of -Inf has a zero gradient, a NaN score a NaN one.
 *
 *   bohip_gp_score_nei_grad   Arguments, errors and laziness as bohip_gp_score_nei (the companion, the fantasies and alpha_s are kept;
 *                             a call on an unchanged model refits and rebuilds nothing).  grad [R][d] row-major as bohip_gp_score_grad
 *                             (d x R column-major), required.  score, mu, var and best are nullable and mean what they mean there; the
 *                             companion's pass runs the route that stores V', so they agree with bohip_gp_score_nei's to rounding, not
 *                             bit for bit.  The model is not changed; two identical calls return identical bytes.
 *                             Stage labels: nei_means, nei_weights, nei_mix, nei_grad_finish (and the companion's pass).
 * BOHIP_E_ARG: as bohip_gp_score_nei, and a null grad;  BOHIP_E_STATE: no observations.
 */
#ifndef BOHIP_NEI_GRAD_H
#define BOHIP_NEI_GRAD_H
#include "bohip.h"
#include "bohip_nei.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_score_nei_grad(bohip_gp *gp, int acq_id, const double *acq_params, const double *Xs, int64_t R, int64_t S, uint64_t seed,
                            double jitter_rel, double *score, double *grad, double *mu, double *var, bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_NEI_GRAD_H */
