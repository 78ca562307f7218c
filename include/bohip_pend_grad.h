/*
 * bohip_pend_grad.h -- C ABI of the gradient of the acquisition under pending evaluations of libbohip.so.  A header of
 * its own beside bohip_pend.h: that header keeps its four symbols, bohip.h its 62.  Conventions (Float64 / Int64, blocking calls,
 * status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.PEND_GRAD_SIGNATURES; Julia: julia/BOHipPendGrad.jl.
 *
 * Role: an EXTENSION, as bohip_gp_score_pending is.  With the seed fixed the fantasy-averaged acquisition P(x) is one deterministic
 * function of the candidate; this symbol gives it the gradient an L-BFGS ascent climbs.  In bohip_pend.h's notation, with S1 = max(S, 1),
 * A = W'V_p (N x p) and u(x) = W'W k*(x):
 *     omega_s = (1 / S1) da/dmu(mu_s, s^2; tau_s),   Omega = sum_s omega_s,   w = sum_s omega_s z_s   (p values)
 *     gamma   = (1 / S1) sum_s da/dsigma^2(mu_s, s^2; tau_s),   gamma = 0 where s^2 == 0 exactly (a clamped variance has zero gradient)
 *     t       = L_p^-T (w - 2 gamma b(x))
 *     grad P(x) = sum_n dk(x, X_n)/dx e[n] + sum_i t_i dk(x, Xp_i)/dx,     e[n] = Omega alpha[n] - 2 gamma u[n] - sum_i A[n, i] t_i
 * with bohip_acq_eval's partials and dk(x, y)/dx_k = fx(r) il2_k (x_k - y_k), fx = 2 dk/dr (Matern 1/2: 0 at r = 0, which also covers a
 * candidate on a pending point).  LogEI's score is the max-shifted log-mean-exp of the per-fantasy values v_s, so omega_s = p_s dv_s/dmu
 * and gamma = sum_s p_s dv_s/dsigma^2 with the soft-max weights p_s; a fantasy of weight exactly 0 contributes 0; a score of -Inf has a
 * zero gradient, a NaN score a NaN one.  S = 0 (the Kriging believer): z = 0, so w = 0 and t = -2 gamma L_p^-T b.  Under
 * BOHIP_PEND_RAISE_TAU tau_s depends on the fantasies alone and has no gradient in x.  Sums over the fantasies: lane l of a wave adds
 * s = l, l + 64, ... in ascending order, then one halving tree over the 64 lanes.
 *
 *   bohip_gp_score_pending_grad   Arguments, errors and laziness as bohip_gp_score_pending.  grad [R][d] row-major as bohip_gp_score_grad
 *                                 (d x R column-major), required.  score, mu, var and best are nullable and are
 *                                 bohip_gp_score_pending's bytes (the same kernels on the same route).  With an empty pending set the
 *                                 call IS bohip_gp_score_grad (and bohip_gp_predict for the moments).  The basis [alpha | A] is derived
 *                                 on the first gradient call and kept like the rest of the pending state; a caller that only scores
 *                                 never builds it.  The model, the pending set and bohip_gp_score_pending's bytes are not changed; two
 *                                 identical calls return identical bytes.
 *                                 Stage labels: those of bohip_gp_score_pending, gemm_U, pend_weights, pend_mix, pend_grad_finish.
 * BOHIP_E_ARG: as bohip_gp_score_pending, and a null grad;  BOHIP_E_STATE: no observations.
 */
#ifndef BOHIP_PEND_GRAD_H
#define BOHIP_PEND_GRAD_H
#include "bohip.h"
#include "bohip_pend.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_score_pending_grad(bohip_gp *gp, int acq_id, const double *acq_params, const double *Xs, int64_t R, int64_t S,
                                uint64_t seed, int flags, double *score, double *grad, double *mu, double *var, bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_PEND_GRAD_H */
