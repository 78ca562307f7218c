/*
 * bohip_pend.h -- C ABI of pending evaluations of libbohip.so.  A header of its own beside bohip.h: the model's ABI
 * (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of
 * bohip.h.  ctypes: _lib.PEND_SIGNATURES; Julia: julia/BOHipPend.jl.
 *
 * Role: an extension (the reference evaluates one point at a time, src/BayesianOptimization.jl:185-196).  A PENDING point is a
 * position that is out for evaluation and not back yet.  The acquisition that accounts for them is the one of Snoek, Larochelle &
 * Adams 2012, section 3.2: the acquisition averaged over fantasised outcomes at the pending points.  For the resident model
 * (X, y, theta), W = L^-1, nu = exp(2 logNoise) + eps + the jitter of the last refit (cK's diagonal term) and pending Xp (d x p):
 *     V_p = W K(X, Xp),   mu_p = beta + K(X, Xp)' alpha,   Sigma_p = K(Xp, Xp) - V_p' V_p + nu I,   L_p = chol(Sigma_p)
 * and for a candidate x with resident mu(x), sigma^2(x), v(x) = W k*(x):
 *     c(x) = k(x, Xp) - v(x)' V_p,   b(x) = L_p^-1 c(x),   s^2(x) = max(sigma^2(x) - |b(x)|^2, 0).
 * Fantasy s is y_f,s = mu_p + L_p z_s with z_s,i = bohip_thompson_normal(seed, s, i), i = 0 .. p-1 in the order of the pending columns.
 * The posterior conditioned on (Xp, y_f,s) has the variance s^2(x) for every s and the mean mu_s(x) = mu(x) + b(x)' z_s -- only the mean
 * depends on the fantasy, so S fantasies are one contraction, not S refits.  The score is the mean over s = 0 .. S-1, in that order, of
 * a(mu_s(x), s^2(x); params_s).  With BOHIP_PEND_RAISE_TAU EI, PI and LogEI take tau_s = max(tau, max_i y_f,s,i).  LogEI returns the
 * log-mean-exp of the per-fantasy values (max-shifted): the logarithm of the averaged EI.  S = 0 is the Kriging believer: z = 0, the
 * mean stays, the variance shrinks (tau_0 = max(tau, max_i mu_p,i) under the flag).  UCB's beta_t and MI's gamma stay as passed.
 *
 *   bohip_gp_pending_set   replaces the handle's pending set by the p columns of Xp (p = 0 clears it).  Copies Xp; nothing is computed
 *                          until the set is read.  BOHIP_E_ARG: p < 0, p > BOHIP_PEND_PMAX, a non-finite coordinate.
 *                          BOHIP_E_UNSUPPORTED on a handle with replicated sites.
 *   bohip_gp_pending_info  every output is nullable.  Brings the model and the pending state up to date and returns p, Xp, mu_p and
 *                          Sigma_p (p x p, nu included).  BOHIP_E_NOTPD when Sigma_p has a failed pivot (no jitter is added here).
 *   bohip_gp_score_pending the score above for R candidates; score, mu, var (R each) are nullable.  mu is the resident mu(x), var is
 *                          s^2(x), best follows bohip_gp_score's arg-max rule.  acq ids 0 .. 4 and BOHIP_ACQ_LOGEI.  BOHIP_E_ARG:
 *                          BOHIP_ACQ_THOMPSON_DRAW, S < 0, S > BOHIP_PEND_SMAX, unknown flags.  BOHIP_E_STATE: no observations.
 *                          With an empty pending set the call IS bohip_gp_score (and bohip_gp_predict for mu, var).  Any R (chunked
 *                          as bohip_gp_score chunks).  The model is not changed; two identical calls return identical bytes.
 *   bohip_pend_values      the averaging stage on its own, from host arrays: mu, var (= s^2) of R candidates, B (p contiguous values
 *                          b(x) per candidate), Z (S x p, row s = z_s), tau_s (S values, NULL: acq_params' tau for every fantasy).
 *                          1 <= p <= BOHIP_PEND_PMAX, 1 <= S <= BOHIP_PEND_SMAX.
 * Every other entry point ignores the pending set.
 */
#ifndef BOHIP_PEND_H
#define BOHIP_PEND_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_PEND_PMAX 32        /* = the incremental append's row limit: the definition exists on the device as ONE append */
#define BOHIP_PEND_SMAX 1024
#define BOHIP_PEND_RAISE_TAU 1

int bohip_gp_pending_set(bohip_gp *gp, const double *Xp, int64_t p);
int bohip_gp_pending_info(bohip_gp *gp, int64_t *p, double *Xp, double *mu_p, double *cov_p);
int bohip_gp_score_pending(bohip_gp *gp, int acq_id, const double *acq_params, const double *Xs, int64_t R, int64_t S, uint64_t seed,
                           int flags, double *score, double *mu, double *var, bohip_best *best);
int bohip_pend_values(bohip_gp *gp, int acq_id, const double *acq_params, int64_t R, int64_t p, int64_t S, const double *mu,
                      const double *var, const double *B, const double *Z, const double *tau_s, double *score, bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_PEND_H */
