/*
 * bohip_nei.h -- C ABI of noisy expected improvement of libbohip.so.  A header of its own beside bohip.h: the model's ABI
 * (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of
 * bohip.h and bohip_pend.h.  ctypes: _lib.NEI_SIGNATURES; Julia: julia/BOHipNEI.jl.
 *
 * Role: an extension.  Every improvement-based acquisition of bohip.h takes tau = maxy, the largest raw observation; with noisy
 * evaluations that is the luckiest noise draw, not the best function value.  Noisy EI (Letham, Karrer, Ottoni & Bakshy 2019, eq. 6)
 * averages the acquisition over posterior draws of the NOISE-FREE function values at the observed sites; every draw supplies its own
 * incumbent and its own noise-free conditional model.
 *
 * Definition.  Resident model: X, y, beta, kernel k, A = K + D = L L', W = L^-1, alpha; D = diag(nu_i), nu_i the noise term cK's
 * diagonal really carries for row i: nu on an ordinary row, nu / r_i on a weighted site (bohip_rep.h), nu = exp(2 logNoise) + eps + the
 * jitter of the last refit, exactly as bohip_pend.h defines nu.  delta = jitter_rel k(x, x); K_d = K + delta I = L_d L_d', W_d = L_d^-1:
 * the noise-free model of the same sites (the COMPANION).  Fantasy s = 0 .. S-1 (Matheron's rule):
 *     z_s,i = bohip_thompson_normal(seed, 2 s, i),   e_s,i = bohip_thompson_normal(seed, 2 s + 1, i),   g_s = L_d z_s,
 *     r_s = (y - beta) - g_s - sqrt(nu_i) e_s,i,     f_s = beta + g_s + r_s - D A^-1 r_s,               tau_s = max_i f_s,i
 * with A^-1 r_s = W'(W r_s) from the resident factors.  For a candidate x with k* = k(X, x):
 *     alpha_s = K_d^-1 (f_s - beta),   m_s(x) = beta + k*' alpha_s,   s^2(x) = max(k(x, x) - |W_d k*|^2, 0)
 *     NEI(x) = (1 / S) sum_s a(m_s(x), s^2(x); tau_s),  summed in the order s = 0, 1, ...,  a in {EI, PI, LogEI}.
 * LogEI returns the max-shifted log-mean-exp of the per-fantasy values, as bohip_gp_score_pending does.  S = 0 is the plug-in form:
 * z = e = 0, so f_0 = y - D alpha, the posterior mean at the sites, tau_0 = max f_0; it is deterministic.  The device evaluates
 * alpha_s as W_d'(z_s + W_d h_s), h_s = r_s - D A^-1 r_s (W_d g_s = z_s exactly), which leaves out the worst-conditioned product.
 * The delta in force: the companion's diagonal carries exp(2 log sqrt(delta - eps)) + eps (delta itself to a relative 1e-16; eps when
 * delta <= 2 eps); a failed pivot in K_d retries with delta x 10 up to three times, and the delta of the successful try is the one
 * the definition uses (BOHIP_NEI_INFO_DELTA, BOHIP_NEI_INFO_JITTER_STEPS).
 *
 * What is kept.  The companion is a second factor state for the same X under the same kernel parameters, built by the code that
 * builds the model's (the same refit plan, the same incremental append for up to 32 new rows).  It is created at the first call of
 * this header, never before; it depends on X, the kernel parameters and jitter_rel.  The fantasies and alpha_s depend additionally on
 * y, beta, D, S and seed.  A second call on an unchanged model refits nothing and rebuilds nothing; one appended observation costs one
 * incremental companion append and one fantasy rebuild.
 *
 *   bohip_gp_nei_prepare    brings the model, the companion, the fantasies and alpha_s up to date (optional: the calls below do it lazily)
 *   bohip_gp_nei_fantasies  the same, and returns F (S1 x N, row s = f_s; S1 = max(S, 1)) and tau (S1); both nullable
 *   bohip_gp_score_nei      the score above for R candidates; score, mu (the mean over s of m_s), var (s^2) are nullable, R each.  best
 *                           follows bohip_gp_score's arg-max rule.  Any R (chunked as bohip_gp_score chunks).  The model is not changed;
 *                           two identical calls return identical bytes.  acq_params' tau is IGNORED (tau_s is the fantasy's own);
 *                           acq_params may be null.  BOHIP_E_ARG: an acquisition without a tau (UCB, MI, MaxMean, THOMPSON_DRAW).
 *   bohip_nei_values        the averaging stage on its own, from host arrays: mu_s (R x S, row r = candidate r), var (R), tau_s (S),
 *                           1 <= S <= BOHIP_NEI_SMAX; mu_mean (the mean over s) is nullable
 *   bohip_gp_nei_info       *value = the quantity `what` (BOHIP_NEI_INFO_*)
 *   bohip_gp_nei_release    frees the companion and the fantasies (bohip_gp_destroy does too); the next call builds them again
 * BOHIP_E_STATE with no observations; BOHIP_E_ARG for jitter_rel <= 0 or non-finite, S < 0, S > BOHIP_NEI_SMAX.
 * Every other entry point ignores all of this.
 */
#ifndef BOHIP_NEI_H
#define BOHIP_NEI_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_NEI_SMAX 1024

#define BOHIP_NEI_INFO_REFITS 0          /* refits of the companion since it was created */
#define BOHIP_NEI_INFO_APPENDS 1         /* incremental appends of the companion */
#define BOHIP_NEI_INFO_REBUILDS 2        /* fantasy rebuilds */
#define BOHIP_NEI_INFO_JITTER_STEPS 3    /* delta x 10 steps the companion's factorisation needed (0 .. 3) */
#define BOHIP_NEI_INFO_BYTES 4           /* device bytes held by the companion's factors and the fantasies */
#define BOHIP_NEI_INFO_DELTA 5           /* the delta in force */

int bohip_gp_nei_prepare(bohip_gp *gp, double jitter_rel, int64_t S, uint64_t seed);
int bohip_gp_nei_fantasies(bohip_gp *gp, double jitter_rel, int64_t S, uint64_t seed, double *F, double *tau);
int bohip_gp_score_nei(bohip_gp *gp, int acq_id, const double *acq_params, const double *Xs, int64_t R, int64_t S, uint64_t seed,
                       double jitter_rel, double *score, double *mu, double *var, bohip_best *best);
int bohip_nei_values(bohip_gp *gp, int acq_id, int64_t R, int64_t S, const double *mu_s, const double *var, const double *tau_s,
                     double *score, double *mu_mean, bohip_best *best);
int bohip_gp_nei_info(const bohip_gp *gp, int what, double *value);
int bohip_gp_nei_release(bohip_gp *gp);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_NEI_H */
