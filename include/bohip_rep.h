/*
 * bohip_rep.h -- C ABI of replicated sites of libbohip.so.  A header of its own beside bohip.h: the model's ABI
 * (bohip.h, 62 symbols) is unchanged; the three symbols here let r evaluations at ONE position enter the model as one row.
 * Conventions (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.REP_SIGNATURES;
 * Julia: julia/BOHipRep.jl.
 *
 * Role: the reference evaluates every proposed point `repetitions` times and appends every evaluation as a column of its own
 * (src/BayesianOptimization.jl:190-196); for a Gaussian likelihood r evaluations at one position are EXACTLY one observation of
 * their mean with noise nu / r, for the posterior and for the marginal likelihood.  A SITE is a position x_i with the mean ybar_i
 * of its r_i >= 1 evaluations, the count r_i and the within-site sum of squares s_i = sum_j (y_ij - ybar_i)^2.  With
 * nu = exp(2 logNoise) + eps + jitter (the diagonal term of the resident build) a handle that holds a site with r_i > 1 is WEIGHTED:
 *     cK_w = K + nu diag(1 / r_i),   L, W, W' of cK_w,   alpha = cK_w^-1 (ybar - beta)
 * and every call that reads the resident L, W, W', alpha (predict, score, score_grad, acquire_max, direct_max, thompson, predict_cov,
 * sample_joint, qei, kg, mes, select_batch, predict_grad, score_con / score_mo members at the C level) answers for the model with
 * every evaluation as its own row, at n sites instead of N_tot = sum r_i rows.
 *   bohip_gp_mll, bohip_gp_mll_grad   on a weighted handle: the log marginal likelihood of ALL evaluations,
 *         mll = [-1/2 (ybar - beta)' alpha - sum log L_ii - n/2 log 2 pi] + C
 *         C   = -1/2 (N_tot - n) log(2 pi nu) - 1/2 sum log r_i - (sum s_i) / (2 nu)
 *     d_lognoise = 2 sigma^2 sum_i G_ii / r_i + 2 sigma^2 (-(N_tot - n) / (2 nu) + (sum s_i) / (2 nu^2)),  G_ii = 1/2 (alpha_i^2 -
 *     (cK_w^-1)_ii), sigma^2 = exp(2 logNoise); the mean and kernel slots are those of bohip_gp_mll_grad computed on cK_w.
 *   bohip_gp_loo          works unchanged (it reads kappa off W' and alpha): it then leaves one SITE out, and predicts the site's mean.
 *   bohip_gp_maxy, bohip_gp_get_xy   speak of the site means; the largest raw evaluation is the caller's to keep (model.maxy does).
 *   The noise of ONE evaluation (the fantasy noise of bohip_gp_select_batch, the nu of bohip_gp_kg) stays nu, as in the expanded model.
 *
 *   bohip_gp_append_sites  p sites: X[p][d], ybar[p], reps[p], ss[p].  BOHIP_E_ARG for reps < 1, for a negative or non-finite ss and
 *                          for ss != 0 where reps = 1 (nothing is stored).  Otherwise it routes like bohip_gp_append: the staged copy,
 *                          the incremental route up to 32 rows (APPEND_PMAX), a refit on growth or when stale; as there, the
 *                          observations are stored when the factorisation fails (BOHIP_E_NOTPD).  With all reps = 1 on an unweighted
 *                          handle it IS bohip_gp_append.  The first site with reps > 1 turns the handle weighted for good; the rows
 *                          it held are sites of one evaluation and its factor stands.  A plain bohip_gp_append on a weighted handle
 *                          adds rows with r = 1.  Sites are never merged: a position given again is a row of its own, as valid as
 *                          a duplicated column is today.
 *   bohip_gp_sites_info    n (sites = rows), N_tot, sum s_i, sum log r_i and whether the handle is weighted; any pointer may be NULL.
 *                          Unweighted: n, n, 0, 0, 0.
 *   bohip_gp_get_reps      r_i of every row (n int64; all 1 on an unweighted handle).
 * An unweighted handle runs the launches it ran before this header existed, with the same arguments, and returns the same bits.
 *
 * Refused on a weighted handle with BOHIP_E_UNSUPPORTED (the message says "replicated sites"), the model untouched: the calls that
 * build cK from the observations in kernels of their own or scale the noise themselves -- bohip_gp_mll_grad_batch, bohip_gp_loo_grad,
 * bohip_gp_loo_grad_batch, bohip_gp_score_ens, bohip_gp_score_ens_grad, bohip_gp_paths_draw -- and every bohip_mgp_* entry point of a
 * device list one of whose replicas was turned weighted.  They refuse; they never answer for a different model.
 */
#ifndef BOHIP_REP_H
#define BOHIP_REP_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_append_sites(bohip_gp *gp, const double *X, const double *ybar, const int64_t *reps, const double *ss, int64_t p);
int bohip_gp_sites_info(const bohip_gp *gp, int64_t *n_sites, int64_t *n_evals, double *ss_total, double *sum_log_reps, int *weighted);
int bohip_gp_get_reps(const bohip_gp *gp, int64_t *reps_out);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_REP_H */
