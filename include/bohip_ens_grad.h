/*
 * bohip_ens_grad.h -- C ABI of the gradient of the acquisition marginalised over hyper-parameter settings of libbohip.so
 * (DESIGN.md 6n).  A header of its own beside bohip_ens.h: that header keeps its one symbol, bohip.h its 62.  Conventions (Float64 /
 * Int64, blocking calls, status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.ENS_GRAD_SIGNATURES; Julia:
 * julia/BOHipEnsGrad.jl.
 *
 * Role: an EXTENSION, as bohip_gp_score_ens is (the integrated acquisition of Snoek, Larochelle & Adams 2012): the reference climbs
 * its acquisition with :LD_LBFGS on a ForwardDiff gradient (src/acquisition.jl:11-17); this symbol gives the average the same.
 *
 *   bohip_gp_score_ens_grad   Arguments, checks, status codes, chunking over settings (BOHIP_FIT_WS_MAX_MB) and over candidates as
 *                        bohip_gp_score_ens.  scores, each, mu, var, pivot and best are THAT symbol's for the same inputs, bit for bit.
 *                        grad [R][d] row-major as bohip_gp_score_grad (required):  grad[j][k] = sum_h w~_h g_h[j][k], added in ascending
 *                        h from 0.0, a setting of weight 0 left out;  each_grad [H][R][d] (nullable): the g_h,
 *                            g_h = da/dmu grad mu_h + (sigma^2_h > 0 ? da/dsigma^2 grad sigma^2_h : 0)
 *                        with bohip_acq_eval's partials -- a clamped variance has zero gradient, as in bohip_gp_score_grad -- and
 *                            grad mu = sum_j alpha_j dk*_j/dx,   grad sigma^2 = -2 sum_j (cK^-1 k*)_j dk*_j/dx,
 *                            dk*_j/dx_k = fx(r_j) il2_k (x_k - X_jk),  fx = 2 dk/dr  (Matern 1/2: 0 at r = 0).
 *                        A failed setting has NaN rows in each_grad and takes no part in the average.
 *                        What is computed for (theta_h, x_j) depends on (model, theta_h, x_j) only, bit for bit, as there: every sum
 *                        over the observations runs in one fixed order.
 *                        Factor reuse: when all settings fit the workspace at once, the factors and alpha that a call leaves on the
 *                        handle serve the next call of THIS symbol with byte-identical theta and unchanged observations (an ascent's
 *                        20-60 calls factor once).  bohip_gp_mll_grad_batch, bohip_gp_score_ens and any change of the observations end
 *                        that.  Results are the same either way; bohip_gp_get_timing shows no "ens_factor" / "ens_alpha" on a reuse.
 *                        Stage labels: ens_factor, ens_alpha, ens_grad, ens_reduce.
 * BOHIP_E_ARG: as bohip_gp_score_ens, and a null grad;  BOHIP_E_STATE: no observations;  BOHIP_E_UNSUPPORTED: more than
 * BOHIP_FIT_NMAX observations;  BOHIP_E_NOTPD: no setting survived (pivot and the NaN rows are still delivered, grad is NaN).
 */
#ifndef BOHIP_ENS_GRAD_H
#define BOHIP_ENS_GRAD_H
#include "bohip.h"
#include "bohip_fit.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_score_ens_grad(bohip_gp *gp, int acq_id, const double *acq_params, int64_t H, const double *theta,
                            const double *weights, const double *xs, int64_t R, double *scores, double *grad, double *each,
                            double *each_grad, double *mu, double *var, int64_t *pivot, bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_ENS_GRAD_H */
