/*
 * bohip_ens.h -- C ABI of the acquisition marginalised over hyper-parameter settings of libbohip.so.  A header of
 * its own beside bohip.h: the model's ABI (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls, status
 * codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.ENS_SIGNATURES; Julia: julia/BOHipEns.jl.
 *
 * Role: an EXTENSION -- the reference fits one MAP setting (src/models/gp.jl:54-77) and scores under it.  The integrated
 * acquisition a(x) = sum_h w_h a(x; theta_h) averages over samples theta_h of the hyper-parameter posterior (Snoek, Larochelle &
 * Adams 2012); bohip_gp_mll_grad_batch (bohip_fit.h) rates such settings, this symbol uses them.
 *
 * P, the row layout of theta and nmax are those of bohip_gp_mll_batch_dims:  [logNoise, mean, ll_0 .. ll_{nk-2}, logsig].
 *   bohip_gp_score_ens   acq_id: any id that bohip_gp_score takes (EI, PI, UCB, MI, MaxMean, LogEI); acq_params as there, shared by
 *                        all settings.  theta: H rows of P doubles (host); weights: H doubles >= 0, or NULL = equal; xs: R candidates
 *                        of d doubles (host).  For every setting the mu_h, sigma^2_h and a_h of bohip_gp_predict / bohip_gp_score of a
 *                        model with those hyper-parameters: noise = exp(2 logNoise) + eps, sigma^2 clamped at 0, the functors of
 *                        bohip_gp_score.  Outputs, each nullable but best: scores[R]; each, mu, var: H x R row-major; pivot[H].
 *                        A setting whose factorisation fails gets pivot[h] = k as in the fit (the 1-based pivot that was not a finite
 *                        positive number; a non-finite entry of the row: 1); its rows of each / mu / var are NaN and it takes no part
 *                        in the average.  scores[j] = sum_h w~_h a_h(x_j), added in ascending h starting from 0.0, w~ the weights
 *                        renormalised over the surviving settings; a setting of weight 0 is left out of the sum.
 *                        best: the arg-max of scores under bohip_gp_score's rule -- first maximum, NaN never wins, {-Inf, -1} if
 *                        nothing can win.
 *                        What is computed for (theta_h, x_j) depends on (model, theta_h, x_j) only: not on H, the row's position or
 *                        other rows failing, not on R or the candidate's position, not on how many launches the call took -- bit
 *                        for bit.
 *                        The model's own hyper-parameters, factor, alpha and staleness are neither read for the result nor changed.
 *                        Workspace: the fit's slabs on the handle (two (N + 8)^2-sized slabs per setting, grown on demand up to 1 GiB,
 *                        BOHIP_FIT_WS_MAX_MB read at every call lowers it); more settings than fit run in consecutive launches with
 *                        the same results.  R of any size is chunked inside the call.
 * BOHIP_E_ARG: null handle / theta / xs / best, H < 1, R < 1, an unknown or Thompson acq_id, a negative or non-finite weight, weights
 * summing to 0;  BOHIP_E_STATE: no observations;  BOHIP_E_UNSUPPORTED: more than BOHIP_FIT_NMAX observations (the text names the
 * limit);  BOHIP_E_NOTPD: no setting survived (pivot and the NaN rows are still delivered).
 */
#ifndef BOHIP_ENS_H
#define BOHIP_ENS_H
#include "bohip.h"
#include "bohip_fit.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_score_ens(bohip_gp *gp, int acq_id, const double *acq_params, int64_t H, const double *theta, const double *weights,
                       const double *xs, int64_t R, double *scores, double *each, double *mu, double *var, int64_t *pivot,
                       bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_ENS_H */
