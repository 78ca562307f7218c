/*
 * bohip_loo.h -- C ABI of leave-one-out cross-validation of libbohip.so.  A header of its own beside bohip.h: the
 * model's ABI (bohip.h, 62 symbols) is unchanged; the two symbols here give the leave-one-out predictions of a resident model at
 * its observations, their predictive log-probability, and the gradient of that sum with respect to the hyper-parameters.
 * Conventions (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.LOO_SIGNATURES;
 * Julia: julia/BOHipLOO.jl.
 *
 * Role: GaussianProcesses.jl predict_LOO, logp_LOO and dlogpdtheta_LOO (Rasmussen & Williams 5.4.2) -- the diagnostic of Jones,
 * Schonlau & Welch 1998 and an alternative objective of the fit beside the marginal likelihood.  With cK = K + (exp(2 logNoise) +
 * eps) I as in the resident build, alpha = cK^-1 (y - beta) and kappa = diag(cK^-1), the prediction of the NOISY observation y_i
 * from all the others is
 *     mu_-i = y_i - alpha_i / kappa_i,   var_-i = 1 / kappa_i,   logp_i = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi
 * and total = sum_i logp_i.  kappa is read off the resident W' = L^-T in one pass; no cK^-1 is formed for the values and nothing
 * is refitted per point.
 *   bohip_gp_loo        mu, var, logp: n doubles each (host), any of them NULL; total is required.  The model at its current
 *                       hyper-parameters, any n; a stale model is refitted first.  mu is in the sign the model stores y.
 *   bohip_gp_loo_grad   total and its gradient in the slots of bohip_gp_mll_grad: d_lognoise, d_mean (filled for a MeanZero model
 *                       too) and d_kern = [d ll_0 .., d logsig], an iso kernel's length entries folded into one.  total is bit for
 *                       bit bohip_gp_loo's.  Cost: the cK^-1 of bohip_gp_mll_grad plus one full N x N x N product.
 *                       Workspace: one more matrix of the model's size on the handle, made on first use, freed by bohip_gp_destroy.
 * Neither call changes the model, its factor or alpha.  No observations: total = 0, a zero gradient, the per-point arrays untouched.
 * BOHIP_E_ARG: null handle / total / gradient slot.  A factorisation that fails reports as from bohip_gp_mll_grad (BOHIP_E_NOTPD).
 */
#ifndef BOHIP_LOO_H
#define BOHIP_LOO_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_loo(bohip_gp *gp, double *mu, double *var, double *logp, double *total);
int bohip_gp_loo_grad(bohip_gp *gp, double *total, double *d_lognoise, double *d_mean, double *d_kern);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_LOO_H */
