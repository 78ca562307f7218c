/*
 * bohip_loo_batch.h -- C ABI of the batched leave-one-out objective of libbohip.so.  A header of its own beside
 * bohip.h, bohip_fit.h and bohip_loo.h, none of which changes: the one symbol here evaluates the leave-one-out predictive
 * log-probability of a resident model (bohip_loo.h: total = sum_i logp_i), and its gradient, at H hyper-parameter settings in ONE
 * launch (one workgroup per setting) -- what bohip_gp_mll_grad_batch is to bohip_gp_mll_grad.  Conventions (Float64 / Int64,
 * blocking calls, status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.LOO_BATCH_SIGNATURES; Julia:
 * julia/BOHipLOOBatch.jl.
 *
 * Role: the objective of a multi-start fit with the leave-one-out criterion (Rasmussen & Williams 5.4.2; Bachoc 2013 for the
 * misspecified case), all starts in one device call per step.  bohip_gp_loo_grad stays the single-setting form at any N.
 *
 *   bohip_gp_loo_grad_batch   theta: H rows of P doubles (host), laid out as for bohip_gp_mll_grad_batch
 *                             [logNoise, mean, ll_0 .., logsig]; bohip_gp_mll_batch_dims gives P and the size cap BOHIP_FIT_NMAX.
 *                             total[H] is required.  grad: H rows of P in theta's order (an iso kernel's length entries folded into
 *                             one, the mean slot filled for a MeanZero model too), or NULL: value only, total and logp are then the
 *                             same bytes as a gradient call's.  logp: H rows of N per-point log-probabilities, or NULL.  pivot[H],
 *                             or NULL: 0 = ok, k = the 1-based pivot that was not a finite positive number; a setting with a
 *                             non-finite entry fails as pivot 1.  A failed row has total = -inf, a zero gradient row and a NaN row
 *                             of logp; it is NOT an error of the call and does not touch other rows.
 *                             The arithmetic of a row depends on (model, its theta) only: not on H, not on the row's position, not
 *                             on which other rows fail -- bit for bit.
 *                             The model's own hyper-parameters, factor, alpha and staleness are neither read for the result nor
 *                             changed: the call reads the observations only and never refits.
 *                             Workspace: that of bohip_gp_mll_grad_batch (the same slabs, the same BOHIP_FIT_WS_MAX_MB), plus H x N
 *                             doubles on the handle when logp is asked for.  Freed by bohip_gp_destroy.
 * BOHIP_E_ARG: null handle / theta / total, H < 1;  BOHIP_E_STATE: no observations;  BOHIP_E_UNSUPPORTED: more than
 * BOHIP_FIT_NMAX observations (the text names the limit and bohip_gp_loo_grad).
 */
#ifndef BOHIP_LOO_BATCH_H
#define BOHIP_LOO_BATCH_H
#include "bohip_fit.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_loo_grad_batch(bohip_gp *gp, int64_t H, const double *theta, double *total, double *grad, double *logp, int64_t *pivot);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_LOO_BATCH_H */
