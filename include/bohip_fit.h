/*
 * bohip_fit.h -- C ABI of the batched marginal likelihood of libbohip.so.  A header of its own beside bohip.h: the
 * model's ABI (bohip.h, 62 symbols) is unchanged; the two symbols here evaluate the log marginal likelihood of a resident model,
 * and its gradient, at H hyper-parameter settings in ONE launch (one workgroup per setting).  Conventions (Float64 / Int64,
 * blocking calls, status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.FIT_SIGNATURES; Julia: julia/BOHipFit.jl.
 *
 * Role: the objective of optimizemodel! (reference src/models/gp.jl:54-77) at many points at once -- restarts of the MAP fit,
 * grids, slice sampling, hyper-parameter marginalisation.  bohip_gp_mll_grad stays the single-setting form at any N.
 *
 * A row of theta has P = 2 + nk entries, nk = d + 1 (ARD kernels) or 2 (iso kernels):
 *     [logNoise, mean, ll_0 .. ll_{nk-2}, logsig]       = GP.get_params order with everything on (src/models/gp.jl:55-58, :74)
 * The noise variance is exp(2 logNoise) + eps, as in the resident build; a MeanZero model passes mean = 0 (its gradient slot is
 * still filled, as by bohip_gp_mll_grad).
 *   bohip_gp_mll_batch_dims   P of this model and nmax = BOHIP_FIT_NMAX, the largest model the batched form takes.
 *   bohip_gp_mll_grad_batch   theta: H rows of P doubles (host).  mll[H]; grad: H rows of P in the same order, or NULL (value
 *                             only: the inverse is not formed); pivot[H], or NULL: 0 = ok, k = the 1-based pivot that was not a
 *                             finite positive number -- then mll = -inf and the gradient row is 0.  A setting with a non-finite
 *                             entry fails as pivot 1.  A failed row is NOT an error of the call and does not touch other rows.
 *                             The arithmetic of a row depends on (model, its theta) only: not on H, not on the row's position, not
 *                             on which other rows fail -- bit for bit.
 *                             The model's own hyper-parameters, factor, alpha and staleness are neither read for the result nor
 *                             changed: the call reads the observations only (rows that a failed append left on the host are uploaded
 *                             first) and never refits.
 *                             Workspace: two (N + 8)^2-sized slabs per setting on the handle, grown on demand up to 1 GiB
 *                             (BOHIP_FIT_WS_MAX_MB in the environment, read at every call, lowers it); a larger H runs in consecutive
 *                             launches inside the call, with the same results.  Freed by bohip_gp_destroy.
 * BOHIP_E_ARG: null handle / theta / mll, H < 1;  BOHIP_E_STATE: no observations;  BOHIP_E_UNSUPPORTED: more than
 * BOHIP_FIT_NMAX observations (the text names the limit).
 */
#ifndef BOHIP_FIT_H
#define BOHIP_FIT_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_FIT_NMAX 512
int bohip_gp_mll_batch_dims(bohip_gp *gp, int64_t *P, int64_t *nmax);
int bohip_gp_mll_grad_batch(bohip_gp *gp, int64_t H, const double *theta, double *mll, double *grad, int64_t *pivot);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_FIT_H */
