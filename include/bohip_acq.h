/*
 * bohip_acq.h -- C ABI of the acquisition functors of libbohip.so on their own, and the id of LogEI.  A header of
 * its own beside bohip.h: the model's ABI (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls,
 * status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.ACQ_SIGNATURES; Julia: julia/BOHipAcq.jl.
 *
 * BOHIP_ACQ_LOGEI (6) is an EXTENSION, as q-EI is: the reference has no such type.  It is the logarithm of the TEXTBOOK expected
 * improvement, params = [tau], in forms that stay finite and accurate for any z = (mu - tau) / sigma:
 *     LogEI(mu, s2) = log sigma + log h(z),   h(z) = phi(z) + z Phi(z)
 *     d/dmu = Phi(z) / (sigma h(z))           d/ds2 = phi(z) / (2 s2 h(z)) > 0
 *     s2 == 0:  value = mu > tau ? log(mu - tau) : -Inf;  d/dmu = mu > tau ? 1 / (mu - tau) : 0;  d/ds2 = 0
 * Every entry point of bohip.h that takes an acq_id for scoring takes 6 as well (score, score_grad, acquire_max, select_batch --
 * BOHIP_BATCH_RAISE_TAU applies --, direct_max, the sharded and multi-GPU forms); 5 keeps its one place and 7 stays unknown.
 * A score of -Inf never wins an arg-max: a batch whose scores are all -Inf gives the record {val = -Inf, idx = -1}, as an all-NaN
 * batch does.
 *
 *   bohip_acq_eval   the reference's functor a(mu, s2) (src/acquisitionfunctions.jl:4-9) and its partials for n pairs, computed on
 *                    the current device by the very functions the scoring kernels inline -- one thread per element, no model
 *                    handle.  acq_id 0-4 and 6; acq_params as in bohip_gp_score (NULL only for MaxMean).  value, dmu, dvar: n
 *                    each; dmu and dvar are nullable TOGETHER (values only).  n == 0 returns at once.
 * BOHIP_E_ARG: unknown acq_id, n < 0, a null pointer where one is needed, only one of dmu / dvar.  BOHIP_E_NODEVICE: no device.
 */
#ifndef BOHIP_ACQ_H
#define BOHIP_ACQ_H
#include "bohip.h"
#define BOHIP_ACQ_LOGEI 6
#ifdef __cplusplus
extern "C" {
#endif

int bohip_acq_eval(int acq_id, const double *acq_params, int64_t n, const double *mu, const double *var,
                   double *value, double *dmu, double *dvar);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_ACQ_H */
