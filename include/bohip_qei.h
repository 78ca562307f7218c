/*
 * bohip_qei.h -- C ABI of the greedy Monte-Carlo q-EI batch selection of libbohip.so.  A header of its own beside
 * bohip.h: the model's ABI (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls, status codes,
 * bohip_last_error) are those of bohip.h.  ctypes: _lib.QEI_SIGNATURES; Julia: julia/BOHipQEI.jl.
 *
 * Role: an EXTENSION, as bohip_gp_select_batch is -- the reference proposes one point per iteration.  It consumes the joint draw
 * of the reference, myrand(model, X::Matrix) = rand(gp, X) (src/models/gp.jl:7), as bohip_gp_sample_joint produces it, and
 * scores a batch as a batch:
 *     qEI(B) = E[max(max_{j in B} f_j - tau, 0)]  ~  (1/S) sum_s max(max_{j in B} F_sj - tau, 0)
 * maximised greedily over the candidates.  The sample average is a monotone submodular set function of B, so the greedy batch is
 * within (1 - 1/e) of the best batch of its size on the same draws.  With q = 1 it estimates the TEXTBOOK expected improvement
 * Delta Phi(z) + sigma phi(z); the reference's ExpectedImprovement functor computes Delta Phi(z) + phi(z), and
 * q-EI takes only tau from that class.
 *
 * Definition (the contract).  F: S x R row-major, draw s at F[s R + j]; tau finite; q >= 1.  State m_s = tau for every draw s.
 * Round k = 0 .. q-1:
 *     u(f, m)   = (f > m) ? f - m : 0                    NaN and -Inf contribute 0; no NaN is ever produced
 *     part_b(j) = sum_{s = 32 b .. min(32 b + 31, S - 1)} u(F_sj, m_s)     s ascending, plain FP64 adds starting from +0.0
 *     tot(j)    = sum_b part_b(j)                        b ascending
 *     gain_k(j) = tot(j) / S                             one IEEE division
 *     j*        = the first maximum of gain_k under strict '>' starting from 0 (value descending, index ascending: the tie rule
 *                 of bohip_gp_score with the floor at 0 instead of -Inf)
 *     no candidate with gain > 0:  idx[k .. q-1] = -1, gain[k .. q-1] = 0, and the selection is over
 *     otherwise idx[k] = j*, gain[k] = gain_k(j*), m_s <- (F_sj* > m_s) ? F_sj* : m_s
 * sum_k gain[k] is the sample-average q-EI of the batch.  A picked candidate, or a duplicate of one, has gain exactly 0 afterwards,
 * so no mask is kept.  A +Inf entry wins once (gain +Inf) and is dead afterwards.  The summation order above (32 draws per block)
 * is part of the ABI: the result depends on (F, tau) only -- not on q (the first k entries of a q-call are the k-call's, bit for
 * bit), not on launch geometry, not on whether F came from a draw or from the caller.  tests/qei_reference.py is its NumPy twin.
 *
 *   bohip_gp_qei_batch    draws exactly bohip_gp_sample_joint's S x R samples for the same (Xs, R, S, seed, jitter_rel, max_tries)
 *                         -- the same kernels, the same switch between them, the same retries -- leaves them on the device and
 *                         runs the selection there.  idx[q], gain[q]; samples: S x R (host) or NULL; jitter_used / tries_used as
 *                         in bohip_gp_sample_joint (nullable).  Only these cross to the host.  One host synchronisation per call
 *                         plus one per jitter retry.  The model is not changed.
 *   bohip_gp_qei_select   the selection alone on the caller's S x R matrix (host), uploaded into the same device buffer.  The
 *                         handle supplies the device and the stream only: a model without observations will do.  Draws from other
 *                         sources (sample paths: bohip_paths_eval) are selected from by the same kernels.
 * BOHIP_E_ARG: null handle or pointers; R, S or q < 1; q > R; tau not finite; jitter_rel negative or not finite, max_tries < 0.
 * BOHIP_E_STATE: bohip_gp_qei_batch on a model without observations.  BOHIP_E_UNSUPPORTED: R beyond one candidate chunk
 * (bohip_gp_sample_joint's limit; bohip_gp_qei_batch only); S R doubles plus the partial sums above 8 GiB, or more than 65535
 * blocks of draws (the text names the largest S).  BOHIP_E_NOTPD as bohip_gp_sample_joint.
 * Workspace (m, the ceil(S / 32) x R partial sums, a few words) lives on the handle, grows on demand and is freed by
 * bohip_gp_destroy.
 */
#ifndef BOHIP_QEI_H
#define BOHIP_QEI_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

int bohip_gp_qei_batch(bohip_gp *gp, const double *Xs, int64_t R, int64_t S, uint64_t seed, double jitter_rel, int max_tries,
                       double tau, int64_t q, int64_t *idx /* q */, double *gain /* q */,
                       double *samples /* S x R, nullable */, double *jitter_used, int *tries_used);
int bohip_gp_qei_select(bohip_gp *gp, const double *samples /* S x R host */, int64_t S, int64_t R, double tau, int64_t q,
                        int64_t *idx, double *gain);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_QEI_H */
