/*
 * bohip_qehvi.h -- C ABI of the greedy Monte-Carlo q-EHVI batch selection for two objectives of libbohip.so.  A
 * header of its own beside bohip.h: the model's ABI (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking
 * calls, status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.QEHVI_SIGNATURES; Julia: julia/BOHipQEHVI.jl.
 *
 * Role: an EXTENSION, as bohip_gp_qei_batch and bohip_gp_score_mo are -- the reference proposes one point per iteration and
 * optimises one objective.  It consumes the joint draw of the reference, myrand(model, X::Matrix) = rand(gp, X)
 * (src/models/gp.jl:7), as bohip_gp_sample_joint produces it, once per objective, and scores a batch as a batch (Daulton, Balandat
 * & Bakshy, NeurIPS 2020, for two objectives on common draws):
 *     qEHVI(B) = E[HV(front + {f(x_j), j in B}) - HV(front)]  ~  (1/S) sum_s [HV(front + {(F0_sj, F1_sj), j in B}) - HV(front)]
 * maximised greedily over the candidates.  The hypervolume of a set is monotone and submodular, so the greedy batch is within
 * (1 - 1/e) of the best batch of its size on the same draws, as bohip_qei.h states for q-EI.
 *
 * Definition (the contract).  Both objectives are MAXIMISED, as in bohip_mo.h.  F0, F1: S x R row-major, draw s of candidate j at
 * F[s R + j]; a front of n <= BOHIP_MO_FRONT_MAX points, validated as bohip_mo_ehvi_values validates it; ref = (r1, r2) finite;
 * q >= 1.
 * State: every draw s has a staircase T_s -- points ascending in f1, hence descending in f2 -- which starts as the front.  With
 * L = |T_s|: c_0 = r1, c_i = T_s[i].f1, c_{L+1} = +Inf, b_i = T_s[i].f2, b_{L+1} = r2.
 * Improvement of one point (a, b) of draw s:
 *     a or b not finite, or not a > r1, or not b > r2:  u_s = 0
 *     otherwise  u_s = sum_{i = 1 .. L+1} t_i,   w_i = (a > c_{i-1}) ? min(a, c_i) - c_{i-1} : 0,   h_i = (b > b_i) ? b - b_i : 0,
 *                t_i = (w_i > 0 and h_i > 0) ? w_i h_i : 0,  added in ascending i from +0.0, contraction off.  Every term is >= 0, so
 *                a strip whose term is exactly 0 may be skipped without changing a bit.
 * Round k = 0 .. q-1 (the blocking of bohip_qei.h):
 *     part_b(j) = sum_{s = 32 b .. min(32 b + 31, S - 1)} u_s(F0_sj, F1_sj)     s ascending, plain FP64 adds starting from +0.0
 *     tot(j)    = sum_b part_b(j)                        b ascending
 *     gain_k(j) = tot(j) / S                             one IEEE division
 *     j*        = the first maximum of gain_k under strict '>' starting from 0 (value descending, index ascending)
 *     no candidate with gain > 0:  idx[k .. q-1] = -1, gain[k .. q-1] = 0, and the selection is over
 *     otherwise idx[k] = j*, gain[k] = gain_k(j*), and for every draw s with p = (F0_sj*, F1_sj*):
 *         T_s is unchanged if p is not finite, is not strictly above ref in both coordinates, or is weakly dominated by a point of T_s;
 *         otherwise the points of T_s that p weakly dominates (a contiguous run) are removed and p is inserted in order.
 *         |T_s| <= n + k + 1 after round k.
 * sum_k gain[k] is the sample-average q-EHVI of the batch: (1/S) sum_s [HV(T_s final) - HV(front)].  A picked candidate, or a
 * duplicate of one, has gain exactly 0 afterwards, so no mask is kept.  The result depends on (F0, F1, front, ref) only -- not on q
 * (the first k entries of a q-call are the k-call's, bit for bit), not on launch geometry, not on where the draws came from.
 * tests/qehvi_reference.py holds the selection in exact rational arithmetic.
 *
 *   bohip_mo_qehvi_select  the selection alone on the caller's S x R matrices (host).  The handle supplies the device and the stream
 *                          only: a model without observations will do.
 *   bohip_gp_qehvi_batch   draws bohip_gp_sample_joint's S x R samples of obj0 for (Xs, R, S, seed, jitter_rel, max_tries) and of
 *                          obj1 for the seed  seed ^ BOHIP_QEHVI_SEED_XOR  (the objectives are independent given their own models:
 *                          equal seeds would correlate them), each on its own handle and stream, where they stay; obj1's stream is
 *                          joined to obj0's by an event, as in bohip_gp_score_mo, and the rounds run on obj0's stream.  idx[q],
 *                          gain[q]; samples: 2 x S x R (host; objective 0 first) or NULL; jitter_used / tries_used: one entry per
 *                          objective (nullable).  One host synchronisation per model plus one per jitter retry.  Nothing of either
 *                          model changes.  obj0 and obj1 may be the same handle.
 * BOHIP_E_ARG: null handles or pointers; R, S or q < 1; n_front < 0; q > R; a reference point that is not finite; a front that fails
 * the validation; jitter_rel negative or not finite, max_tries < 0; objectives that differ in dimension or device.
 * BOHIP_E_STATE: bohip_gp_qehvi_batch with a model without observations.  BOHIP_E_UNSUPPORTED: R beyond one candidate chunk
 * (bohip_gp_sample_joint's limit; bohip_gp_qehvi_batch only); q > BOHIP_QEHVI_QMAX; n_front > BOHIP_MO_FRONT_MAX; the two S x R
 * matrices plus the workspace above 8 GiB, or more than 65535 blocks of draws.  The message names the limit, and nothing is allocated
 * before the check.  BOHIP_E_NOTPD as bohip_gp_sample_joint.
 * Workspace (the S staircases of n + q + 2 entries, their lengths, the ceil(S / 32) x R partial sums, a few words) is one block on
 * obj0's handle (gp's for the selection alone), grows on demand and is freed by bohip_gp_destroy.
 */
#ifndef BOHIP_QEHVI_H
#define BOHIP_QEHVI_H
#include "bohip_mo.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_QEHVI_QMAX 16
#define BOHIP_QEHVI_SEED_XOR 0x9E3779B97F4A7C15ull

int bohip_mo_qehvi_select(bohip_gp *gp, const double *F0, const double *F1 /* S x R host */, int64_t S, int64_t R,
                          const double *front /* 2 x n_front */, int64_t n_front, const double *ref /* 2 */, int64_t q, int64_t *idx,
                          double *gain);
int bohip_gp_qehvi_batch(bohip_gp *obj0, bohip_gp *obj1, const double *front /* 2 x n_front */, int64_t n_front,
                         const double *ref /* 2 */, const double *Xs, int64_t R, int64_t S, uint64_t seed, double jitter_rel,
                         int max_tries, int64_t q, int64_t *idx, double *gain, double *samples /* 2 x S x R, nullable */,
                         double *jitter_used /* 2 */, int *tries_used /* 2 */);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_QEHVI_H */
