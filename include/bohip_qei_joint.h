/*
 * bohip_qei_joint.h -- C ABI of the joint q-EI of B batches of q points and its gradient of libbohip.so.  A header of
 * its own beside bohip_qei.h: that header keeps its two symbols, bohip.h its 62.  Conventions (Float64 / Int64, blocking calls,
 * status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.QEI_JOINT_SIGNATURES; Julia: julia/BOHipQEIJoint.jl.
 *
 * Role: an EXTENSION, as bohip_gp_qei_batch is.  That call picks a batch from a finite candidate set; this one scores B batches as
 * batches anywhere in the box and returns the gradient in every coordinate of every point, which is what an ascent over the q d
 * variables of a batch climbs (Wilson, Hutter & Deisenroth 2018: the reparameterised sample average).
 *
 * Definition (the contract).  Xs: B q points, group b = rows b q .. b q + q - 1, [B q][d] row-major as bohip_gp_score_grad takes its
 * candidates.  Per group, with sigma_f^2 = exp(2 logsig):
 *     mu (q), Sigma (q x q)   the noise-free posterior mean and covariance of f at the group's points,
 *                             Sigma = K(X_b, X_b) - V_b V_b' from the resident inverse factor (V = W K*)
 *     L L' = Sigma + jitter_rel sigma_f^2 I    formed once, no retries, right-looking: at column k with d = A_kk,
 *                             A_ji <- A_ji - A_jk (A_ik / d) for j >= i > k, then L_ji = A_ji / sqrt(A_ii).  A pivot d that is not a
 *                             finite positive number FLAGS the group: pivot[b] = k + 1 (1-based), value[b] = -Inf, a zero gradient
 *                             -- bohip_gp_mll_grad_batch's rule, not an error of the call, and no other group is touched.  (Written
 *                             this way a repeated point cancels exactly: at jitter_rel = 0 its pivot is never positive.)
 *     z_s,i = bohip_thompson_normal(seed, s, i), i < q: the same for every group (common random numbers)
 *     f_s = mu + L z_s (row i: mu_i, then + L_ik z_s,k for k = 0 .. i),   j*_s = the first maximum of f_s under strict '>',
 *     a_s = [f_s,j* > tau]
 *     value[b] = (sum_s a_s (f_s,j* - tau)) / S        s ascending, plain FP64 adds from +0.0, one division
 * Gradient, with g = 1 / S:
 *     mubar_j = sum_s a_s [j*_s = j] g,     Lbar_ji = sum_s a_s [j*_s = j] g z_s,i  (i <= j)       both over s ascending
 *     Sbar = sym(L^-T Phi(L'Lbar) L^-1)     Phi: the lower triangle with its diagonal halved;  sym(A) = (A + A') / 2
 *     e_j[n] = mubar_j alpha[n] - 2 sum_i Sbar_ji u_i[n],     u_i = W'W k*(x_i)
 *     grad_j = sum_n dk(x_j, X_n)/dx e_j[n] + 2 sum_{i != j} Sbar_ji dk(x_j, x_i)/dx_j       (i ascending, after the first sum)
 * dk(x, y)/dx_k = fx(r) il2_k (x_k - y_k), fx = 2 dk/dr (Matern 1/2: 0 at r = 0).  With the seed fixed the value is one deterministic
 * function of the points and grad is its derivative wherever the arg-max does not change.  A group in which no sample exceeds tau has
 * value 0 and an exactly zero gradient.  tests/qei_joint_reference.py is the NumPy twin.
 *
 *   bohip_gp_qei_joint   value[B]; grad [B q][d] row-major (d x B q column-major) or NULL: then U' = V'W is not formed and neither
 *                        the mix nor the finish runs; mu [B q] (the latent means) or NULL; pivot[B] or NULL.  The model is not
 *                        changed; two identical calls return identical bytes; a group's value and gradient depend on (model, its
 *                        points, S, seed, tau, jitter_rel) only -- not on B, not on the group's position among the groups.
 *                        Stage labels: kstar, trigemm_sq+V, gemm_U, qeij_cov, qeij_core, qeij_mix, qeij_grad_finish.
 * BOHIP_E_ARG: null handle, Xs or value; B < 1; q outside [1, BOHIP_QEIJ_QMAX]; S outside [1, BOHIP_QEIJ_SMAX]; tau or jitter_rel not
 * finite, jitter_rel < 0.  BOHIP_E_STATE: no observations.  BOHIP_E_UNSUPPORTED: B q beyond one candidate chunk (the text names the
 * largest B); a model with replicated sites.  Errors leave the handle usable.
 * Workspace (Z, Sigma, Sbar, mubar, the results) lives on the handle, grows on demand and is freed by bohip_gp_destroy.
 */
#ifndef BOHIP_QEI_JOINT_H
#define BOHIP_QEI_JOINT_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_QEIJ_QMAX 16
#define BOHIP_QEIJ_SMAX 1024
int bohip_gp_qei_joint(bohip_gp *gp, const double *Xs, int64_t B, int64_t q, int64_t S, uint64_t seed, double tau, double jitter_rel,
                       double *value, double *grad, double *mu, int64_t *pivot);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_QEI_JOINT_H */
