/*
 * bohip_mo.h -- C ABI of two-objective optimisation of libbohip.so: the observed Pareto front and the exact expected hypervolume
 * improvement (EHVI) over it, for two models scored together.  A header of its own beside bohip.h: the model's ABI
 * (bohip.h, 62 symbols) is unchanged.  Conventions (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of
 * bohip.h.  ctypes: _lib.MO_SIGNATURES; Julia: julia/BOHipMO.jl.
 *
 * Role: an EXTENSION -- the reference optimises one objective.  The strip form of the two-objective EHVI is that of Emmerich,
 * Yang, Deutz, Wang & Fonseca (2016) and Yang, Emmerich, Deutz & Baeck (2019); Daulton, Balandat & Bakshy (NeurIPS 2020) give the
 * context (q points, many objectives), which is out of scope here.
 *
 * 1. The quantity.  Both objectives are MAXIMISED.  A reference point r = (r1, r2), finite.  The front F of n points,
 *    0 <= n <= BOHIP_MO_FRONT_MAX: the observations that strictly dominate r in both coordinates and are not weakly dominated by
 *    another observation, ascending in f1 (hence descending in f2), of equal points one.  Corners c_0 = r1, c_i = F[i].f1
 *    (i = 1..n), c_{n+1} = +Inf; heights b_i = F[i].f2 (i = 1..n), b_{n+1} = r2.  Strip i = 1..n+1 spans [c_{i-1}, c_i] above b_i.
 *    With independent latent posteriors N(mu_m, s2_m) of bohip_gp_predict (clamp included), contraction off, sqrt 2 =
 *    1.4142135623730951 (tests/mo_reference.py is the NumPy twin, operation for operation):
 *      Psi_m(t) = E[(f_m - t)+]:
 *        t = +Inf   Psi = 0, Phi = 0, phi = 0
 *        s2_m == 0  D = mu_m - t;  Psi = D > 0 ? D : 0,  Phi = D > 0 ? 1 : 0,  phi = 0
 *        otherwise  sd = sqrt(s2_m),  D = mu_m - t,  z = D / sd,  Phi = 0.5 erfc(-z / sqrt 2),
 *                   phi = 0.3989422804014327 exp(-0.5 (z z)),  Psi = sd phi + D Phi
 *      EHVI = sum_i [Psi_1(c_{i-1}) - Psi_1(c_i)] Psi_2(b_i)
 *    and with Delta_i = Psi_1(c_{i-1}) - Psi_1(c_i), the sums A1 = sum_i [phi_1(c_{i-1}) - phi_1(c_i)] Psi_2(b_i) and
 *    A2 = sum_i Delta_i phi_2(b_i):
 *      d/dmu_1 = sum_i [Phi_1(c_{i-1}) - Phi_1(c_i)] Psi_2(b_i)        d/ds2_1 = s2_1 > 0 ? A1 / (2 sd_1) : 0
 *      d/dmu_2 = sum_i Delta_i Phi_2(b_i)                              d/ds2_2 = s2_2 > 0 ? A2 / (2 sd_2) : 0
 *    Summation order (BOHIP_MO_GROUP = 16 lanes take one candidate, whatever R is): lane g = 0..15 adds the terms of strips
 *    g + 1, g + 17, g + 33, ... in ascending order into its own accumulator from +0.0; the 16 accumulators are then added by a
 *    butterfly, a_g <- a_g + a_{g xor o} for o = 8, 4, 2, 1 in that order, and lane 0's result is the sum.  All five sums use this
 *    order.  Each Psi_1(c_i) is evaluated once: strip i takes its lower corner from strip i - 1.  So what is computed for candidate
 *    j depends on (mu_j, s2_j, F, r) alone, bit for bit.
 *    A moment that is not finite, or s2_m < 0: the score and the four partials are NaN.
 *    Gradient in x:  grad = sum_m [ dE/dmu_m grad mu_m + (s2_m > 0 ? dE/ds2_m grad s2_m : 0) ], added in ascending m from +0.0 --
 *    a clamped variance has zero gradient, as in bohip_gp_score_grad.
 *    best: bohip_gp_score's record -- first maximum under strict '>' from -Inf, NaN never wins, {-Inf, -1} if nothing can win.
 *
 * 2. The symbols.
 *   bohip_mo_front        HOST code only (a sort and a sweep; no device is touched, so it works on a machine without a GPU).
 *                         Y is 2 x n row-major (row 0 the first objective).  Writes the front into `front`, 2 x cap row-major
 *                         (f1 of point i at front[i], f2 at front[cap + i]), its size into n_front and the dominated hypervolume
 *                         hv = sum_i (f1_i - f1_{i-1}) (f2_i - r2), f1_0 = r1, added in ascending i from +0.0, into hv (n_front and
 *                         hv nullable).  cap = 0 is a size query: front is not written.  0 < cap < the front's size is BOHIP_E_ARG
 *                         (n_front is still written).
 *   bohip_mo_ehvi_values  the combine stage alone on the caller's moments: front 2 x n_front row-major, mu and var 2 x R row-major
 *                         (row m objective m).  value R; dmu, dvar 2 x R (nullable TOGETHER): the four partials.  gp gives the
 *                         device and the stream only.  The front is validated: finite, strictly ascending in f1, strictly
 *                         descending in f2, strictly above ref in both.  value and best are the same bytes with and without the
 *                         partials.
 *   bohip_gp_score_mo     the whole call: the candidates are uploaded once into obj0's block, obj1's stream waits for the copy
 *                         and runs its posterior into obj0's block, an event joins it back before the EHVI and the record run on
 *                         obj0's stream; ONE host synchronisation.  Every output is nullable and only what is asked for is copied
 *                         back.  grad d x R column-major; non-null selects the gradient route.  mu, var 2 x R.  The scores of a
 *                         gradient call are those of a value call bit for bit, and what is computed for candidate j depends on
 *                         (models, front, ref, x_j) alone as long as the batch stays on one posterior route (chosen per model from
 *                         R and its n, as in bohip_gp_score_grad).  obj0 and obj1 may be the same handle, may hold different
 *                         numbers of observations and different kernel ids.
 *                         Stage labels on obj0: mo_ehvi; on both models: kstar, trigemm_sq[+V], gemm_U, split_V, split_U, con_post.
 * Errors.  BOHIP_E_ARG: a null handle or a null required pointer; n, n_front, R or cap < 0; a reference point that is not finite;
 * a NaN or an infinite observation; a front that fails the validation; only one of dmu / dvar; differing d or device.
 * BOHIP_E_UNSUPPORTED: n_front > BOHIP_MO_FRONT_MAX.  BOHIP_E_STATE: a model without observations.  Scratch lives on obj0's handle
 * (the block of bohip_con.h's calls and a front buffer), grows on demand and is freed by bohip_gp_destroy.
 */
#ifndef BOHIP_MO_H
#define BOHIP_MO_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_MO_FRONT_MAX 1024
#define BOHIP_MO_GROUP 16

int bohip_mo_front(const double *Y /* 2 x n */, int64_t n, const double *ref /* 2 */, double *front /* 2 x cap */, int64_t cap,
                   int64_t *n_front, double *hv);
int bohip_mo_ehvi_values(bohip_gp *gp, const double *front /* 2 x n_front */, int64_t n_front, const double *ref /* 2 */,
                         const double *mu, const double *var /* 2 x R */, int64_t R, double *value /* R */, double *dmu,
                         double *dvar /* 2 x R, nullable TOGETHER */, bohip_best *best /* nullable */);
int bohip_gp_score_mo(bohip_gp *obj0, bohip_gp *obj1, const double *front /* 2 x n_front */, int64_t n_front,
                      const double *ref /* 2 */, const double *Xs, int64_t R, double *score /* R */, double *grad /* d x R */,
                      double *mu, double *var /* 2 x R */, bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_MO_H */
