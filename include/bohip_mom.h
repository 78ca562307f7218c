/*
 * bohip_mom.h -- C ABI of optimisation with two to four objectives of libbohip.so: the observed Pareto front, its decomposition into
 * boxes and the exact expected hypervolume improvement (EHVI) as a sum over them, for M models scored together.  A
 * header of its own beside bohip_mo.h: the model's ABI (bohip.h, 62 symbols) and bohip_mo.h (3 symbols, the two-objective strip
 * form) are unchanged.  Conventions (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of bohip.h.
 * ctypes: _lib.MOM_SIGNATURES; Julia: julia/BOHipMOM.jl.
 *
 * Role: an EXTENSION -- the reference optimises one objective.  The box form of the EHVI is that of Emmerich, Yang, Deutz, Wang &
 * Fonseca (2016) and Yang, Emmerich, Deutz & Baeck (2019); the decomposition of the non-dominated region into boxes by slabs is the
 * dimension sweep of Lacour, Klamroth & Fonseca (2017) in its simplest form; Daulton, Balandat & Bakshy (NeurIPS 2020) give the
 * context (q points, noisy fronts), which is out of scope here.
 *
 * 1. The quantity.  M objectives, 2 <= M <= BOHIP_MOM_OBJ_MAX, all MAXIMISED.  A reference point r, finite.  The front F of n points,
 *    0 <= n <= BOHIP_MOM_FRONT_MAX: observations strictly above r in every coordinate, none weakly dominated by another, of equal
 *    points one.  What is computed depends on the SET F, not on the order of its points.
 *    Levels.  Per objective m the level array L_m: L_m[0] = r_m, then the distinct values F[.][m] ascending, then +Inf;
 *    n_levels[m] <= n + 2 entries.
 *    Boxes.  decomp(P, r) of a non-dominated set P above r in k dimensions:
 *      k = 1   one box [max(r_1, max_P p_1), +Inf)
 *      k > 1   z_0 = r_k < z_1 < ... < z_K the distinct values of the last coordinate in P, z_{K+1} = +Inf; for slab j = 0 .. K in
 *              ascending order: Q_j = the points of P with p_k > z_j, projected on the first k - 1 coordinates and reduced to their
 *              non-dominated subset (weak dominance; of equal projections one); emit decomp(Q_j, r[1 .. k-1]) x [z_j, z_{j+1}),
 *              the boxes of the recursion in its own order.
 *    The boxes B = [l_B, u_B) partition the region above r that no point of F weakly dominates; box b is stored as 2M level
 *    indices, lo_m(b) and hi_m(b) with l_{B,m} = L_m[lo_m], u_{B,m} = L_m[hi_m].  The list is a function of the set F and r alone.
 *    The dominated hypervolume from the same recursion: HV_1(P) = max(r_1, max_P p_1) - r_1, HV_k(P) = sum_{j = 0 .. K-1}
 *    (z_{j+1} - z_j) HV_{k-1}(Q_j), added in ascending j from +0.0.
 *    With independent latent posteriors N(mu_m, s2_m) of bohip_gp_predict (clamp included), contraction off, sqrt 2 =
 *    1.4142135623730951 (tests/mom_reference.py is the NumPy twin, operation for operation), Psi, Phi, phi exactly bohip_mo.h's:
 *      Psi_m(t) = E[(f_m - t)+]:
 *        t = +Inf   Psi = 0, Phi = 0, phi = 0
 *        s2_m == 0  D = mu_m - t;  Psi = D > 0 ? D : 0,  Phi = D > 0 ? 1 : 0,  phi = 0
 *        otherwise  sd = sqrt(s2_m),  D = mu_m - t,  z = D / sd,  Phi = 0.5 erfc(-z / sqrt 2),
 *                   phi = 0.3989422804014327 exp(-0.5 (z z)),  Psi = sd phi + D Phi
 *    each evaluated ONCE per (candidate, objective, level), and with dPsi_m(b) = Psi_m(L_m[lo_m(b)]) - Psi_m(L_m[hi_m(b)]) (dPhi_m,
 *    dphi_m likewise):
 *      EHVI     = sum_b prod_m dPsi_m(b)
 *      d/dmu_m  = sum_b dPhi_m(b) prod_{l != m} dPsi_l(b)
 *      d/ds2_m  = s2_m > 0 ? [ sum_b dphi_m(b) prod_{l != m} dPsi_l(b) ] / (2 sd_m) : 0
 *    Product order: the M factors in ascending objective, p = f_0, p = p f_1, ..., p = p f_{M-1} (factor m replaced by dPhi_m or
 *    dphi_m in the partials).  Summation order (one wavefront of BOHIP_MOM_LANES = 64 lanes takes one candidate, whatever R is):
 *    lane g adds the terms of boxes g, g + 64, g + 128, ... in ascending order into its own accumulator from +0.0; the 64
 *    accumulators are then added by a butterfly, a_g <- a_g + a_{g xor o} for o = 32, 16, 8, 4, 2, 1 in that order, and lane 0's
 *    result is the sum.  All 2M + 1 sums use this order.  So what is computed for candidate j depends on (mu_j, s2_j, the set F, r)
 *    alone, bit for bit.
 *    A moment that is not finite, or s2_m < 0: the score and the 2M partials are NaN.
 *    Gradient in x:  grad = sum_m [ dE/dmu_m grad mu_m + (s2_m > 0 ? dE/ds2_m grad s2_m : 0) ], added in ascending m from +0.0 --
 *    a clamped variance has zero gradient, as in bohip_gp_score_grad.
 *    best: bohip_gp_score's record -- first maximum under strict '>' from -Inf, NaN never wins, {-Inf, -1} if nothing can win.
 *
 * 2. The symbols.
 *   bohip_mom_front        HOST code only (no device is touched).  Y is M x n row-major (row m objective m).  Writes the front into
 *                          `front`, M x cap row-major (coordinate m of point i at front[m cap + i]), in lexicographic ascending
 *                          order (by objective 0, then 1, ...), its size into n_front and the dominated hypervolume HV_M(F) into hv
 *                          (n_front and hv nullable).  cap = 0 is a size query: front is not written.  0 < cap < the front's size
 *                          is BOHIP_E_ARG (n_front is still written).  A front beyond BOHIP_MOM_FRONT_MAX points is returned whole;
 *                          hv is then computed all the same.
 *   bohip_mom_boxes        HOST code only: the levels and the boxes of a front (M x n_front row-major, any order).  levels is
 *                          M x (n_front + 2) row-major, row m holding L_m in its first n_levels[m] entries (the rest is not
 *                          written); boxes is 2M x cap row-major Int32, row m the lo_m and row M + m the hi_m of every box.
 *                          levels, n_levels and n_boxes are nullable.  cap = 0 is a size query: boxes is not written.  0 < cap < the
 *                          number of boxes is BOHIP_E_ARG (n_boxes is still written).  The front is validated.
 *   bohip_mom_ehvi_values  the stage alone on the caller's moments: front M x n_front, mu and var M x R row-major (row m objective
 *                          m).  value R; dmu, dvar M x R (nullable TOGETHER): the 2M partials.  gp gives the device and the stream
 *                          only.  value and best are the same bytes with and without the partials.
 *   bohip_gp_score_mom     the whole call, bohip_gp_score_mo's structure: the candidates are uploaded once into objs[0]'s block,
 *                          every other member's stream waits for the copy and runs its posterior into objs[0]'s block, events join
 *                          them back before the EHVI and the record run on objs[0]'s stream; ONE host synchronisation.  Every output
 *                          is nullable and only what is asked for is copied back.  grad d x R column-major; non-null selects the
 *                          gradient route.  mu, var M x R.  The scores of a gradient call are those of a value call bit for bit.
 *                          Handles may repeat, may hold different numbers of observations and different kernel ids.
 *                          Stage labels on objs[0]: mom_ehvi; on every member: kstar, trigemm_sq[+V], gemm_U, split_V, split_U,
 *                          con_post.
 * Errors.  BOHIP_E_ARG: a null handle or a null required pointer; M outside 2 .. BOHIP_MOM_OBJ_MAX; n, n_front, R or cap < 0; a
 * reference point that is not finite; a NaN or an infinite observation or front coordinate; a front point not strictly above ref; a
 * front that holds a weakly dominated or a duplicated point; only one of dmu / dvar; differing d or device.
 * BOHIP_E_UNSUPPORTED (the number is in the message): n_front > BOHIP_MOM_FRONT_MAX (bohip_mom_boxes, bohip_mom_ehvi_values,
 * bohip_gp_score_mom); more than BOHIP_MOM_BOX_MAX boxes.  BOHIP_E_STATE: a member without observations.  Scratch lives on
 * objs[0]'s handle (the block of bohip_con.h's calls, a level buffer and a box buffer), grows on demand and is freed by
 * bohip_gp_destroy.  The handle remembers which (front, ref) its two buffers hold: a call with the same arguments bit for bit, in the
 * same order -- every step of an ascent -- neither decomposes nor uploads again; the result does not depend on it.
 */
#ifndef BOHIP_MOM_H
#define BOHIP_MOM_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_MOM_OBJ_MAX 4
#define BOHIP_MOM_FRONT_MAX 256
#define BOHIP_MOM_BOX_MAX 65536
#define BOHIP_MOM_LANES 64

int bohip_mom_front(const double *Y /* M x n */, int64_t M, int64_t n, const double *ref /* M */, double *front /* M x cap */,
                    int64_t cap, int64_t *n_front, double *hv);
int bohip_mom_boxes(const double *front /* M x n_front */, int64_t M, int64_t n_front, const double *ref /* M */,
                    double *levels /* M x (n_front + 2) */, int64_t *n_levels /* M */, int32_t *boxes /* 2M x cap */, int64_t cap,
                    int64_t *n_boxes);
int bohip_mom_ehvi_values(bohip_gp *gp, int64_t M, const double *front /* M x n_front */, int64_t n_front, const double *ref /* M */,
                          const double *mu, const double *var /* M x R */, int64_t R, double *value /* R */, double *dmu,
                          double *dvar /* M x R, nullable TOGETHER */, bohip_best *best /* nullable */);
int bohip_gp_score_mom(bohip_gp *const *objs /* M handles */, int64_t M, const double *front /* M x n_front */, int64_t n_front,
                       const double *ref /* M */, const double *Xs, int64_t R, double *score /* R */, double *grad /* d x R */,
                       double *mu, double *var /* M x R */, bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_MOM_H */
