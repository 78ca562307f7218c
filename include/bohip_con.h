/*
 * bohip_con.h -- C ABI of constrained optimisation of libbohip.so: feasibility-weighted acquisitions over several models, and the
 * posterior's own Jacobians.  A header of its own beside bohip.h: the model's ABI (bohip.h, 62 symbols) is
 * unchanged.  Conventions (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of bohip.h.
 * ctypes: _lib.CON_SIGNATURES; Julia: julia/BOHipCon.jl.
 *
 * Role: an EXTENSION -- the reference's acquisition functor closes over ONE model and has no place for a constraint.  The product
 * form is the constrained expected improvement of Gardner et al. (ICML 2014) and Gelbart, Snoek & Adams (UAI 2014); the log form
 * adds log Phi to LogEI (bohip_acq.h) and survives deep infeasibility.
 *
 * 1. The quantity.  Model 0 is the objective, models 1..C (0 <= C <= BOHIP_CON_CMAX) are the constraints: bohip_gp handles of one
 *    dimension d on one device, each with its own kernel id, hyper-parameters and observations.  Constraint c has a finite
 *    threshold t_c and a sense s_c: +1 feasible where g_c(x) >= t_c, -1 feasible where g_c(x) <= t_c.  With (mu_c, s2_c) the latent
 *    posterior of bohip_gp_predict (clamp included), contraction off (tests/con_reference.py is the NumPy twin, operation for
 *    operation), c0 = 0.9189385332046728, sqrt 2 = 1.4142135623730951:
 *      mu_c or s2_c not finite, or s2_c < 0   l_c = NaN, both partials NaN
 *      s2_c == 0                              l_c = 0 if s_c (mu_c - t_c) >= 0, else -Inf;  both partials 0
 *      otherwise  sd = sqrt(s2_c),  z = (s_c (mu_c - t_c)) / sd,  phi = 0.3989422804014327 exp(-0.5 (z z)) and
 *        z > 0        Phic = 0.5 erfc(z / sqrt 2),   l_c = log1p(-Phic),  rho = phi / (1 - Phic)
 *        -4 < z <= 0  Phi = 0.5 erfc(-z / sqrt 2),   l_c = log(Phi),      rho = phi / Phi
 *        z <= -4      t = -z;  r = 2 / (t + 3 / (t + ...)) and c1 = 1 / (t + r) from csrc/acq_log.h's continued fraction at depth 40;
 *                     rho = t + c1,  l_c = (-0.5 (z z) - c0) - log(t + c1)      (z^2 / 2 is the leading term, never a difference)
 *        dl_c/dmu_c = (s_c rho) / sd,      dl_c/ds2_c = -((z rho) / (2 s2_c))
 *    L = sum_c l_c, added in ascending c from +0.0.  a(mu_0, s2_0): bohip_acq_eval's functor, da its partials.
 *      BOHIP_ACQ_EI, BOHIP_ACQ_PI    e = exp(L),  score = a e;   d/d(mu_0, s2_0) = e da,   d/d(mu_c, s2_c) = score dl_c;  all 0 if e == 0
 *      BOHIP_ACQ_LOGEI               score = a + L;              d/d(mu_0, s2_0) = da,     d/d(mu_c, s2_c) = dl_c
 *      BOHIP_CON_FEASIBILITY (-1)    score = L;                  d/d(mu_0, s2_0) = 0,      d/d(mu_c, s2_c) = dl_c
 *    A score of -Inf has partials 0; a NaN score has partials NaN.  UCB, MI, MaxMean and the Thompson id are refused: a signed
 *    score has no product form.  BOHIP_CON_FEASIBILITY with C = 1 is log PI of the constraint.
 *    Gradient in x:  grad = sum_m [ dscore/dmu_m grad mu_m + (s2_m > 0 ? dscore/ds2_m grad s2_m : 0) ], added in ascending m from
 *    +0.0 (the objective left out under BOHIP_CON_FEASIBILITY) -- a clamped variance has zero gradient, as in bohip_gp_score_grad.
 *    best: bohip_gp_score's record -- first maximum under strict '>' from -Inf, NaN never wins, {-Inf, -1} if nothing can win.
 *
 * 2. The symbols.
 *   bohip_gp_predict_grad  mu, var as bohip_gp_predict; dmu, dvar each d x R column-major (candidate j at [j d, (j + 1) d)):
 *                          grad mu = sum_j alpha_j dk*_j/dx,  grad s2 = -2 sum_j (cK^-1 k*)_j dk*_j/dx, the latter reported UNMASKED
 *                          (where var == 0 the clamp is the caller's).  Every kernel id, any R (candidate chunks inside the call),
 *                          any N the handle holds.  The route is the split-K one where the batch is too small to fill the chip
 *                          with whole-K jobs and the chunked one otherwise; mu and var are those of bohip_gp_predict_dev on that
 *                          route.  The sums over the observations run in bohip_gp_score_grad's order.
 *   bohip_con_values       the combine stage alone on the caller's moments: mu, var (C + 1) x R row-major, row 0 the objective (read
 *                          but unused under BOHIP_CON_FEASIBILITY).  value R, logfeas R (nullable), dmu and dvar (C + 1) x R
 *                          (nullable TOGETHER): the partials of the score.  gp gives the device and the stream only.
 *   bohip_gp_score_con     the whole call: every model's posterior on its own handle's stream, the constraints' streams joined to
 *                          the objective's by events, the combine and the record on the objective's; ONE host synchronisation.
 *                          Every output is nullable and only what is asked for is copied back.  grad d x R column-major; non-null
 *                          selects the gradient route.  mu, var (C + 1) x R; under BOHIP_CON_FEASIBILITY their row 0 is NaN and
 *                          the objective may have no observations.  The scores of a gradient call are those of a value call bit
 *                          for bit, and what is computed for candidate j depends on (models, x_j) alone as long as the batch stays
 *                          on one route (the route is chosen per model from R and its n, as in bohip_gp_score_grad).
 *                          A handle may serve several constraints (t_lo <= g <= t_hi) and may be the objective's.
 *                          Stage labels on the objective: con_combine; on every model: kstar, trigemm_sq[+V], gemm_U, split_V,
 *                          split_U, con_post.
 * Errors.  BOHIP_E_ARG: C outside [0, BOHIP_CON_CMAX]; a null handle or a null required pointer; R < 0; differing d or device; a
 * threshold that is not finite; a sense other than +1 / -1; a refused acq_id; only one of dmu / dvar.  BOHIP_E_STATE: a model the
 * score needs has no observations.  Scratch lives on the objective's handle, grows on demand and is freed by bohip_gp_destroy.
 */
#ifndef BOHIP_CON_H
#define BOHIP_CON_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_CON_CMAX 16
#define BOHIP_CON_FEASIBILITY (-1)

int bohip_gp_predict_grad(bohip_gp *gp, const double *Xs, int64_t R, double *mu /* R */, double *var /* R */,
                          double *dmu /* d x R */, double *dvar /* d x R */);
int bohip_con_values(bohip_gp *gp, int acq_id, const double *acq_params, int64_t C, const double *thresholds /* C */,
                     const int *senses /* C */, const double *mu, const double *var /* (C + 1) x R */, int64_t R,
                     double *value /* R */, double *logfeas /* R, nullable */, double *dmu,
                     double *dvar /* (C + 1) x R, nullable TOGETHER */, bohip_best *best /* nullable */);
int bohip_gp_score_con(bohip_gp *obj, int acq_id, const double *acq_params, int64_t C, bohip_gp *const *cons /* C */,
                       const double *thresholds /* C */, const int *senses /* C */, const double *Xs, int64_t R,
                       double *score /* R */, double *logfeas /* R */, double *grad /* d x R */, double *mu,
                       double *var /* (C + 1) x R */, bohip_best *best);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_CON_H */
