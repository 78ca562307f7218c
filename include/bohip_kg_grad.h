/*
 * bohip_kg_grad.h -- C ABI of the knowledge gradient at free points and of its gradient in the point.  A header of its
 * own beside bohip.h and bohip_kg.h: the model's ABI (bohip.h, 62 symbols) and bohip_kg.h's two symbols are unchanged.  Conventions
 * (Float64 / Int64, blocking calls, status codes, bohip_last_error) are those of bohip.h.  ctypes: _lib.KG_GRAD_SIGNATURES; Julia:
 * julia/BOHipKGGrad.jl.
 *
 * Role: an EXTENSION -- the knowledge gradient for continuous parameters (Scott, Frazier & Powell 2011).  bohip_gp_kg evaluates points
 * of a candidate set against that set; here the set is a DISCRETISATION kept on the handle and the evaluation point is anywhere, so
 * KG is a function of x alone: it has a gradient and an ascent can climb it.
 *
 * Definition (the contract).  Discretisation A = a_0 .. a_{R-1}, R + 1 <= BOHIP_KG_RMAX, set once and kept on the handle; mu_j = mu(a_j);
 * nu as in bohip_kg.h.  The lines of an evaluation point x (R + 1 of them), s = sqrt(sigma^2(x) + nu):
 *     j < R    intercept mu_j,   slope b_j = Sigma(a_j, x) / s            Sigma(a_j, x) = k(x, a_j) - v_x . v_{a_j},  v(.) = W k(X, .)
 *     j = R    intercept mu(x),  slope sigma^2(x) / s                     the point's own line; sigma^2 the clamped posterior variance
 * KG(x) and nseg: bohip_kg.h's march on these R + 1 lines -- its start rule, tie rules, term forms and order of additions -- so they
 * equal bohip_kg_lines on the same (a, b) bit for bit.
 * Gradient.  c_0 .. c_n the envelope's lines, z_1 .. z_n its break points, z_0 = -Inf, z_{n+1} = +Inf, q_i = phi(z_i) - phi(z_{i+1}),
 * P_i = Phi(z_{i+1}) - Phi(z_i).  By the envelope theorem the break points carry no derivative:
 *     grad KG(x) = sum_i q_i grad b_{c_i}(x) + c_mu grad mu(x),   c_mu = P_own [own line on the envelope] - [mu(x) > max_j mu_j strictly]
 * where both brackets hold P_own - 1 is formed as -(Phi(z_own) + Phi(-z_{own+1})), so nothing cancels; P_own alone as a difference of two
 * tail values on the side of the origin its span begins on.
 *     grad b_j   = grad_x Sigma(a_j, x) / s - Sigma(a_j, x) grad sigma^2 / (2 s^3)    (j < R)
 *     grad b_own = grad sigma^2 (sigma^2 + 2 nu) / (2 s^3)
 *     grad_x Sigma(a_j, x) = grad_x k(x, a_j) - sum_n (W'v_{a_j})_n grad_x k(x, X_n);  grad mu = sum_n alpha_n grad_x k(x, X_n);
 *     grad sigma^2 = -2 sum_n (W'v_x)_n grad_x k(x, X_n)
 * Collected, with c_sigma the total coefficient of grad sigma^2 (the lines < R in envelope order, then the own line's):
 *     grad KG = sum_n e[n] grad_x k(x, X_n) + sum_{i: c_i < R} (q_i / s) grad_x k(x, a_{c_i})
 *     e = c_mu alpha + W'(-2 c_sigma v_x - (1 / s) sum_{i: c_i < R} q_i v_{a_{c_i}})
 * Zero rules: a clamped sigma^2(x) = 0 has c_sigma = 0, as in bohip_gp_score_grad; Matern 1/2 takes dk/dx = 0 at r = 0, as everywhere;
 * where sigma^2(x) + nu is not positive and finite KG = 0, nseg = 0 and the gradient is zero.
 * best: the arg-max over the E values under bohip_gp_score's rule.
 *
 *   bohip_gp_kg_set_points   keeps a copy of A (R x d, row = point) on the handle; R = 0 releases it and everything derived from it.
 *                            Nothing runs on the device: mu_A and V'_A are built by the next bohip_gp_kg_grad, and again by the first
 *                            one after the model changed (observations, hyper-parameters, a refit's jitter) -- from the kept A.
 *   bohip_gp_kg_grad         E points anywhere: kg[E], grad[E][d], and nullable nseg[E], mu[E], var[E] (the point's own posterior),
 *                            best.  One pass that stores V'_x, the cross-covariances on the MFMA engine, one workgroup's march per
 *                            point, one triangular product, one contraction with dk/dx.  One host synchronisation.  Two identical
 *                            calls return identical bytes.  The model is not changed.
 *   bohip_gp_kg_points_info  what = BOHIP_KG_POINTS_R (value[0] = R), _REBUILDS (how often mu_A / V'_A were built), _BYTES (device
 *                            bytes of the resident state and the call block), _LINES and _LINE_ROWS: DIAGNOSTIC, NOT PART OF THE STABLE
 *                            INTERFACE (they exist so that a test can hand the device's own lines to bohip_kg_lines; they may change
 *                            or go).  _LINES copies the rows the last call's march read, rows x (R + 1) packed -- Sigma(a_j, x) for
 *                            j < R, then sigma^2(x) -- for the points of that call's LAST BLOCK ONLY: all E points while E (R + 1) 20
 *                            bytes fit 256 MB and one K*' chunk, else the last rows of E; value[0 .. cap) must hold them.
 *                            _LINE_ROWS: how many rows that is (0 before any call, and after bohip_gp_kg_set_points).
 * BOHIP_E_ARG: null handle or pointers (gp, A with R > 0, Xe, kg, grad, value); R < 0; E < 1; unknown `what`; cap too small.
 * BOHIP_E_STATE: bohip_gp_kg_grad on a model without observations, or without points; _LINES before any call.
 * BOHIP_E_UNSUPPORTED: R + 1 above BOHIP_KG_RMAX (a point's lines live in one workgroup's LDS); the message names the limit.
 * A model with replicated sites is served as bohip_gp_kg serves it: nu is the model's one noise term.
 * Scratch lives on the handle, grows on demand and is freed by bohip_gp_destroy.
 */
#ifndef BOHIP_KG_GRAD_H
#define BOHIP_KG_GRAD_H
#include "bohip_kg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BOHIP_KG_POINTS_R 0
#define BOHIP_KG_POINTS_REBUILDS 1
#define BOHIP_KG_POINTS_BYTES 2
#define BOHIP_KG_POINTS_LINES 3
#define BOHIP_KG_POINTS_LINE_ROWS 4

int bohip_gp_kg_set_points(bohip_gp *gp, const double *A /* R x d, row = point */, int64_t R);
int bohip_gp_kg_points_info(bohip_gp *gp, int what, double *value, int64_t cap);
int bohip_gp_kg_grad(bohip_gp *gp, const double *Xe /* E x d */, int64_t E, double *kg /* E */, double *grad /* E x d */,
                     int32_t *nseg /* E, nullable */, double *mu /* E, nullable */, double *var /* E, nullable */,
                     bohip_best *best /* nullable */);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_KG_GRAD_H */
