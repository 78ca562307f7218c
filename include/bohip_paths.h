/*
 * bohip_paths.h -- C ABI of the posterior sample paths of libbohip.so.  A header of its own beside bohip.h: the
 * model's ABI (bohip.h, 62 symbols) is unchanged; the six symbols here belong to a second opaque object, bohip_paths.  Conventions
 * (Float64 / Int64, d x n column-major, blocking calls, status codes, bohip_last_error) are those of bohip.h.
 * ctypes: _lib.PATHS_SIGNATURES; Julia: julia/BOHipPaths.jl.
 */
#ifndef BOHIP_PATHS_H
#define BOHIP_PATHS_H
#include "bohip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct bohip_paths bohip_paths;

/* posterior SAMPLE PATHS: draws of the posterior that are functions (pathwise conditioning, Matheron's rule with a
 * random-feature prior).  AN EXTENSION: the reference's myrand (src/models/gp.jl:6-7) draws at given points only, so its default
 * search for ThompsonSamplingSimple (:GN_DIRECT_L over x -> myrand(model, x), src/acquisition.jl:7-9) sees an unrelated draw at
 * every point it evaluates.  A paths object holds S functions that can be evaluated, and differentiated, anywhere afterwards:
 *   f_s(x) = beta + sum_m w_sm phi_m(x) + sum_j u_sj k(x, X_j)
 *   u_s    = K^-1 (y - beta - Phi(X) w_s - eps_s),  eps_si = sqrt(n) z,  n = what the model added to K's diagonal
 *            (exp(2 logNoise) + eps + jitter), K^-1 = W'W the model's own; the data term is exact, only the prior is approximated
 *   phi_2m(x) = sqrt(sigma2 / F) cos(omega_m . x),  phi_2m+1(x) = sqrt(sigma2 / F) sin(omega_m . x),  F = M / 2 frequencies
 *            (paired features, no phase: the prior variance sum_m phi_m(x)^2 is sigma2 exactly at every x)
 *   omega_mk = z_mk exp(-loglen_k) t_m;  t_m = 1 for SE, 1 / sqrt(chi2_m / n) for Matérn nu with n = 2 nu in {1, 3, 5} and
 *            chi2_m the sum of n squared standard normals (the Matérn spectral density is a multivariate t); iso kernels use loglen[0]
 * RANDOMNESS.  Every number is a bohip_thompson_normal(seed, stream, counter):
 *   basis   z_mk   = (seed, -1 - m, k)      k < d          the n normals of chi2_m = (seed, -1 - m, d + i), i < n
 *   path s  w_sm   = (seed, s, m)           m < M          eps_si = sqrt(n) (seed, s, M + i), i < N
 * Negative streams belong to the basis, so it does not depend on S, and S' < S paths are the leading paths of S, bit for bit.
 * The object is self-contained: it copies X, beta, the kernel and its hyper-parameters, Omega and the coefficients, so later
 * append / set_hyper / refit calls on the model neither change nor invalidate it.  It uses the handle's device and stream and must
 * be destroyed before the handle.  The model (L, W, alpha, the INFO counters) is not changed, except that a stale model is
 * refitted first, as by the scoring calls.  One host synchronisation per call.
 *   bohip_gp_paths_draw  *out = the object (NULL on failure).  Cost: two triangular products
 *                        with S right-hand sides, O(N^2 S), plus Phi(X) w on the evaluation kernel.
 *   bohip_paths_eval     values (S x R row-major: path s at values[s*R + j], nullable) and best (S records, nullable): arg-max_j
 *                        f_s(x_j) under bohip_gp_score's rule (strict '>' from -Inf, ties -> smallest j, NaN never wins).  Xs is d x R
 *                        column-major, walked in chunks: R is bounded only by the memory of the S x R result when it is asked for.
 *                        Two kernels: row form below BOHIP_PATH_MFMA_MIN paths (environment, read at every draw; default 24), FP64 MFMA
 *                        tiles (128 candidates x 64 paths) from there.  Within one form a value depends on neither S nor R nor on what
 *                        else was in the call, bit for bit; the two forms agree to rounding.  The coefficients never depend on the form.
 *   bohip_paths_eval_grad  f (R) and grad (d x R column-major) of ONE path per point: point j on path path_of[j] (NULL: path 0).
 *                        One workgroup per point; meant for tens to thousands of ascent iterates.  No limit on R or R d (chunked).
 *                        Matérn 1/2: bohip.h's rule at rho = 0 (that observation contributes 0).
 *   bohip_paths_coef     one path's numbers for tests: omega (F x d row-major), w (M), u (N); each nullable.
 * BOHIP_E_ARG: S < 1, M < 2, M odd or not a multiple of 16, R < 1, a path_of entry outside [0, S), s outside [0, S), null
 * pointers; BOHIP_E_STATE: no observations; BOHIP_E_UNSUPPORTED: S > BOHIP_PATHS_S_MAX or M > BOHIP_PATHS_M_MAX (the text names
 * the limit).  Memory of an object: S x (N + M) doubles; the draw needs 2 S N doubles more while it runs.                       */
#define BOHIP_PATHS_S_MAX 4096
#define BOHIP_PATHS_M_MAX 16384
int bohip_gp_paths_draw(bohip_gp *gp, int64_t S, int64_t M, uint64_t seed, bohip_paths **out);
void bohip_paths_destroy(bohip_paths *paths);
int bohip_paths_dims(const bohip_paths *paths, int64_t *S, int64_t *M, int64_t *N, int64_t *d);
int bohip_paths_eval(bohip_paths *paths, const double *Xs, int64_t R, double *values, bohip_best *best);
int bohip_paths_eval_grad(bohip_paths *paths, const double *Xs, int64_t R, const int64_t *path_of, double *f, double *grad);
int bohip_paths_coef(const bohip_paths *paths, int64_t s, double *omega, double *w, double *u);

#ifdef __cplusplus
}
#endif
#endif /* BOHIP_PATHS_H */
