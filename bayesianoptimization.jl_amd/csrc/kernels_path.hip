// kernels_path.hip -- posterior SAMPLE PATHS (pathwise conditioning, Matheron's rule with a random-feature prior): S draws of the
// posterior that are FUNCTIONS, evaluated at any point after the draw (bohip_paths in include/bohip_paths.h):
//     f_s(x) = beta + sum_m w_sm phi_m(x) + sum_j u_sj k(x, X_j),      u_s = K^-1 (y - beta - Phi(X) w_s - eps_s)
//     phi_2m = sqrt(sigma2 / F) cos(omega_m . x),  phi_2m+1 = sqrt(sigma2 / F) sin(omega_m . x),  F = M / 2
// The coefficient matrix Cf[S][ldc] = (u_s, zero-padded to Npad | w_s) keeps the contraction index contiguous, so one evaluation
// is ONE contraction V[s][j] = sum_c Cf[s][c] b_c(x_j) against a basis panel that exists only in LDS:
//   k_path_omega   the F frequencies (Gaussian for SE, multivariate t with 2 nu degrees of freedom for Matérn nu)
//   k_path_w       the M prior weights of every path, straight into Cf
//   k_path_rhs     y - beta - Phi(X) w_s - eps_s from the feature values of the observations
//   k_path_pack    u_s into Cf
//   k_path_rows    few paths: 8 candidates per workgroup, every thread owns a contraction index per chunk of 256 and keeps
//                  8 x SD running sums in registers (no MFMA); one pass over X and Omega per group of SD paths
//   k_path_mfma    many paths: 128 candidates x 64 paths per workgroup on v_mfma_f64_4x4x4 (k_sample_mfma's tiling); per chunk of
//                  KC = 16 contraction indices the 128 x 16 basis panel is generated into LDS (one exp per kernel entry, one sincos
//                  per frequency = two entries) and 64 x 16 of Cf is read K-major
//   k_path_best    per-(path, candidate tile) arg-max records -> best[s], carried over the chunks of one call
//   k_path_grad    value and gradient of ONE path per point, one workgroup per point
// Both evaluation kernels add the terms of one (path, candidate) pair in an order that depends on neither S nor R nor the chunking
// of R: thread-owned partial sums in chunk order, then a fixed reduction tree (rows); chunk order inside the MFMA accumulator
// (mfma).  So a value does not depend on what else was in the call, bit for bit, within one form.
#include "gemm_core.h"   // (mfma444; `better`, thompson_normal and cov_from_r_fast come from kernels_score.hip, included before)

namespace bohip {

constexpr int PR_CAND = 8;     // candidates per workgroup of k_path_rows
constexpr int PM_ROWS = 128;   // k_path_mfma: candidates x paths per workgroup
constexpr int PM_PATHS = 64;
constexpr int PM_LD = KC + 1;
constexpr int PG_DIMS = 8;     // k_path_grad: gradient components per pass over the basis

struct PathLen { double inv[DMAX]; };   // exp(-loglen_k)

// What an evaluation needs of a paths object (all device pointers are the object's own copies)
struct PathArgs {
    const double* X;    // [N][d]
    const double* Om;   // [F][d]
    const double* Cf;   // [S][ldc]: u (N, zeros up to Npad) | w (M)
    int64_t N, Npad, ldc, S;
    int F;
    double amp, beta;   // sqrt(sigma2 / F), the constant mean
};

// dof = 2 nu of the family's spectral density (0: Gaussian)
__host__ __device__ inline int path_family_dof(int fam) { return fam == FAM_M12 ? 1 : fam == FAM_M32 ? 3 : fam == FAM_M52 ? 5 : 0; }

// omega_mk = z_mk exp(-loglen_k) t_m;  z_mk = normal(seed, -1 - m, k);  t_m = 1 (SE) or 1 / sqrt(chi2_m / n) with
// chi2_m = sum_{i < n} normal(seed, -1 - m, d + i)^2, n = 2 nu.  Keys with a negative stream belong to the basis alone.
__global__ __launch_bounds__(256) void k_path_omega(uint64_t seed, int F, int d, int dof, PathLen len, double* __restrict__ Om) {
#pragma clang fp contract(off)
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= F) return;
    double t = 1.0;
    if (dof > 0) {
        double chi2 = 0.0;
        for (int i = 0; i < dof; ++i) {
            const double z = thompson_normal(seed, -1 - (int64_t)m, d + i);
            chi2 += z * z;
        }
        t = 1.0 / sqrt(chi2 / (double)dof);
    }
    for (int k = 0; k < d; ++k) Om[(int64_t)m * d + k] = thompson_normal(seed, -1 - (int64_t)m, k) * len.inv[k] * t;
}

// w_sm = normal(seed, s, m), m < M
__global__ __launch_bounds__(256) void k_path_w(uint64_t seed, int64_t M, double* __restrict__ Cf, int64_t ldc, int64_t Npad) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (m < M) Cf[s * ldc + Npad + m] = thompson_normal(seed, s, m);
}

// T[s][i] <- (y_i - beta) - T[s][i] - sqrt(noise) normal(seed, s, M + i)      (T holds Phi(X) w_s on entry)
__global__ __launch_bounds__(256) void k_path_rhs(uint64_t seed, int64_t M, int64_t N, const double* __restrict__ y, double beta,
                                                  double noise_sd, double* __restrict__ T, int64_t ldt) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (i < N) T[s * ldt + i] = ((y[i] - beta) - T[s * ldt + i]) - noise_sd * thompson_normal(seed, s, M + i);
}

__global__ __launch_bounds__(256) void k_path_pack(const double* __restrict__ U, int64_t ldu, int64_t N, double* __restrict__ Cf,
                                                   int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (i < N) Cf[s * ldc + i] = U[s * ldu + i];
}

// fx = 2 dk/dr of common.h, for every family (the expressions of k_grad_rows)
template <bool LOW>
__device__ __forceinline__ double path_fx(int fam, double sigma2, double rr) {
    if constexpr (LOW) {
        return matern_lo_fx(fam, sigma2, rr);
    } else {
        if (fam == FAM_M52) {
            const double s = sqrt(5.0) * sqrt(rr);
            return -(5.0 / 3.0) * sigma2 * (1.0 + s) * exp(-s);
        }
        return -(sigma2 * exp(-0.5 * rr));
    }
}

// ------------------------------------------------------------------------------------------------
// Few paths.  Workgroup = PR_CAND candidates x SD paths.  Chunks of 256 contraction indices, kernel part first, then the
// frequencies; thread t owns index c0 + t of every chunk, so X, Omega and Cf are read once per workgroup, coalesced.
// Xs: this launch's candidates [R][d]; values[s * ldv + j] (nullable); part[s * ntiles + tile] (nullable) with the GLOBAL
// candidate index j_off + j.  feat_only: the prior term alone, without beta (the draw's right-hand sides).
// ------------------------------------------------------------------------------------------------
template <int SD, bool LOW>
__global__ __launch_bounds__(256) void k_path_rows(PathArgs p, KernelHyper hp, const double* __restrict__ Xs, int64_t R,
                                                   int64_t j_off, double* __restrict__ values, int64_t ldv,
                                                   Best* __restrict__ part, int ntiles, int feat_only) {
    __shared__ double x_l[PR_CAND][DMAX];
    __shared__ double red_l[4][PR_CAND * SD];
    __shared__ double f_l[SD][PR_CAND];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = hp.d;
    const int64_t j0 = (int64_t)blockIdx.x * PR_CAND, s0 = (int64_t)blockIdx.y * SD;
    for (int e = tid; e < PR_CAND * d; e += 256) {
        const int i = e / d, k = e % d;
        x_l[i][k] = (j0 + i < R) ? Xs[(j0 + i) * d + k] : 0.0;
    }
    __syncthreads();
    double acc[PR_CAND][SD];
#pragma unroll
    for (int i = 0; i < PR_CAND; ++i)
#pragma unroll
        for (int sd = 0; sd < SD; ++sd) acc[i][sd] = 0.0;
    if (!feat_only) {
        for (int64_t c0 = 0; c0 < p.N; c0 += 256) {
            const int64_t c = c0 + tid;
            const bool ok = c < p.N;
            const double* xc = p.X + (ok ? c : p.N - 1) * d;
            double rr[PR_CAND];
#pragma unroll
            for (int i = 0; i < PR_CAND; ++i) rr[i] = 0.0;
            for (int k = 0; k < d; ++k) {
                const double xk = xc[k], w = hp.il2[k];
#pragma unroll
                for (int i = 0; i < PR_CAND; ++i) {
                    const double t = x_l[i][k] - xk;
                    rr[i] += w * (t * t);
                }
            }
            double cf[SD];
#pragma unroll
            for (int sd = 0; sd < SD; ++sd) cf[sd] = (ok && s0 + sd < p.S) ? p.Cf[(s0 + sd) * p.ldc + c] : 0.0;
#pragma unroll
            for (int i = 0; i < PR_CAND; ++i) {
                const double b = cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr[i]);
#pragma unroll
                for (int sd = 0; sd < SD; ++sd) acc[i][sd] += cf[sd] * b;
            }
        }
    }
    for (int m0 = 0; m0 < p.F; m0 += 256) {
        const int m = m0 + tid;
        const bool ok = m < p.F;
        const double* om = p.Om + (int64_t)(ok ? m : p.F - 1) * d;
        double ph[PR_CAND];
#pragma unroll
        for (int i = 0; i < PR_CAND; ++i) ph[i] = 0.0;
        for (int k = 0; k < d; ++k) {
            const double o = om[k];
#pragma unroll
            for (int i = 0; i < PR_CAND; ++i) ph[i] += o * x_l[i][k];
        }
        double cw[SD], sw[SD];
#pragma unroll
        for (int sd = 0; sd < SD; ++sd) {
            const bool live = ok && s0 + sd < p.S;
            const double* w = p.Cf + (s0 + sd) * p.ldc + p.Npad + 2 * (int64_t)m;
            cw[sd] = live ? w[0] : 0.0;
            sw[sd] = live ? w[1] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < PR_CAND; ++i) {
            double sn, cs;
            sincos(ph[i], &sn, &cs);
            sn *= p.amp;
            cs *= p.amp;
#pragma unroll
            for (int sd = 0; sd < SD; ++sd) {
                acc[i][sd] += cw[sd] * cs;
                acc[i][sd] += sw[sd] * sn;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PR_CAND; ++i)
#pragma unroll
        for (int sd = 0; sd < SD; ++sd) {
            double v = acc[i][sd];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) red_l[wave][i * SD + sd] = v;
        }
    __syncthreads();
    if (tid < PR_CAND * SD) {
        const int i = tid / SD, sd = tid % SD;
        const int64_t j = j0 + i, s = s0 + sd;
        const double f = (feat_only ? 0.0 : p.beta) + (((red_l[0][tid] + red_l[1][tid]) + red_l[2][tid]) + red_l[3][tid]);
        f_l[sd][i] = f;
        if (values && j < R && s < p.S) values[s * ldv + j] = f;
    }
    __syncthreads();
    if (part && tid < SD && s0 + tid < p.S) {
        double v = -INFINITY;
        long long idx = -1;
        for (int i = 0; i < PR_CAND && j0 + i < R; ++i)
            if (better(f_l[tid][i], j_off + j0 + i, v, idx)) { v = f_l[tid][i]; idx = j_off + j0 + i; }
        part[(s0 + tid) * ntiles + blockIdx.x] = Best{idx >= 0 ? v : -INFINITY, idx};
    }
}

// ------------------------------------------------------------------------------------------------
// Many paths.  V tile = B[128 candidates][c] Cf'[c][64 paths]; 4 waves in 2 x 2, wave tile 64 x 32 = 8 x 4 groups of 8 x 8
// (32 accumulators per lane), lane layout of mfma444 as in k_sample_mfma.  Dynamic LDS: a_l[128][17] basis panel,
// b_l[64][17] coefficients, x_l[128][d | 1] the tile's candidates, c_l[16][d] the chunk's observations / 8 frequencies.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t path_mfma_lds_bytes(int d) {
    return (size_t)(PM_ROWS * PM_LD + PM_PATHS * PM_LD + PM_ROWS * (d | 1) + KC * d) * sizeof(double);
}
template <bool LOW>
__global__ __launch_bounds__(256) void k_path_mfma(PathArgs p, KernelHyper hp, const double* __restrict__ Xs, int64_t R,
                                                   int64_t j_off, double* __restrict__ values, int64_t ldv,
                                                   Best* __restrict__ part, int ntiles, int feat_only) {
    extern __shared__ __attribute__((aligned(16))) double pm_lds[];
    __shared__ Best rec_l[2][PM_PATHS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = hp.d, dl = d | 1;
    double* a_l = pm_lds;
    double* b_l = a_l + PM_ROWS * PM_LD;
    double* x_l = b_l + PM_PATHS * PM_LD;
    double* c_l = x_l + PM_ROWS * dl;
    const int64_t j0 = (int64_t)blockIdx.x * PM_ROWS, s0 = (int64_t)blockIdx.y * PM_PATHS;
    const int wr = wave >> 1, wc = wave & 1;
    const int kq = lane >> 4, bb = (lane >> 2) & 3, t = lane & 3;
    const int ar = 4 * (bb >> 1) + t, bc = 4 * (bb & 1) + t;
    const int dr = 4 * (bb >> 1) + (lane >> 4), dc = 4 * (bb & 1) + (lane & 3);
    const int row = tid >> 1, half = tid & 1;
    for (int e = tid; e < PM_ROWS * d; e += 256) {
        const int i = e / d, k = e % d;
        x_l[i * dl + k] = (j0 + i < R) ? Xs[(j0 + i) * d + k] : 0.0;
    }
    double acc[8][4];
#pragma unroll
    for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int h = 0; h < 4; ++h) acc[g][h] = 0.0;
    const int64_t nk = feat_only ? 0 : p.Npad / KC, nchunks = nk + p.F / (KC / 2);
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        const bool feat = ch >= nk;
        const int64_t k0 = feat ? (ch - nk) * (KC / 2) : ch * KC;       // first observation / first frequency of the chunk
        const int64_t cf0 = feat ? p.Npad + 2 * k0 : k0;                // first column of Cf
        __syncthreads();
        if (feat) {
            for (int e = tid; e < (KC / 2) * d; e += 256) c_l[e] = p.Om[k0 * d + e];
        } else {
            for (int e = tid; e < KC * d; e += 256) c_l[e] = (k0 + e / d < p.N) ? p.X[k0 * d + e] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < PM_PATHS * KC / 256; ++q) {
            const int e = tid + 256 * q, si = e >> 4, kk = e & 15;
            b_l[si * PM_LD + kk] = (s0 + si < p.S) ? p.Cf[(s0 + si) * p.ldc + cf0 + kk] : 0.0;
        }
        __syncthreads();
        const double* xr = x_l + row * dl;
        if (feat) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int mm = 4 * half + e;
                double ph = 0.0;
                for (int k = 0; k < d; ++k) ph += c_l[mm * d + k] * xr[k];
                double sn, cs;
                sincos(ph, &sn, &cs);
                a_l[row * PM_LD + 2 * mm] = p.amp * cs;
                a_l[row * PM_LD + 2 * mm + 1] = p.amp * sn;
            }
        } else {
            double rr[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) rr[e] = 0.0;
            for (int k = 0; k < d; ++k) {
                const double xk = xr[k], w = hp.il2[k];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const double tt = xk - c_l[(8 * half + e) * d + k];
                    rr[e] += w * (tt * tt);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)
                a_l[row * PM_LD + 8 * half + e] = (k0 + 8 * half + e < p.N) ? cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr[e]) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {
            const int kk = 4 * ks + kq;
            double av[8], bv[4];
#pragma unroll
            for (int g = 0; g < 8; ++g) av[g] = a_l[(64 * wr + 8 * g + ar) * PM_LD + kk];
#pragma unroll
            for (int h = 0; h < 4; ++h) bv[h] = b_l[(32 * wc + 8 * h + bc) * PM_LD + kk];
#pragma unroll
            for (int g = 0; g < 8; ++g)
#pragma unroll
                for (int h = 0; h < 4; ++h) acc[g][h] = mfma444(av[g], bv[h], acc[g][h]);
        }
    }
    // epilogue: beta, the S x R result when asked for, and the tile's arg-max per path (rows ascending inside a lane, then the
    // lanes that hold the same path: bits 3, 4, 5 of the lane number)
    const double beta = feat_only ? 0.0 : p.beta;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int64_t s = s0 + 32 * wc + 8 * h + dc;
        double v = -INFINITY;
        long long idx = -1;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int64_t j = j0 + 64 * wr + 8 * g + dr;
            if (j < R && s < p.S) {
                const double f = beta + acc[g][h];
                if (values) values[s * ldv + j] = f;
                if (better(f, j_off + j, v, idx)) { v = f; idx = j_off + j; }
            }
        }
        for (int o = 8; o <= 32; o <<= 1) {
            const double ov = __shfl_xor(v, o);
            const long long oi = __shfl_xor(idx, o);
            if (better(ov, oi, v, idx)) { v = ov; idx = oi; }
        }
        if (lane < 8) rec_l[wr][32 * wc + 8 * h + lane] = Best{v, idx};
    }
    __syncthreads();
    if (part && tid < PM_PATHS && s0 + tid < p.S) {
        double v = rec_l[0][tid].val;
        long long idx = rec_l[0][tid].idx;
        if (better(rec_l[1][tid].val, rec_l[1][tid].idx, v, idx)) { v = rec_l[1][tid].val; idx = rec_l[1][tid].idx; }
        part[(s0 + tid) * ntiles + blockIdx.x] = Best{idx >= 0 ? v : -INFINITY, idx};
    }
}

// one wave per path: the tile records of one chunk of candidates in tile order, folded onto the record of the chunks before it
// (carry != 0) under (value desc, index asc)
__global__ __launch_bounds__(64) void k_path_best(const Best* __restrict__ part, int ntiles, Best* __restrict__ out, int carry) {
    const int64_t s = blockIdx.x;
    double v = -INFINITY;
    long long idx = -1;
    for (int t = threadIdx.x; t < ntiles; t += 64) {
        const Best b = part[s * ntiles + t];
        if (better(b.val, b.idx, v, idx)) { v = b.val; idx = b.idx; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const long long oi = __shfl_xor(idx, o);
        if (better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
    if (threadIdx.x == 0) {
        if (carry) {
            const Best b = out[s];
            if (better(b.val, b.idx, v, idx)) { v = b.val; idx = b.idx; }
        }
        out[s] = Best{idx >= 0 ? v : -INFINITY, idx >= 0 ? idx : -1};
    }
}

// ------------------------------------------------------------------------------------------------
// Value and gradient of path path_of[j] (NULL: path 0) at point j; one workgroup per point, PG_DIMS gradient components per pass
// over the observations and the frequencies (d <= 8: one pass).
//   df/dx_k = sum_j u_j fx(r_j) (x_k - X_jk) il2_k + sum_m amp omega_mk (-w_2m sin(omega_m . x) + w_2m+1 cos(omega_m . x))
// ------------------------------------------------------------------------------------------------
template <bool LOW>
__global__ __launch_bounds__(256) void k_path_grad(PathArgs p, KernelHyper hp, const double* __restrict__ Xs, int64_t R,
                                                   const int64_t* __restrict__ path_of, double* __restrict__ f,
                                                   double* __restrict__ grad) {
    __shared__ double x_l[DMAX];
    __shared__ double red_l[4][PG_DIMS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = hp.d;
    const int64_t j = blockIdx.x;
    if (j >= R) return;
    const int64_t s = path_of ? path_of[j] : 0;
    const double* cf = p.Cf + s * p.ldc;
    if (tid < d) x_l[tid] = Xs[j * d + tid];
    __syncthreads();
    for (int kb = 0; kb < d; kb += PG_DIMS) {
        double g[PG_DIMS], fv = 0.0;
#pragma unroll
        for (int kk = 0; kk < PG_DIMS; ++kk) g[kk] = 0.0;
        for (int64_t c = tid; c < p.N; c += 256) {
            const double* xc = p.X + c * d;
            double rr = 0.0;
            for (int k = 0; k < d; ++k) {
                const double t = x_l[k] - xc[k];
                rr += hp.il2[k] * (t * t);
            }
            const double u = cf[c];
            if (kb == 0) fv += u * cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr);
            const double q = u * path_fx<LOW>(hp.fam, hp.sigma2, rr);
#pragma unroll
            for (int kk = 0; kk < PG_DIMS; ++kk)
                if (kb + kk < d) g[kk] += q * ((x_l[kb + kk] - xc[kb + kk]) * hp.il2[kb + kk]);
        }
        for (int m = tid; m < p.F; m += 256) {
            const double* om = p.Om + (int64_t)m * d;
            double ph = 0.0;
            for (int k = 0; k < d; ++k) ph += om[k] * x_l[k];
            double sn, cs;
            sincos(ph, &sn, &cs);
            const double cw = cf[p.Npad + 2 * (int64_t)m], sw = cf[p.Npad + 2 * (int64_t)m + 1];
            if (kb == 0) {
                fv += cw * (p.amp * cs);
                fv += sw * (p.amp * sn);
            }
            const double q = p.amp * (sw * cs - cw * sn);
#pragma unroll
            for (int kk = 0; kk < PG_DIMS; ++kk)
                if (kb + kk < d) g[kk] += q * om[kb + kk];
        }
#pragma unroll
        for (int kk = 0; kk <= PG_DIMS; ++kk) {
            double v = kk < PG_DIMS ? g[kk < PG_DIMS ? kk : 0] : fv;
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) red_l[wave][kk] = v;
        }
        __syncthreads();
        if (tid <= PG_DIMS) {
            const double v = ((red_l[0][tid] + red_l[1][tid]) + red_l[2][tid]) + red_l[3][tid];
            if (tid < PG_DIMS) {
                if (kb + tid < d) grad[j * d + kb + tid] = v;
            } else if (kb == 0) {
                f[j] = p.beta + v;
            }
        }
        __syncthreads();
    }
}

}  // namespace bohip
