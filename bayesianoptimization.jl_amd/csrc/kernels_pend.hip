// kernels_pend.hip -- pending evaluations (include/bohip_pend.h): the acquisition averaged over fantasised outcomes at
// points that are out for evaluation (Snoek, Larochelle & Adams 2012, section 3.2).  Only the MEAN of the conditioned posterior
// depends on the fantasy:  mu_s(x) = mu(x) + b(x)' z_s,  s^2(x) = sigma^2(x) - |b(x)|^2,  b(x) = L_p^-1 (k(x, Xp) - v(x)' V_p),
// so S fantasies are one contraction against the p <= 32 columns of V_p (k_gemm_nt on the stored V' of the chunk, B = V_p' padded
// to one 64-column tile) and a p-term sum per fantasy.  Kernels, in the order a call runs them:
//   k_pend_state   ONE workgroup: Sigma_p = K(Xp, Xp) - V_p' V_p + nu I from the lower triangle of the MFMA product, L_p = chol(Sigma_p)
//                  in LDS, the failed pivot's number in *info (the host turns it into BOHIP_E_NOTPD; no jitter is added)
//   k_pend_tables  thread = fantasy: z_s (bohip_thompson_normal(seed, s, i)), y_f,s = mu_p + L_p z_s and tau_s = max(tau, max_i y_f,s,i)
//   k_pend_cross   thread = candidate of the K*' chunk: c = k(x, Xp) - (V' V_p)[r], the substitution b = L_p^-1 c with L_p in LDS
//   k_pend_score   thread = candidate: s^2, then the S fantasies in ascending order with the Z and tau tables read from LDS in tiles
//                  of fantasies; the functor is acq_eval (kernels_score.hip; acq_log.h for LogEI) -- the code k_score and bohip_acq_eval
//                  run; per-block arg-max records for k_argmax_final.  No atomics: every sum has one writer and a fixed order.
// Included by bohip.hip after kernels_score.hip (AcqParams, acq_eval, block_argmax, cov_from_r_fast, thompson_normal).
#pragma once
#include "common.h"

namespace bohip {

constexpr int PEND_PMAX = 32;          // BOHIP_PEND_PMAX = APPEND_PMAX
constexpr int PEND_SMAX = 1024;        // BOHIP_PEND_SMAX
constexpr int PEND_GLD = CTILE;        // leading dimension of the two MFMA products (one 64-column tile)
constexpr int PEND_ZCAP = 6144;        // doubles of one tile of Z in LDS (48 KB; + 8 KB of tau_s: under the 64 KB every kernel gets)
constexpr int PEND_CROSS_THREADS = 64;
constexpr int PEND_SCORE_THREADS = 64;   // one wave a workgroup: R = 4096 candidates are 64 workgroups, not 16 (the tables are 56 KB: one workgroup a CU either way)
static_assert(PEND_PMAX == APPEND_PMAX, "the pending set is one incremental append");
static_assert(PEND_ZCAP / PEND_PMAX >= 1 && PEND_ZCAP <= PEND_SMAX * PEND_PMAX, "a tile holds at least one fantasy");

// fantasies per LDS tile of k_pend_score (host and device agree on it)
__host__ __device__ inline int pend_tile_fantasies(int p, int S) {
    const int st = PEND_ZCAP / p;
    return st < S ? st : S;
}

template <int DT, bool LOW>
__device__ __forceinline__ double pend_cov(const double (&x)[DT], const double* __restrict__ y, const KernelHyper& hp) {
    double rr = 0.0;
#pragma unroll
    for (int k = 0; k < DT; ++k)
        if (k < hp.d) {
            const double t = x[k] - y[k];
            rr += hp.il2[k] * (t * t);
        }
    return cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr);
}

// Sigma [p][p] (dense, symmetric, nu on the diagonal) and L [p][p] (lower, zeros above) from G = V_p' V_p (PEND_GLD columns a row; the
// lower triangle is read so that Sigma is exactly symmetric).  *info = 0, or 1 + the column whose pivot is not positive.
template <int DT, bool LOW>
__global__ __launch_bounds__(256) void k_pend_state(const double* __restrict__ Xp, int p, KernelHyper hp, double nu,
                                                    const double* __restrict__ G, double* __restrict__ Sigma, double* __restrict__ L,
                                                    int* __restrict__ info) {
#pragma clang fp contract(off)
    __shared__ double S[PEND_PMAX][PEND_PMAX + 1];
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    for (int e = tid; e < p * p; e += 256) {
        const int i = e / p, j = e % p;
        if (j > i) continue;
        double xi[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) xi[k] = k < hp.d ? Xp[i * hp.d + k] : 0.0;
        double v = pend_cov<DT, LOW>(xi, Xp + j * hp.d, hp) - G[i * PEND_GLD + j];
        if (i == j) v += nu;
        S[i][j] = v;
        Sigma[i * p + j] = v;
        Sigma[j * p + i] = v;
    }
    __syncthreads();
    for (int j = 0; j < p; ++j) {      // right-looking, column by column: every entry has one writer per step
        if (tid == 0) {
            const double dj = S[j][j];
            if (!(dj > 0.0) || dj == INFINITY) bad = j + 1;   // (false for NaN too)
            else S[j][j] = sqrt(dj);
        }
        __syncthreads();
        if (bad) break;                // (uniform: read after the barrier)
        const double ljj = S[j][j];
        for (int i = j + 1 + tid; i < p; i += 256) S[i][j] = S[i][j] / ljj;
        __syncthreads();
        const int m = p - j - 1;       // trailing block: rows and columns j + 1 .. p - 1, lower triangle
        for (int e = tid; e < m * m; e += 256) {
            const int i = j + 1 + e / m, k = j + 1 + e % m;
            if (k <= i) S[i][k] = S[i][k] - S[i][j] * S[k][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < p * p; e += 256) {
        const int i = e / p, j = e % p;
        L[i * p + j] = j <= i ? S[i][j] : 0.0;
    }
    if (tid == 0) *info = bad;
}

// Z [S1][p] and tau [S1] of the S1 = max(S, 1) fantasies; S = 0 (zero_z): z = 0, the Kriging believer.  raise: tau_s = max(tau0, max_i
// y_f,s,i), y_f,s = mu_p + L_p z_s summed in ascending column order; otherwise tau_s = tau0.
__global__ __launch_bounds__(64) void k_pend_tables(const double* __restrict__ mu_p, const double* __restrict__ L, int p, int S1, int zero_z,
                                                   unsigned long long seed, double tau0, int raise, double* __restrict__ Z,
                                                   double* __restrict__ tau) {
#pragma clang fp contract(off)
    __shared__ double zl[PEND_PMAX][64];
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S1) return;
    for (int i = 0; i < p; ++i) {
        const double z = zero_z ? 0.0 : thompson_normal(seed, s, i);
        zl[i][threadIdx.x] = z;
        Z[(int64_t)s * p + i] = z;
    }
    double t = tau0;
    if (raise)
        for (int i = 0; i < p; ++i) {
            double y = mu_p[i];
            for (int j = 0; j <= i; ++j) y = y + L[i * p + j] * zl[j][threadIdx.x];
            if (y > t) t = y;
        }
    tau[s] = t;
}

// B[r][0 .. p) = L_p^-1 (k(x_r, Xp) - C[r - r0][0 .. p)) for the candidates r0 <= r < r1 of one K*' chunk; C = V' V_p of the chunk
// (PEND_GLD columns a row, row 0 = candidate r0) arrives as nsl split-K planes, `plane` doubles apart, added here in ascending order.
template <int DT, bool LOW>
__global__ __launch_bounds__(PEND_CROSS_THREADS) void k_pend_cross(const double* __restrict__ Xs, int64_t r0, int64_t r1, KernelHyper hp,
                                                                    const double* __restrict__ Xp, int p, const double* __restrict__ L,
                                                                    const double* __restrict__ C, int nsl, int64_t plane,
                                                                    double* __restrict__ B) {
#pragma clang fp contract(off)
    __shared__ double Ll[PEND_PMAX][PEND_PMAX + 1];
    __shared__ double xp[PEND_PMAX * DT];
    __shared__ double bl[PEND_PMAX][PEND_CROSS_THREADS];
    const int tid = threadIdx.x, d = hp.d;
    for (int e = tid; e < p * p; e += PEND_CROSS_THREADS) Ll[e / p][e % p] = L[e];
    for (int e = tid; e < p * DT; e += PEND_CROSS_THREADS) xp[e] = (e % DT) < d ? Xp[(e / DT) * d + e % DT] : 0.0;
    __syncthreads();
    const int64_t r = r0 + (int64_t)blockIdx.x * PEND_CROSS_THREADS + tid;
    if (r >= r1) return;
    double x[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) x[k] = k < d ? Xs[r * d + k] : 0.0;
    const double* c_row = C + (r - r0) * PEND_GLD;
    for (int i = 0; i < p; ++i) {
        double c = c_row[i];
        for (int z = 1; z < nsl; ++z) c = c + c_row[z * plane + i];
        double b = pend_cov<DT, LOW>(x, xp + i * DT, hp) - c;
        for (int j = 0; j < i; ++j) b = b - Ll[i][j] * bl[j][tid];
        b = b / Ll[i][i];
        bl[i][tid] = b;
        B[r * p + i] = b;
    }
}

struct PendScore {
    const double* mu;       // [R] resident mean
    const double* var;      // [R] sub_bb: the resident sigma^2 (clamped), else s^2 itself
    const double* B;        // [R][p]
    const double* Z;        // [S1][p]
    const double* tau;      // [S1], nullable: ap.p0 for every fantasy
    int64_t R;
    int p, S1, sub_bb, tau_acq;   // tau_acq: the acquisition has an incumbent (EI, PI, LogEI)
    AcqParams ap;
    double *score_out, *var_out;   // nullable
    Best* block_best;              // nullable: [blocks]
};

__global__ __launch_bounds__(PEND_SCORE_THREADS) void k_pend_score(PendScore a) {
#pragma clang fp contract(off)
    __shared__ double zl[PEND_ZCAP];
    __shared__ double tl[PEND_SMAX];
    __shared__ Best sh[4];
    const int64_t r = (int64_t)blockIdx.x * PEND_SCORE_THREADS + threadIdx.x;
    const bool live = r < a.R;
    const int p = a.p;
    double b[PEND_PMAX];
    double mu = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < PEND_PMAX; ++i) b[i] = (live && i < p) ? a.B[r * p + i] : 0.0;
    if (live) {
        mu = a.mu[r];
        s2 = a.var[r];
        if (a.sub_bb) {
            double bb = 0.0;
#pragma unroll
            for (int i = 0; i < PEND_PMAX; ++i)
                if (i < p) bb = bb + b[i] * b[i];
            s2 = s2 - bb;
            if (!(s2 >= 0.0) && s2 == s2) s2 = 0.0;   // max(., 0); a NaN stays a NaN
        }
        if (a.var_out) a.var_out[r] = s2;
    }
    const int ST = pend_tile_fantasies(p, a.S1);
    const bool lme = a.ap.acq == ACQ_LOGEI;     // log-mean-exp: pass 0 finds the largest value, pass 1 sums exp(v - max)
    double vmax = -INFINITY, sum = 0.0;
    for (int pass = lme ? 0 : 1; pass < 2; ++pass) {
        for (int s0 = 0; s0 < a.S1; s0 += ST) {
            const int ns = min(ST, a.S1 - s0);
            __syncthreads();
            for (int e = threadIdx.x; e < ns * p; e += PEND_SCORE_THREADS) zl[e] = a.Z[(int64_t)s0 * p + e];
            for (int e = threadIdx.x; e < ns; e += PEND_SCORE_THREADS) tl[e] = a.tau ? a.tau[s0 + e] : a.ap.p0;
            __syncthreads();
            if (!live) continue;
            for (int s = 0; s < ns; ++s) {
                double m = mu;
#pragma unroll
                for (int i = 0; i < PEND_PMAX; ++i)
                    if (i < p) m = m + b[i] * zl[s * p + i];
                AcqParams ap = a.ap;
                if (a.tau_acq) ap.p0 = tl[s];
                const double v = acq_eval(ap, m, s2);
                if (!lme) sum = sum + v;
                else if (pass == 0) vmax = (v > vmax || v != v) ? v : vmax;   // a NaN sticks
                else sum = sum + (v == vmax ? 1.0 : exp(v - vmax));           // (v == vmax: also the case -Inf - -Inf)
            }
        }
    }
    double f = -INFINITY;
    long long idx = -1;
    double val = NAN;
    if (live) {
        if (!lme) val = sum / (double)a.S1;
        else val = vmax == -INFINITY ? -INFINITY : vmax + log(sum / (double)a.S1);
        if (a.score_out) a.score_out[r] = val;
        if (val > -INFINITY) { f = val; idx = r; }   // false for NaN and -Inf
    }
    if (a.block_best) {
        block_argmax(f, idx, sh);
        if (threadIdx.x == 0) { a.block_best[blockIdx.x].val = idx >= 0 ? f : -INFINITY; a.block_best[blockIdx.x].idx = idx; }
    }
}

}  // namespace bohip
