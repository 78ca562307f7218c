// kernels_nei.hip -- noisy expected improvement (include/bohip_nei.h): EI, PI and LogEI averaged over posterior draws of
// the noise-free function values at the observed sites (Letham, Karrer, Ottoni & Bakshy 2019, eq. 6).  Every draw supplies its own
// incumbent tau_s and its own noise-free conditional mean; the variance is shared (the companion's ordinary posterior pass), so S
// fantasies cost one R x N x S contraction, not S refits.  The fantasies are S1 = max(S, 1) rows of [rows][ld] matrices (columns >= N
// stay zero); the five N x N x S triangular products between the stages below are k_gemm_nt launches (bohip.hip, ensure_nei_fantasies).
//   k_nei_normals  Z[s][i] = thompson_normal(seed, 2 s, i)                                  (the operand of G = Z L_d')
//   k_nei_resid    R[s][i] = ((y_i - beta) - G[s][i]) - sqrt(nu_i) thompson_normal(seed, 2 s + 1, i)
//   k_nei_mask     columns >= N of a product's output back to zero (row N of the resident W holds alpha: bohip.hip compute_alpha)
//   k_nei_fant     H = R - nu_i Q (Q = A^-1 R),  F = ((beta + G) + R) - nu_i Q
//   k_nei_tau      tau_s = max_i F[s][i], one workgroup a fantasy
//   k_nei_t2       T2 = z + P (P = W_d H): W_d (g + h) with W_d g = z taken exactly
//   k_nei_means    MT[s][r] = beta + sum_n K*'[r][n] alpha_s[n]: v_mfma_f64_4x4x4 on the LDS-DMA tile loop of gemm_core.h, 128 candidates x
//                  64 fantasies a workgroup and slice of the contraction, the tile leaves through LDS fantasy-major so that
//                  k_nei_reduce reads it coalesced
//   k_nei_reduce   thread = candidate: the S1 fantasies in ascending order with acq_eval (kernels_score.hip; acq_log.h for LogEI), the mean
//                  of m_s, per-block arg-max records for k_argmax_final.  No atomics: every sum has one writer and a fixed order.
// Included by bohip.hip after kernels_score.hip (AcqParams, acq_eval, block_argmax, thompson_normal).
#pragma once
#include "common.h"
#include "gemm_core.h"

namespace bohip {

constexpr int NEI_SMAX = 1024;          // BOHIP_NEI_SMAX
constexpr int NEI_RED_THREADS = 128;    // a K*' chunk starts at a multiple of 128 candidates: a workgroup never straddles two chunks

__global__ __launch_bounds__(256) void k_nei_normals(double* __restrict__ Z, int64_t ld, int64_t N, int S, unsigned long long seed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i < N && s < S) Z[(int64_t)s * ld + i] = thompson_normal(seed, 2 * (int64_t)s, i);
}

// invr: 1 / r_i of a weighted handle, null otherwise; zero_e: S = 0, the plug-in form
__global__ __launch_bounds__(256) void k_nei_resid(const double* __restrict__ y, double beta, const double* __restrict__ G, int64_t ld,
                                                   int64_t N, int zero_e, unsigned long long seed, double nu,
                                                   const double* __restrict__ invr, double* __restrict__ Rm) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= N) return;
    const double nui = invr ? nu * invr[i] : nu;
    const double e = zero_e ? 0.0 : thompson_normal(seed, 2 * (int64_t)s + 1, i);
    Rm[(int64_t)s * ld + i] = ((y[i] - beta) - G[(int64_t)s * ld + i]) - sqrt(nui) * e;
}

__global__ __launch_bounds__(256) void k_nei_mask(double* __restrict__ A, int64_t ld, int64_t N, int64_t Npad) {
    const int64_t i = N + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < Npad) A[(int64_t)blockIdx.y * ld + i] = 0.0;
}

__global__ __launch_bounds__(256) void k_nei_fant(const double* __restrict__ G, const double* __restrict__ Q, int64_t ld, int64_t N,
                                                  double beta, double nu, const double* __restrict__ invr, double* __restrict__ RH,
                                                  double* __restrict__ F) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t o = (int64_t)blockIdx.y * ld + i;
    if (i >= N) return;
    const double nui = invr ? nu * invr[i] : nu;
    const double r = RH[o], dq = nui * Q[o];
    F[o] = ((beta + G[o]) + r) - dq;
    RH[o] = r - dq;
}

__global__ __launch_bounds__(256) void k_nei_tau(const double* __restrict__ F, int64_t ld, int64_t N, double* __restrict__ tau) {
    __shared__ double red[256];
    const double* f = F + (int64_t)blockIdx.x * ld;
    double m = -INFINITY;
    bool nan = false;
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const double v = f[i];
        nan = nan || v != v;
        if (v > m) m = v;
    }
    red[threadIdx.x] = nan ? NAN : m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const double a = red[threadIdx.x], b = red[threadIdx.x + o];
            red[threadIdx.x] = (a != a || b != b) ? NAN : (b > a ? b : a);   // a NaN sticks
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) tau[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_nei_t2(const double* __restrict__ P, int64_t ld, int64_t N, int64_t Npad, int zero_z,
                                                unsigned long long seed, double* __restrict__ T2) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= Npad) return;
    double v = 0.0;
    if (i < N) v = (zero_z ? 0.0 : thompson_normal(seed, 2 * (int64_t)s, i)) + P[(int64_t)s * ld + i];
    T2[(int64_t)s * ld + i] = v;
}

// MT_z[tj 64 + c][ti 128 + r] = [z == 0] beta + sum over slice z of n of A[ti 128 + r][n] B[tj 64 + c][n]:  A = the K*' chunk
// (candidate-major, K-major rows), B = alpha_s rows.  The contraction is cut into slices of kz 16-deep steps (blockIdx.y; a function
// of the row tiles alone, bohip.hip) so that 4096 candidates x 64 fantasies are 256 workgroups, not 32; every slice writes a plane of
// its own and k_nei_reduce adds the planes in ascending order: a candidate's means depend neither on its row nor on its batch.
struct NeiMeans {
    const double* A;   // [mt 128][lda]
    const double* B;   // [nt 64][ldb]
    double* MT;        // [slices][nt 64][ldm], `plane` doubles apart
    int64_t lda, ldb, ldm, plane;
    int mt, nt, kc, kz;   // 128-candidate tiles, 64-fantasy tiles, 16-deep chunks of the whole contraction and of one slice
    double beta;
};
__global__ __launch_bounds__(GEMM_THREADS_8, 2) void k_nei_means(NeiMeans p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int ti = (int)blockIdx.x / p.nt, tj = (int)blockIdx.x % p.nt, z = (int)blockIdx.y;
    const int kb = z * p.kz, ke = min(p.kc, kb + p.kz);   // (never empty: the grid has ceil(kc / kz) slices)
    const double beta = z == 0 ? p.beta : 0.0;
    double acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    gemm_tile_loop_glds3_ks<4>(p.A + (int64_t)ti * TILE * p.lda, p.lda, p.B + (int64_t)tj * CTILE * p.ldb, p.ldb, kb, ke, smem, acc);
    const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6), wr = (wave & 3) >> 1, wc = wave & 1;
    constexpr int TS = CTILE + 2;
    double* Tl = smem;   // [128][66]: the staging buffers are free (the loop ended on a barrier)
    if (wave < 4) {
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) Tl[acc_row(lane, wr, mi) * TS + acc_col<4>(lane, wc, nj)] = beta + acc[mi][nj];
    }
    __syncthreads();
    double* out = p.MT + (int64_t)z * p.plane + (int64_t)tj * CTILE * p.ldm + (int64_t)ti * TILE;
#pragma unroll
    for (int u = 0; u < (TILE * CTILE / 2) / GEMM_THREADS_8; ++u) {
        const int piece = threadIdx.x + GEMM_THREADS_8 * u, c = piece >> 6, r = (piece & 63) * 2;
        d2 v;
        v.x = Tl[r * TS + c];
        v.y = Tl[(r + 1) * TS + c];
        *reinterpret_cast<d2*>(out + (int64_t)c * p.ldm + r) = v;
    }
}

struct NeiReduce {
    const double* MT;       // [nsl][S1 ..][ldm] the planes of m_s of the chunk's candidates (`plane` doubles apart), column 0 = candidate r0
    const double* var;      // [R] s^2 (absolute candidate index)
    const double* tau;      // [S1]
    int64_t ldm, plane, r0, r1;
    int S1, nsl;
    AcqParams ap;
    double *score_out, *mu_out;   // [R], nullable
    Best* block_best;             // nullable: [blocks of the whole call], this launch writes from r0 / NEI_RED_THREADS on
};
__global__ __launch_bounds__(NEI_RED_THREADS) void k_nei_reduce(NeiReduce a) {
#pragma clang fp contract(off)
    __shared__ double tl[NEI_SMAX];
    __shared__ Best sh[4];
    for (int e = threadIdx.x; e < a.S1; e += NEI_RED_THREADS) tl[e] = a.tau[e];
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * NEI_RED_THREADS + threadIdx.x, r = a.r0 + c;
    const bool live = r < a.r1;
    const bool lme = a.ap.acq == ACQ_LOGEI;     // log-mean-exp: pass 0 finds the largest value, pass 1 sums exp(v - max)
    double f = -INFINITY;
    long long idx = -1;
    if (live) {
        const double s2 = a.var[r];
        double vmax = -INFINITY, sum = 0.0, msum = 0.0;
        for (int pass = lme ? 0 : 1; pass < 2; ++pass)
            for (int s = 0; s < a.S1; ++s) {
                double m = a.MT[(int64_t)s * a.ldm + c];
                for (int z = 1; z < a.nsl; ++z) m = m + a.MT[z * a.plane + (int64_t)s * a.ldm + c];
                if (pass == 1) msum = msum + m;
                AcqParams ap = a.ap;
                ap.p0 = tl[s];
                const double v = acq_eval(ap, m, s2);
                if (!lme) sum = sum + v;
                else if (pass == 0) vmax = (v > vmax || v != v) ? v : vmax;   // a NaN sticks
                else sum = sum + (v == vmax ? 1.0 : exp(v - vmax));           // (v == vmax: also the case -Inf - -Inf)
            }
        double val;
        if (!lme) val = sum / (double)a.S1;
        else val = vmax == -INFINITY ? -INFINITY : vmax + log(sum / (double)a.S1);
        if (a.score_out) a.score_out[r] = val;
        if (a.mu_out) a.mu_out[r] = msum / (double)a.S1;
        if (val > -INFINITY) { f = val; idx = r; }   // false for NaN and -Inf
    }
    if (a.block_best) {
        block_argmax(f, idx, sh);
        if (threadIdx.x == 0) {
            Best* o = a.block_best + a.r0 / NEI_RED_THREADS + blockIdx.x;
            o->val = idx >= 0 ? f : -INFINITY;
            o->idx = idx;
        }
    }
}

}  // namespace bohip
