// kernels_sample.hip -- joint posterior draws over a candidate set (reference: myrand(model, X::Matrix) = rand(gp, X),
// src/models/gp.jl:7), S draws at once:   f_s = mu + C z_s,   C C' = Sigma + jitter I,   z_sk = thompson_normal(seed, s, k).
//   k_sample_cov      Sigma = K** - V'V (k_post_cov's expression) into the kept copy AND into the factor workspace: lower 128-tiles,
//                     zeros above the diagonal of the diagonal tiles, identity in the padding rows (k_build_cov's layout)
//   k_sample_rejit    a retry: the workspace again from the kept Sigma, jitter on the diagonal (no GEMM is repeated)
//   k_sample_diagmax  max_j Sigma_jj, the scale of the jitter
//   k_sample_pack     the factor as a dense R x R lower-triangular matrix for the host
//   k_sample_rows     few draws: one pass over the lower triangle of C in coalesced row panels (bandwidth bound, no MFMA)
//   k_sample_mfma     many draws: 128 candidates x 64 draws per workgroup on v_mfma_f64_4x4x4 (2 x 2 blocks = 8 x 8 x 4 per
//                     instruction, gemm_core.h), contraction cut at the diagonal tile
//   k_sample_best     per-(draw, candidate tile) arg-max records -> best[s]
// z is generated inside the draw kernels (one LDS panel per contraction chunk, shared by the workgroup's candidates) and never
// stored in HBM.  Both draw kernels add the terms of one (candidate, draw) pair in an order that does not depend on S, so a
// call with fewer draws reproduces the leading rows of a call with more, bit for bit, as long as both take the same kernel.
// Where the two forms meet is measured (MI355X, R = 4096, N = 3000, the `sample_draw` stage = draw kernel + k_sample_best, ms;
// tools/time_joint_draw.py --mode forms, profiles/joint_draw_ab.txt):
//     S             1      8      16     64     128    192    256    512    1024
//     k_sample_rows 0.041  0.094  0.128  0.370  0.690  1.010  1.341  2.697  5.634     (linear in S: one pass over C per 4 draws)
//     k_sample_mfma 0.691  0.687  0.689  1.045  1.049  1.045  1.049  1.067  1.712
// so the row-panel kernel serves up to 199 draws and the MFMA kernel takes over from 200 (g_sample_mfma_min in bohip.hip,
// BOHIP_SAMPLE_MFMA_MIN).  The MFMA kernel's floor is not the matrix pipe: a workgroup walks R / 16 chunks in sequence and
// generates 4 normals per thread per chunk (FP64 log, cos, sqrt), about three times the chunk's 128 MFMAs per wave; with 32 row
// tiles x S / 64 draw tiles it fills the chip only from S = 512 on.  At S = 1 the row-panel kernel reads the 67 MB of C in 41 us
// = 1.6 TB/s including the finish kernel (k_batch_cond reaches 4.0 TB/s on its stream).
#include "gemm_core.h"   // (mfma444; `better`, thompson_normal and cov_from_r_fast come from kernels_score.hip, included before)

namespace bohip {

constexpr int SROWS = 16;     // candidates per workgroup of k_sample_rows (R = 4096: 256 workgroups, one per CU)
constexpr int SCH = 256;      // its contraction chunk: every lane reads 4 x 8 B of each of its wave's 4 rows per chunk
constexpr int SM_ROWS = 128;  // k_sample_mfma: candidates x draws per workgroup, contraction chunk KC
constexpr int SM_DRAWS = 64;
constexpr int SM_LD = KC + 1;

template <int DT, bool LOW>
__global__ __launch_bounds__(256) void k_sample_cov(const double* __restrict__ Xs, int64_t R, int64_t Rp, KernelHyper hp,
                                                    const double* __restrict__ VV, int64_t ldv, double* __restrict__ Sig,
                                                    int64_t lds, double* __restrict__ Lw, int64_t ldl) {
    const int d = hp.d;
    const int64_t s = blockIdx.x * 256 + threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * 16, r1 = min(Rp, r0 + 16);
    if (s >= Rp || s / TILE > r0 / TILE) return;   // past the matrix, or a tile above the diagonal tiles (stays zero)
    double xs[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) xs[k] = (k < d && s < R) ? Xs[s * d + k] : 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        if (r < R && s <= r) {
            double rr = 0.0;
#pragma unroll
            for (int k = 0; k < DT; ++k)
                if (k < d) {
                    const double t = Xs[r * d + k] - xs[k];
                    rr += hp.il2[k] * (t * t);
                }
            const double v = cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr) - VV[r * ldv + s];
            Sig[r * lds + s] = v;
            Lw[r * ldl + s] = v;
        } else {
            Lw[r * ldl + s] = (r == s) ? 1.0 : 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void k_sample_rejit(const double* __restrict__ Sig, int64_t lds, int64_t R, int64_t Rp,
                                                      double jitter, double* __restrict__ Lw, int64_t ldl) {
    const int64_t s = blockIdx.x * 256 + threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * 16, r1 = min(Rp, r0 + 16);
    if (s >= Rp || s / TILE > r0 / TILE) return;
    for (int64_t r = r0; r < r1; ++r) {
        double v = (r == s) ? 1.0 : 0.0;
        if (r < R && s <= r) v = Sig[r * lds + s] + (r == s ? jitter : 0.0);
        Lw[r * ldl + s] = v;
    }
}

// out[0] = max(max_j Sigma_jj, DBL_MIN)  (one workgroup; fmax drops a NaN)
__global__ __launch_bounds__(256) void k_sample_diagmax(const double* __restrict__ Sig, int64_t lds, int64_t R,
                                                        double* __restrict__ out) {
    __shared__ double sh[4];
    double m = 2.2250738585072014e-308;
    for (int64_t j = threadIdx.x; j < R; j += 256) m = fmax(m, Sig[j * (lds + 1)]);
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// (the trailing updates of the factorisation write whole diagonal tiles, so what lies above the diagonal of the workspace is
// not the zero the caller is promised: the dense copy masks it)
__global__ __launch_bounds__(256) void k_sample_pack(const double* __restrict__ Lw, int64_t ldl, int64_t R,
                                                     double* __restrict__ out) {
    const int64_t j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j < R) out[i * R + j] = (j <= i) ? Lw[i * ldl + j] : 0.0;
}

// ------------------------------------------------------------------------------------------------
// Few draws.  Workgroup = SROWS candidates x SD draws, heaviest (lowest) row tiles first; wave w owns rows 4w..4w+3 and
// reads them 64 consecutive doubles at a time (512 B per wave load), so C is read exactly once per group of SD draws.
// part[s * ntiles + tile] = the tile's arg-max record of draw s.
// ------------------------------------------------------------------------------------------------
template <int SD>
__global__ __launch_bounds__(256) void k_sample_rows(const double* __restrict__ C, int64_t ld, int64_t R, int64_t S,
                                                     uint64_t seed, const double* __restrict__ mu,
                                                     double* __restrict__ samples, Best* __restrict__ part, int ntiles) {
    __shared__ double z_l[SD][SCH];
    __shared__ double f_l[SD][SROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = ntiles - 1 - (int)blockIdx.x;
    const int64_t j0 = (int64_t)tile * SROWS, s0 = (int64_t)blockIdx.y * SD;
    const int64_t jend = min(R, j0 + SROWS);
    double acc[4][SD];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int sd = 0; sd < SD; ++sd) acc[i][sd] = 0.0;
    for (int64_t k0 = 0; k0 < jend; k0 += SCH) {
        __syncthreads();
#pragma unroll
        for (int sd = 0; sd < SD; ++sd)
            z_l[sd][tid] = (s0 + sd < S && k0 + tid < R) ? thompson_normal(seed, s0 + sd, k0 + tid) : 0.0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t j = j0 + 4 * wave + i;
            double c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t k = k0 + 64 * u + lane;
                c[u] = (j < R && k <= j) ? C[j * ld + k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int sd = 0; sd < SD; ++sd) acc[i][sd] += c[u] * z_l[sd][64 * u + lane];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int sd = 0; sd < SD; ++sd) {
            double v = acc[i][sd];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) f_l[sd][4 * wave + i] = v;
        }
    __syncthreads();
    if (tid < SD * SROWS) {
        const int sd = tid / SROWS, i = tid % SROWS;
        const int64_t j = j0 + i, s = s0 + sd;
        if (j < R && s < S) {
            const double f = mu[j] + f_l[sd][i];
            f_l[sd][i] = f;
            if (samples) samples[s * R + j] = f;
        }
    }
    __syncthreads();
    if (tid < SD && s0 + tid < S) {
        double v = -INFINITY;
        long long idx = -1;
        for (int i = 0; i < SROWS && j0 + i < R; ++i)
            if (better(f_l[tid][i], j0 + i, v, idx)) { v = f_l[tid][i]; idx = j0 + i; }
        part[(s0 + tid) * ntiles + tile] = Best{idx >= 0 ? v : -INFINITY, idx};
    }
}

// ------------------------------------------------------------------------------------------------
// Many draws.  F tile = C[128 candidates][k] Z'[k][64 draws]; 4 waves in 2 x 2, wave tile 64 x 32 = 8 x 4 groups of 8 x 8
// (32 accumulators per lane); the contraction stops at the end of the tile's own diagonal block.  Per chunk of KC contraction
// indices the workgroup stages 128 x 16 of C (masked above the diagonal) and generates 64 x 16 normals into LDS.
// Lane layout of mfma444 as in kernels_linalg.hip's inv_level.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sample_mfma(const double* __restrict__ C, int64_t ld, int64_t R, int64_t S,
                                                     uint64_t seed, const double* __restrict__ mu,
                                                     double* __restrict__ samples, Best* __restrict__ part, int ntiles) {
    __shared__ double a_l[SM_ROWS * SM_LD];
    __shared__ double b_l[SM_DRAWS * SM_LD];
    __shared__ Best rec_l[2][SM_DRAWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = ntiles - 1 - (int)blockIdx.x;
    const int64_t j0 = (int64_t)tile * SM_ROWS, s0 = (int64_t)blockIdx.y * SM_DRAWS;
    const int64_t kend = min(R, j0 + SM_ROWS);
    const int wr = wave >> 1, wc = wave & 1;
    const int kq = lane >> 4, bb = (lane >> 2) & 3, t = lane & 3;
    const int ar = 4 * (bb >> 1) + t, bc = 4 * (bb & 1) + t;
    const int dr = 4 * (bb >> 1) + (lane >> 4), dc = 4 * (bb & 1) + (lane & 3);
    double acc[8][4];
#pragma unroll
    for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int h = 0; h < 4; ++h) acc[g][h] = 0.0;
    for (int64_t k0 = 0; k0 < kend; k0 += KC) {
        __syncthreads();
        {
            const int row = tid >> 1, half = tid & 1;
            const int64_t j = j0 + row;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t k = k0 + 8 * half + e;
                a_l[row * SM_LD + 8 * half + e] = (j < R && k <= j) ? C[j * ld + k] : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < SM_DRAWS * KC / 256; ++q) {
            const int e = tid + 256 * q, si = e >> 4, kk = e & 15;
            b_l[si * SM_LD + kk] = (s0 + si < S && k0 + kk < R) ? thompson_normal(seed, s0 + si, k0 + kk) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {
            const int kk = 4 * ks + kq;
            double av[8], bv[4];
#pragma unroll
            for (int g = 0; g < 8; ++g) av[g] = a_l[(64 * wr + 8 * g + ar) * SM_LD + kk];
#pragma unroll
            for (int h = 0; h < 4; ++h) bv[h] = b_l[(32 * wc + 8 * h + bc) * SM_LD + kk];
#pragma unroll
            for (int g = 0; g < 8; ++g)
#pragma unroll
                for (int h = 0; h < 4; ++h) acc[g][h] = mfma444(av[g], bv[h], acc[g][h]);
        }
    }
    // epilogue: mu, the S x R result when asked for, and the tile's arg-max per draw (rows ascending inside a lane, then the
    // lanes that hold the same draw: bits 3, 4, 5 of the lane number)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int64_t s = s0 + 32 * wc + 8 * h + dc;
        double v = -INFINITY;
        long long idx = -1;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int64_t j = j0 + 64 * wr + 8 * g + dr;
            if (j < R && s < S) {
                const double f = mu[j] + acc[g][h];
                if (samples) samples[s * R + j] = f;
                if (better(f, j, v, idx)) { v = f; idx = j; }
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
    if (tid < SM_DRAWS && s0 + tid < S) {
        double v = rec_l[0][tid].val;
        long long idx = rec_l[0][tid].idx;
        if (better(rec_l[1][tid].val, rec_l[1][tid].idx, v, idx)) { v = rec_l[1][tid].val; idx = rec_l[1][tid].idx; }
        part[(s0 + tid) * ntiles + tile] = Best{idx >= 0 ? v : -INFINITY, idx};
    }
}

// one wave per draw: the tile records in tile order (ties -> the smallest index)
__global__ __launch_bounds__(64) void k_sample_best(const Best* __restrict__ part, int ntiles, Best* __restrict__ out) {
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
    if (threadIdx.x == 0) out[s] = Best{idx >= 0 ? v : -INFINITY, idx >= 0 ? idx : -1};
}

}  // namespace bohip
