// kernels_nei_grad.hip -- the gradient of noisy expected improvement in the candidate (include/bohip_nei_grad.h).
//     grad NEI(x) = sum_n dk(x, X_n)/dx e[n],   e[n] = sum_s omega_s alpha_s[n] - 2 c u[n],   u = W_d'W_d k* (the companion's U' row)
//     omega_s = (1 / S1) da/dmu(m_s, s^2; tau_s),   c = (1 / S1) sum_s da/ds^2(m_s, s^2; tau_s),   c = 0 where s^2 == 0 exactly
// (LogEI: omega_s = p_s dv_s/dmu, c = sum_s p_s dv_s/ds^2 with p_s the soft-max weights of the log-mean-exp.)  Per K*' chunk:
//   k_nei_transpose            alpha' [Npad][Sp] from alpha [s][n], once per fantasy rebuild: the NT tile loop wants both operands K-major
//   k_nei_weights              k_nei_reduce's frame and statements (the same score bits from the same means) plus a pass for the partials:
//                              omega [r][Sp] candidate-major, s contiguous, padded with zeros; c [r]
//   k_nei_mix                  E = omega alpha'' - 2 c U' on v_mfma_f64_4x4x4 through gemm_core.h's LDS-DMA tile loop, 128 candidates x 64
//                              observations a workgroup, the whole contraction (Sp <= 1024) in one job; the tile leaves through LDS
//                              row-major and the epilogue reads the U' tile and writes E over it in place; columns >= N leave as zero
//   k_nei_grad_finish<DT, LOW> grad[r][k] = sum_n dk(x_r, X_n)/dx_k E[r][n]: k_post_grad_finish's loop with ONE stream (same order, same
//                              observation split with the last arriver adding the splits in fixed order)
//   k_nei_grad_finish_tiled    k_post_grad_finish_tiled's likewise: GC candidates share the observation stream
// No atomics beyond the finish's arrival counter; every sum has one writer and a fixed order.
// Included by bohip.hip after kernels_nei.hip and kernels_con.hip (NeiReduce, acq_eval / acq_partials, grad_finish_waves, GC).
#pragma once
#include "common.h"
#include "gemm_core.h"

namespace bohip {

constexpr int NEI_TR = 32;   // k_nei_transpose's tile

// AT[n][s] = A[s][n] for n < Npad, s < Sp (rows >= S1 and columns >= N of alpha are zero: so is the padding of alpha')
__global__ __launch_bounds__(256) void k_nei_transpose(const double* __restrict__ A, int64_t lda, int64_t Npad, int Sp, double* __restrict__ AT) {
    __shared__ double t[NEI_TR][NEI_TR + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int64_t n0 = (int64_t)blockIdx.x * NEI_TR;
    const int s0 = blockIdx.y * NEI_TR;
#pragma unroll
    for (int i = 0; i < NEI_TR; i += 8) {
        const int s = s0 + ty + i;
        t[ty + i][tx] = (s < Sp && n0 + tx < Npad) ? A[(int64_t)s * lda + n0 + tx] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NEI_TR; i += 8) {
        const int64_t n = n0 + ty + i;
        if (n < Npad && s0 + tx < Sp) AT[n * Sp + s0 + tx] = t[tx][ty + i];
    }
}

struct NeiWeights {
    NeiReduce r;         // k_nei_reduce's arguments, read the same way
    double* omega;       // [tiles 128][ldo]: row = the chunk's candidate (column of MT), s contiguous; columns [S1, ldo) zero
    double* c;           // [tiles 128]
    int64_t ldo;
};
__global__ __launch_bounds__(NEI_RED_THREADS) void k_nei_weights(NeiWeights w) {
#pragma clang fp contract(off)
    const NeiReduce& a = w.r;
    __shared__ double tl[NEI_SMAX];
    __shared__ Best sh[4];
    for (int e = threadIdx.x; e < a.S1; e += NEI_RED_THREADS) tl[e] = a.tau[e];
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * NEI_RED_THREADS + threadIdx.x, r = a.r0 + c;
    const bool live = r < a.r1;
    const bool lme = a.ap.acq == ACQ_LOGEI;
    double* om = w.omega + c * w.ldo;
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
        // the partials, s = 0, 1, ...: the plain mean's weights are 1 / S1, the log-mean-exp's the soft-max p_s (a fantasy of weight
        // exactly 0 contributes 0 whatever its partials; a score of -Inf has a zero gradient, a NaN score a NaN one)
        double cs = 0.0;
        for (int s = 0; s < a.S1; ++s) {
            double m = a.MT[(int64_t)s * a.ldm + c];
            for (int z = 1; z < a.nsl; ++z) m = m + a.MT[z * a.plane + (int64_t)s * a.ldm + c];
            AcqParams ap = a.ap;
            ap.p0 = tl[s];
            double p = 1.0 / (double)a.S1;
            if (lme) {
                const double v = acq_eval(ap, m, s2);
                p = vmax == -INFINITY ? 0.0 : (v == vmax ? 1.0 : exp(v - vmax)) / sum;
            }
            double dmu = 0.0, ds2 = 0.0;
            if (p != 0.0) acq_partials(ap, m, s2, dmu, ds2);
            om[s] = p * dmu;
            cs = cs + p * ds2;
        }
        w.c[c] = s2 > 0.0 ? cs : 0.0;   // k_grad_finish's rule for a clamped variance
        for (int s = a.S1; s < w.ldo; ++s) om[s] = 0.0;
    } else {
        for (int s = 0; s < w.ldo; ++s) om[s] = 0.0;   // the rest of the 128-candidate tile k_nei_mix reads
        w.c[c] = 0.0;
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

// E[ti 128 + r][tj 64 + n] = sum_s A[ti 128 + r][s] B[tj 64 + n][s] - 2 c[ti 128 + r] E[..][..]:  A = omega (candidate-major), B = alpha'
// (observation-major), both K-major with the leading dimension Sp = 16 kc; E holds U' on entry.
struct NeiMix {
    const double* A;   // [mt 128][ld]
    const double* B;   // [nt 64][ld]
    const double* c;   // [mt 128]
    double* E;         // [rows][lde], in place
    int64_t ld, lde, N;
    int mt, nt, kc, rows;   // rows: live candidates (only their rows of E are touched)
};
__global__ __launch_bounds__(GEMM_THREADS_8, 2) void k_nei_mix(NeiMix p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int ti = (int)blockIdx.x / p.nt, tj = (int)blockIdx.x % p.nt;
    double acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    gemm_tile_loop_glds3_ks<4>(p.A + (int64_t)ti * TILE * p.ld, p.ld, p.B + (int64_t)tj * CTILE * p.ld, p.ld, 0, p.kc, smem, acc);
    const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6), wr = (wave & 3) >> 1, wc = wave & 1;
    constexpr int TS = CTILE + 2;
    double* Tl = smem;   // [128][66]: the staging buffers are free (the loop ended on a barrier)
    if (wave < 4) {
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) Tl[acc_row(lane, wr, mi) * TS + acc_col<4>(lane, wc, nj)] = acc[mi][nj];
    }
    __syncthreads();
    // a row of the tile is 32 pairs: 32 consecutive threads read and write 512 contiguous bytes of U' / E
#pragma unroll
    for (int u = 0; u < (TILE * CTILE / 2) / GEMM_THREADS_8; ++u) {
        const int piece = threadIdx.x + GEMM_THREADS_8 * u, row = piece >> 5, col = (piece & 31) * 2;
        const int64_t r = (int64_t)ti * TILE + row, n = (int64_t)tj * CTILE + col;
        if (r >= p.rows) continue;
        d2* e = reinterpret_cast<d2*>(p.E + r * p.lde + n);
        const double c2 = 2.0 * p.c[r];
        d2 v = {0.0, 0.0};
        if (n < p.N) {
            const d2 uu = *e;
            v.x = Tl[row * TS + col] - c2 * uu.x;
            if (n + 1 < p.N) v.y = Tl[row * TS + col + 1] - c2 * uu.y;
        }
        *e = v;
    }
}

template <int DT, bool LOW>
__global__ __launch_bounds__(256, grad_finish_waves(DT, LOW)) void k_nei_grad_finish(const double* __restrict__ X, int64_t N,
                                                     const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                                     KernelHyper hp, const double* __restrict__ E, int64_t lde,
                                                     double* __restrict__ grad, double* __restrict__ parts,
                                                     unsigned* __restrict__ counters) {
    // workgroup (r, sp): candidate r, observations [sp len, (sp + 1) len) -- see k_grad_finish.  Contraction is off here and in the
    // tiled form, so a candidate's gradient does not depend on which of the two the batch size selects (one split).
#pragma clang fp contract(off)
    __shared__ double red[4][DT];
    __shared__ int is_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = r_begin + blockIdx.x;
    if (r >= r_end) return;
    const int d = hp.d, S = gridDim.y, sp = blockIdx.y;
    const int64_t len = ((N + S - 1) / S + 255) / 256 * 256;
    const int64_t j_lo = sp * len, j_hi = min(N, j_lo + len);
    const double* xs = Xs + r * d;
    double ge[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) ge[k] = 0.0;
    const double* e = E + (r - r_begin) * lde;
    for (int64_t j = j_lo + threadIdx.x; j < j_hi; j += 256) {
        double t[DT], rr = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                t[k] = xs[k] - X[j * d + k];
                rr += hp.il2[k] * (t[k] * t[k]);
            }
        double fac;
        if constexpr (LOW) {
            fac = matern_lo_fx(hp.fam, hp.sigma2, rr);
        } else if (hp.fam == FAM_M52) {
            const double s = sqrt(5.0) * sqrt(rr);
            fac = -(5.0 / 3.0) * hp.sigma2 * (1.0 + s) * exp(-s);
        } else {
            fac = -(hp.sigma2 * exp(-0.5 * rr));
        }
        const double ej = e[j];
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) ge[k] += fac * t[k] * hp.il2[k] * ej;
    }
#pragma unroll
    for (int k = 0; k < DT; ++k)
        if (k < d) {
            double a = ge[k];
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
            if (lane == 0) red[wave][k] = a;
        }
    __syncthreads();
    if (S > 1) {
        double* mine = parts + ((int64_t)blockIdx.x * S + sp) * DT;
        if (threadIdx.x < d)
            __hip_atomic_store(mine + threadIdx.x, (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (agent-scope stores and a wait, not a fence: see k_grad_finish)
        __syncthreads();
        if (threadIdx.x == 0) is_last = atomicAdd(&counters[blockIdx.x], 1u) == (unsigned)(S - 1);
        __syncthreads();
        if (!is_last) return;
        if (threadIdx.x == 0) counters[blockIdx.x] = 0u;
    }
    if (threadIdx.x < d) {
        const int k = threadIdx.x;
        double a;
        if (S > 1) {
            a = 0.0;
            const double* all = parts + (int64_t)blockIdx.x * S * DT;
            for (int q = 0; q < S; ++q) a += __hip_atomic_load(all + q * DT + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            a = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        }
        grad[r * d + k] = a;
    }
}


template <int DT, bool LOW>
__global__ __launch_bounds__(256) void k_nei_grad_finish_tiled(const double* __restrict__ X, int64_t N,
                                                               const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                                               KernelHyper hp, const double* __restrict__ E, int64_t lde,
                                                               double* __restrict__ grad) {
#pragma clang fp contract(off)
    __shared__ double red[4][GC][DT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rb = r_begin + (int64_t)blockIdx.x * GC;
    if (rb >= r_end) return;
    const int d = hp.d, nc = (int)min((int64_t)GC, r_end - rb);
    double xs[GC][DT], ge[GC][DT], w[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) w[k] = k < d ? hp.il2[k] : 0.0;
#pragma unroll
    for (int c = 0; c < GC; ++c)
#pragma unroll
        for (int k = 0; k < DT; ++k) {
            xs[c][k] = (c < nc && k < d) ? Xs[(rb + c) * d + k] : 0.0;
            ge[c][k] = 0.0;
        }
    for (int64_t j = threadIdx.x; j < N; j += 256) {
        double xj[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) xj[k] = k < d ? X[j * d + k] : 0.0;
#pragma unroll
        for (int c = 0; c < GC; ++c) {
            double t[DT], rr = 0.0;
#pragma unroll
            for (int k = 0; k < DT; ++k) {
                t[k] = xs[c][k] - xj[k];
                rr += w[k] * (t[k] * t[k]);
            }
            double fac;
            if constexpr (LOW) {
                fac = matern_lo_fx(hp.fam, hp.sigma2, rr);
            } else if (hp.fam == FAM_M52) {
                const double s = sqrt(5.0) * sqrt(rr);
                fac = -(5.0 / 3.0) * hp.sigma2 * (1.0 + s) * exp(-s);
            } else {
                fac = -(hp.sigma2 * exp(-0.5 * rr));
            }
            const double ej = c < nc ? E[(rb + c - r_begin) * lde + j] : 0.0;
#pragma unroll
            for (int k = 0; k < DT; ++k) ge[c][k] += fac * t[k] * w[k] * ej;
        }
    }
#pragma unroll
    for (int c = 0; c < GC; ++c)
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                double a = ge[c][k];
                for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
                if (lane == 0) red[wave][c][k] = a;
            }
    __syncthreads();
    if ((int)threadIdx.x < GC * d) {
        const int c = threadIdx.x / d, k = threadIdx.x % d;
        if (c < nc) grad[(rb + c) * d + k] = (red[0][c][k] + red[1][c][k]) + (red[2][c][k] + red[3][c][k]);
    }
}

}  // namespace bohip
