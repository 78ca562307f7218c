// kernels_kg_grad.hip -- the knowledge gradient at free points and its gradient in the point (include/bohip_kg_grad.h).
// A discretisation A = a_0 .. a_{R-1} is resident (V' of A, mu of A, A itself); an evaluation point x has R + 1 lines, a_j's with the
// slope Sigma(a_j, x) / s and its own with sigma^2(x) / s, s = sqrt(sigma^2(x) + nu).  By the envelope theorem
//     grad KG(x) = sum_n e[n] dk(x, X_n)/dx + sum_{i: c_i < R} (q_i / s) dk(x, a_{c_i})/dx
//     e = c_mu alpha + W'(-2 c_sigma v_x - (1 / s) sum_{i: c_i < R} q_i v_{a_{c_i}}),     q_i = phi(z_i) - phi(z_{i+1})
// over the envelope's lines c_0 .. c_n and break points z_1 .. z_n.  Per block of evaluation points:
//   k_kg_cross<LOW>            C[e][j] = k(x_e, a_j) - v_{x_e} . v_{a_j}: an E x R x N NT contraction on v_mfma_f64_4x4x4 through
//                              gemm_core.h's LDS-DMA tile loop, 128 lines x 64 points a workgroup, the whole contraction in one job.  The
//                              tile leaves through LDS point-major; the epilogue adds the kernel value (coordinates streamed from
//                              memory: no register array, one instantiation for every d) and puts sigma^2(x_e) in column R, so the
//                              march reads ONE contiguous, 16-byte aligned row
//   k_kg_march_w               one workgroup per point: k_kg's march (kg_before, kg_reduce, kg_term; the same statements in the same
//                              order, so KG and nseg are bohip_kg_lines' bits on the same lines) on R + 1 lines in LDS.  Thread 0
//                              closes a line when its successor is known: q_i from the two break points, the line and q_i / s to a
//                              strip in global memory, the coefficient of grad sigma^2 in envelope order.  After the march the
//                              strip is staged over the dead lines in LDS and the 256 threads stride N: the mix row
//                              t = -2 c_sigma v_x - sum_i (q_i / s) v_{a_{c_i}} is written over v_x in place, lines in envelope order
//   (U' = V'W on the rows of t: the pass's own product, k_gemm_nt, as it stands)
//   k_kg_grad_finish<DT, LOW>  k_nei_grad_finish's loop, observation split and last-arriver add with e[n] + c_mu alpha[n] as the
//                              coefficient, plus a second stream over the point's envelope lines against A (split 0 takes it)
//   k_kg_grad_finish_tiled     k_nei_grad_finish_tiled's likewise
// No atomics beyond the finish's arrival counter; every sum has one writer and a fixed order.
// Included by bohip.hip after kernels_kg.hip and kernels_nei_grad.hip (KgRec, kg_before, kg_reduce, kg_term; grad_finish_waves, GC).
#pragma once
#include "common.h"
#include "gemm_core.h"

namespace bohip {

struct KgCross {
    const double* VA;    // [mt 128][ld] V' of the discretisation, rows >= R zero
    const double* VX;    // [nt 64][ld]  V' of the block's points
    const double* XA;    // [R][d]
    const double* Xe;    // [rows][d]
    const double* var;   // [rows] sigma^2(x_e), clamped
    double* C;           // [rows][ldc]: Sigma(a_j, x_e) in column j < R, sigma^2(x_e) in column R, zero behind it
    int64_t ld, ldc;
    int R, rows, mt, nt, kc;
};
template <bool LOW>
__global__ __launch_bounds__(GEMM_THREADS_8, 2) void k_kg_cross(KgCross p, KernelHyper hp) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int ti = (int)blockIdx.x / p.nt, tj = (int)blockIdx.x % p.nt;
    double acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    gemm_tile_loop_glds3_ks<4>(p.VA + (int64_t)ti * TILE * p.ld, p.ld, p.VX + (int64_t)tj * CTILE * p.ld, p.ld, 0, p.kc, smem, acc);
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
    // a thread keeps its pair of lines (j, j + 1) and walks 8 points: 64 consecutive threads write 1 KiB of one row of C
    const int d = hp.d, r = (threadIdx.x & 63) * 2;
    const int j = ti * TILE + r;
    if (j >= p.ldc) return;
#pragma unroll 1
    for (int u = 0; u < (TILE * CTILE / 2) / GEMM_THREADS_8; ++u) {
        const int c = (int)(threadIdx.x >> 6) + (GEMM_THREADS_8 / 64) * u, e = tj * CTILE + c;
        if (e >= p.rows) break;
        double rr0 = 0.0, rr1 = 0.0;
        const double* xe = p.Xe + (int64_t)e * d;
        if (j < p.R) {
            const double* a0 = p.XA + (int64_t)j * d;
            const bool two = j + 1 < p.R;
            for (int k = 0; k < d; ++k) {
                const double x = xe[k], t0 = x - a0[k], t1 = two ? x - a0[d + k] : 0.0;
                rr0 += hp.il2[k] * (t0 * t0);
                rr1 += hp.il2[k] * (t1 * t1);
            }
        }
        const double s2 = p.var[e];
        d2 v;
        v.x = j < p.R ? cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr0) - Tl[r * TS + c] : (j == p.R ? s2 : 0.0);
        v.y = j + 1 < p.R ? cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr1) - Tl[(r + 1) * TS + c] : (j + 1 == p.R ? s2 : 0.0);
        *reinterpret_cast<d2*>(p.C + (int64_t)e * p.ldc + j) = v;
    }
}

struct KgMarchW {
    const double* muA;   // [R]
    const double* C;     // [rows][ldc] k_kg_cross's rows
    const double* mu;    // [rows] mu(x_e)
    const double* VA;    // [..][ld]
    double* VX;          // [rows][ld]: v_x on entry, the mix row t on exit (columns < N)
    double* kg;          // [rows]
    int* nseg;           // [rows]
    double* cmu;         // [rows] the coefficient of grad mu
    int* lidx;           // [rows][ldl] the envelope's lines c_i < R, in envelope order
    double* lw;          // [rows][ldl] q_i / s
    int* nline;          // [rows]
    int64_t ld, ldc, ldl, N;
    int R;
    double nu;
};
__device__ __forceinline__ double kgw_phi(double z) { return 0.3989422804014327 * exp(-0.5 * (z * z)); }
__device__ __forceinline__ double kgw_Phi(double z) { return 0.5 * erfc(-z / 1.4142135623730951); }

__global__ __launch_bounds__(KG_THREADS) void k_kg_march_w(KgMarchW p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char kg_smem[];
    __shared__ double bc_cs[2];   // c_sigma, and the number of listed lines (as a double: one broadcast)
    const int R = p.R, R1 = R + 1, Rp = (R1 + 1) & ~1;
    double* sa = reinterpret_cast<double*>(kg_smem);
    double* sb = sa + Rp;
    KgRec* slots = reinterpret_cast<KgRec*>(sb + Rp);
    const int e = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ row = p.C + (int64_t)e * p.ldc;
    double* vx = p.VX + (int64_t)e * p.ld;
    int* li = p.lidx + (int64_t)e * p.ldl;
    double* lw = p.lw + (int64_t)e * p.ldl;
    const double s2x = row[R], dd = s2x + p.nu;
    if (!(dd > 0.0) || !(dd < INFINITY)) {   // (the same in every thread: nobody is left at a barrier)
        for (int64_t n = tid; n < p.N; n += KG_THREADS) vx[n] = 0.0;
        if (tid == 0) { p.kg[e] = 0.0; p.nseg[e] = 0; p.cmu[e] = 0.0; p.nline[e] = 0; }
        return;
    }
    const double s = sqrt(dd);
    auto line = [&](double aj, double bj) {
        bj = bj / s;
        return (fabs(aj) < INFINITY && fabs(bj) < INFINITY) ? bj : NAN;
    };
    for (int j = 2 * tid; j + 1 < R; j += 2 * KG_THREADS) {   // (muA and the rows of C start on 16-byte boundaries)
        const double2 av = *reinterpret_cast<const double2*>(p.muA + j), bv = *reinterpret_cast<const double2*>(row + j);
        *reinterpret_cast<double2*>(sa + j) = av;
        *reinterpret_cast<double2*>(sb + j) = make_double2(line(av.x, bv.x), line(av.y, bv.y));
    }
    if (tid == 0) {
        if (R & 1) { sa[R - 1] = p.muA[R - 1]; sb[R - 1] = line(p.muA[R - 1], row[R - 1]); }
        sa[R] = p.mu[e];
        sb[R] = line(p.mu[e], s2x);   // the point's own line
    }
    __syncthreads();
    // the largest intercept of the discretisation's lines (kg_before on -a: ascending)
    double kz = 0.0, kb = 0.0, ka = 0.0;
    int ki = -1;
    for (int j = tid; j < R; j += KG_THREADS)
        if (sb[j] == sb[j] && kg_before(-sa[j], 0.0, 0.0, j, kz, kb, ka, ki)) { kz = -sa[j]; ki = j; }
    kg_reduce(kz, kb, ka, ki, slots + KG_THREADS / 64);
    const bool own_top = sb[R] == sb[R] && (ki < 0 || sa[R] > -kz);
    // the start: smallest b, then largest a, then smallest index (kg_before on (b, a, 0))
    kz = 0.0; kb = 0.0; ka = 0.0; ki = -1;
    for (int j = tid; j < R1; j += KG_THREADS) {
        const double bj = sb[j];
        if (bj == bj) {
            const double aj = sa[j];
            if (kg_before(bj, aj, 0.0, j, kz, kb, ka, ki)) { kz = bj; kb = aj; ki = j; }
        }
    }
    kg_reduce(kz, kb, ka, ki, slots);
    double acc = 0.0;
    int n = 0;
    // thread 0's books: the line in force since z_in, the listed lines, the coefficient of grad sigma^2, the own line's span
    int cur = ki, nl = 0;
    double z_in = -INFINITY, csig = 0.0, own_lo = 0.0, own_hi = 0.0, q_own = 0.0;
    bool own_on = false;
    const double s3 = 2.0 * (dd * s);
    auto close_line = [&](double z_out) {   // the line `cur` holds the maximum on [z_in, z_out]
        const double q = kgw_phi(z_in) - kgw_phi(z_out);
        if (cur == R) { own_on = true; own_lo = z_in; own_hi = z_out; q_own = q; }
        else { li[nl] = cur; lw[nl] = q / s; csig = csig - q * row[cur] / s3; ++nl; }
    };
    if (ki >= 0) {
        double bc = kz, ac = kb;
        for (int step = 1;; ++step) {
            ki = -1;
            for (int j = tid; j < R1; j += KG_THREADS) {
                const double bj = sb[j];
                if (bj > bc) {
                    const double aj = sa[j];
                    const double z = (ac - aj) / (bj - bc);
                    if (z == z && kg_before(z, bj, aj, j, kz, kb, ka, ki)) { kz = z; kb = bj; ka = aj; ki = j; }
                }
            }
            kg_reduce(kz, kb, ka, ki, slots + (step & 1) * (KG_THREADS / 64));
            if (ki < 0) break;
            if (tid < 64) acc += kg_term(kb - bc, -fabs(kz));
            if (tid == 0) { close_line(kz); cur = ki; z_in = kz; }
            ++n;
            bc = kb;
            ac = ka;
        }
        if (tid == 0) close_line(INFINITY);
    }
    if (tid == 0) {
        double cm = 0.0;
        if (own_on && own_top) cm = -(kgw_Phi(own_lo) + kgw_Phi(-own_hi));   // P_own - 1 with nothing cancelling
        else if (own_on) cm = own_lo >= 0.0 ? kgw_Phi(-own_lo) - kgw_Phi(-own_hi) : kgw_Phi(own_hi) - kgw_Phi(own_lo);
        else if (own_top) cm = -1.0;
        if (own_on) csig = csig + q_own * (s2x + 2.0 * p.nu) / s3;
        if (!(s2x > 0.0)) csig = 0.0;   // k_grad_finish's rule for a clamped variance
        p.kg[e] = acc; p.nseg[e] = n; p.cmu[e] = cm; p.nline[e] = nl;
        bc_cs[0] = csig; bc_cs[1] = (double)nl;
    }
    __syncthreads();   // the march has read its last line; thread 0's strip is visible to the workgroup
    const double c2 = 2.0 * bc_cs[0];
    const int nlist = (int)bc_cs[1];
    int* si = reinterpret_cast<int*>(sb);
    for (int i = tid; i < nlist; i += KG_THREADS) { sa[i] = lw[i]; si[i] = li[i]; }
    __syncthreads();
    for (int64_t c = tid; c < p.N; c += KG_THREADS) {
        double t = 0.0;
        for (int i = 0; i < nlist; ++i) t = t + sa[i] * p.VA[(int64_t)si[i] * p.ld + c];
        vx[c] = -(c2 * vx[c]) - t;
    }
}

template <bool LOW>
__device__ __forceinline__ double kgg_fx(const KernelHyper& hp, double rr) {
    if constexpr (LOW) {
        return matern_lo_fx(hp.fam, hp.sigma2, rr);
    } else {
        if (hp.fam == FAM_M52) {
            const double s = sqrt(5.0) * sqrt(rr);
            return -(5.0 / 3.0) * hp.sigma2 * (1.0 + s) * exp(-s);
        }
        return -(hp.sigma2 * exp(-0.5 * rr));
    }
}

struct KgFinish {
    const double* E;       // [rows][lde] W't of the block's points
    const double* alpha;   // [N]
    const double* cmu;     // [rows]
    const double* XA;      // [R][d]
    const int* lidx;       // [rows][ldl]
    const double* lw;      // [rows][ldl]
    const int* nline;      // [rows]
    int64_t lde, ldl;
};
template <int DT, bool LOW>
__global__ __launch_bounds__(256, grad_finish_waves(DT, LOW)) void k_kg_grad_finish(const double* __restrict__ X, int64_t N,
                                                    const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                                    KernelHyper hp, KgFinish f, double* __restrict__ grad,
                                                    double* __restrict__ parts, unsigned* __restrict__ counters) {
    // workgroup (r, sp): point r, observations [sp len, (sp + 1) len) -- see k_grad_finish; split 0 also takes the envelope's lines
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
    const double* e = f.E + (r - r_begin) * f.lde;
    const double cm = f.cmu[r - r_begin];
    auto add = [&](const double* xo, double coef) {   // ge += coef dk(x, xo)/dx
        double t[DT], rr = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                t[k] = xs[k] - xo[k];
                rr += hp.il2[k] * (t[k] * t[k]);
            }
        const double fac = kgg_fx<LOW>(hp, rr);
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) ge[k] += fac * t[k] * hp.il2[k] * coef;
    };
    for (int64_t j = j_lo + threadIdx.x; j < j_hi; j += 256) add(X + j * d, e[j] + cm * f.alpha[j]);
    if (sp == 0) {
        const int nl = f.nline[r - r_begin];
        const int* li = f.lidx + (r - r_begin) * f.ldl;
        const double* lw = f.lw + (r - r_begin) * f.ldl;
        for (int i = threadIdx.x; i < nl; i += 256) add(f.XA + (int64_t)li[i] * d, lw[i]);
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
__global__ __launch_bounds__(256) void k_kg_grad_finish_tiled(const double* __restrict__ X, int64_t N, const double* __restrict__ Xs,
                                                              int64_t r_begin, int64_t r_end, KernelHyper hp, KgFinish f,
                                                              double* __restrict__ grad) {
#pragma clang fp contract(off)
    __shared__ double red[4][GC][DT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rb = r_begin + (int64_t)blockIdx.x * GC;
    if (rb >= r_end) return;
    const int d = hp.d, nc = (int)min((int64_t)GC, r_end - rb);
    double xs[GC][DT], ge[GC][DT], w[DT], cm[GC];
#pragma unroll
    for (int k = 0; k < DT; ++k) w[k] = k < d ? hp.il2[k] : 0.0;
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        cm[c] = c < nc ? f.cmu[rb + c - r_begin] : 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k) {
            xs[c][k] = (c < nc && k < d) ? Xs[(rb + c) * d + k] : 0.0;
            ge[c][k] = 0.0;
        }
    }
    auto add = [&](int c, const double (&xo)[DT], double coef) {
        double t[DT], rr = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k) {
            t[k] = xs[c][k] - xo[k];
            rr += w[k] * (t[k] * t[k]);
        }
        const double fac = kgg_fx<LOW>(hp, rr);
#pragma unroll
        for (int k = 0; k < DT; ++k) ge[c][k] += fac * t[k] * w[k] * coef;
    };
    for (int64_t j = threadIdx.x; j < N; j += 256) {
        double xj[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) xj[k] = k < d ? X[j * d + k] : 0.0;
        const double aj = f.alpha[j];
#pragma unroll
        for (int c = 0; c < GC; ++c) add(c, xj, c < nc ? f.E[(rb + c - r_begin) * f.lde + j] + cm[c] * aj : 0.0);
    }
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        if (c >= nc) continue;
        const int64_t o = rb + c - r_begin;
        const int nl = f.nline[o];
        for (int i = threadIdx.x; i < nl; i += 256) {
            const double* a = f.XA + (int64_t)f.lidx[o * f.ldl + i] * d;
            double xj[DT];
#pragma unroll
            for (int k = 0; k < DT; ++k) xj[k] = k < d ? a[k] : 0.0;
            add(c, xj, f.lw[o * f.ldl + i]);
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
