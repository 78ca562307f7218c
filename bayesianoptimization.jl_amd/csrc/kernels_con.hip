// kernels_con.hip -- constrained optimisation (include/bohip_con.h): the posterior's own Jacobians and the stage that
// combines several models' moments into one score, one gradient and one arg-max record.
//
//   k_post_grad_finish<DT, LOW>        k_grad_finish's loop (same summation order, same observation split with the last-arriver
//                                      combine for a handful of candidates) without a functor: it writes the two raw sums per
//                                      coordinate, grad mu = sum_j alpha_j dk*_j/dx and grad s2 = -2 sum_j u_j dk*_j/dx
//   k_post_grad_finish_tiled<DT, LOW>  k_grad_finish_tiled's loop likewise: GC = 2 candidates per workgroup share the observation stream
//   k_con_combine<GRAD>                thread = candidate: the models in ascending order, contraction off; value, log feasibility,
//                                      with GRAD the partials of the score and (given the models' Jacobians) the d gradient entries;
//                                      the workgroup's arg-max record, then k_argmax_final
// No atomics beyond k_grad_finish's arrival counter, no scratch.  tests/con_reference.py is the NumPy twin of k_con_combine,
// operation for operation; exp, erfc, log and log1p are the device's.
#include "common.h"   // (`better`, block_argmax, acq_eval / acq_partials, grad_finish_waves and GC come from kernels_score.hip, included before)
#include "acq_log.h"

namespace bohip {

constexpr int CON_CMAX = 16;               // BOHIP_CON_CMAX
constexpr int CON_FEAS = -1;               // BOHIP_CON_FEASIBILITY
constexpr int CON_GRID_MAX = 1024;         // workgroups of k_con_combine: beyond 262144 candidates a thread takes a second one
constexpr double CON_C0 = 0.9189385332046728, CON_SQRT2 = 1.4142135623730951, CON_RSQRT2PI = 0.3989422804014327;

template <int DT, bool LOW>
__global__ __launch_bounds__(256, grad_finish_waves(DT, LOW)) void k_post_grad_finish(const double* __restrict__ X, int64_t N,
                                                     const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                                     KernelHyper hp, const double* __restrict__ alpha,
                                                     const double* __restrict__ UT, int64_t ldu,
                                                     double* __restrict__ dmu_out, double* __restrict__ dvar_out,
                                                     double* __restrict__ parts, unsigned* __restrict__ counters) {
    // workgroup (r, sp): candidate r, observations [sp len, (sp + 1) len) -- see k_grad_finish.  Contraction is off in this kernel and
    // in its tiled form: the two then compute the same bits from the same operation order, so a candidate's Jacobians do not
    // depend on which of them the batch size selects.
#pragma clang fp contract(off)
    __shared__ double red[4][2 * DT];
    __shared__ int is_last;
    constexpr int PS = 2 * DT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = r_begin + blockIdx.x;
    if (r >= r_end) return;
    const int d = hp.d, S = gridDim.y, sp = blockIdx.y;
    const int64_t len = ((N + S - 1) / S + 255) / 256 * 256;
    const int64_t j_lo = sp * len, j_hi = min(N, j_lo + len);
    const double* xs = Xs + r * d;
    double gm[DT], gv[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) { gm[k] = 0.0; gv[k] = 0.0; }
    const double* u = UT + (r - r_begin) * ldu;
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
        const double a = alpha[j], uj = u[j];
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                const double dk = fac * t[k] * hp.il2[k];
                gm[k] += dk * a;
                gv[k] += dk * uj;
            }
    }
#pragma unroll
    for (int k = 0; k < DT; ++k)
        if (k < d) {
            double a = gm[k], b = gv[k];
            for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
            if (lane == 0) { red[wave][2 * k] = a; red[wave][2 * k + 1] = b; }
        }
    __syncthreads();
    if (S > 1) {
        double* mine = parts + ((int64_t)blockIdx.x * S + sp) * PS;
        if (threadIdx.x < 2 * d)
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
        double a, b;
        if (S > 1) {
            a = 0.0; b = 0.0;
            const double* all = parts + (int64_t)blockIdx.x * S * PS;
            for (int q = 0; q < S; ++q) {
                a += __hip_atomic_load(all + q * PS + 2 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b += __hip_atomic_load(all + q * PS + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            a = (red[0][2 * k] + red[1][2 * k]) + (red[2][2 * k] + red[3][2 * k]);
            b = (red[0][2 * k + 1] + red[1][2 * k + 1]) + (red[2][2 * k + 1] + red[3][2 * k + 1]);
        }
        dmu_out[r * d + k] = a;
        dvar_out[r * d + k] = -2.0 * b;
    }
}

template <int DT, bool LOW>
__global__ __launch_bounds__(256) void k_post_grad_finish_tiled(const double* __restrict__ X, int64_t N,
                                                                const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                                                KernelHyper hp, const double* __restrict__ alpha,
                                                                const double* __restrict__ UT, int64_t ldu,
                                                                double* __restrict__ dmu_out, double* __restrict__ dvar_out) {
#pragma clang fp contract(off)
    __shared__ double red[4][GC][2 * DT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rb = r_begin + (int64_t)blockIdx.x * GC;
    if (rb >= r_end) return;
    const int d = hp.d, nc = (int)min((int64_t)GC, r_end - rb);
    double xs[GC][DT], gm[GC][DT], gv[GC][DT], w[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) w[k] = k < d ? hp.il2[k] : 0.0;
#pragma unroll
    for (int c = 0; c < GC; ++c)
#pragma unroll
        for (int k = 0; k < DT; ++k) {
            xs[c][k] = (c < nc && k < d) ? Xs[(rb + c) * d + k] : 0.0;
            gm[c][k] = 0.0;
            gv[c][k] = 0.0;
        }
    for (int64_t j = threadIdx.x; j < N; j += 256) {
        double xj[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) xj[k] = k < d ? X[j * d + k] : 0.0;
        const double a = alpha[j];
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
            const double uj = c < nc ? UT[(rb + c - r_begin) * ldu + j] : 0.0;
#pragma unroll
            for (int k = 0; k < DT; ++k) {
                const double dk = fac * t[k] * w[k];
                gm[c][k] += dk * a;
                gv[c][k] += dk * uj;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < GC; ++c)
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                double a = gm[c][k], b = gv[c][k];
                for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
                if (lane == 0) { red[wave][c][2 * k] = a; red[wave][c][2 * k + 1] = b; }
            }
    __syncthreads();
    if ((int)threadIdx.x < GC * d) {
        const int c = threadIdx.x / d, k = threadIdx.x % d;
        if (c < nc) {
            const int64_t r = rb + c;
            const double a = (red[0][c][2 * k] + red[1][c][2 * k]) + (red[2][c][2 * k] + red[3][c][2 * k]);
            const double b = (red[0][c][2 * k + 1] + red[1][c][2 * k + 1]) + (red[2][c][2 * k + 1] + red[3][c][2 * k + 1]);
            dmu_out[r * d + k] = a;
            dvar_out[r * d + k] = -2.0 * b;
        }
    }
}

// ---- the combine stage ---------------------------------------------------------------------------------------------------------
struct ConParams {
    int acq, C;                // ACQ_EI / ACQ_PI / ACQ_LOGEI / CON_FEAS;  constraints
    double p0;                 // tau of the objective's functor
    double thr[CON_CMAX];
    double sense[CON_CMAX];    // +1.0 / -1.0
};

__device__ __forceinline__ bool con_finite(double x) { return fabs(x) < INFINITY; }   // (false for NaN)

// l = log Phi(z) of one constraint and its partials in (mu, s2): bohip_con.h, section 1
__device__ __forceinline__ void con_term(double mu, double s2, double thr, double s, double& l, double& dm, double& dv) {
#pragma clang fp contract(off)
    if (!con_finite(mu) || !con_finite(s2) || s2 < 0.0) { l = NAN; dm = NAN; dv = NAN; return; }
    const double D = s * (mu - thr);
    if (s2 == 0.0) { l = D >= 0.0 ? 0.0 : -INFINITY; dm = 0.0; dv = 0.0; return; }
    const double sd = sqrt(s2), z = D / sd;
    double rho;
    if (z > LOGEI_SWITCH) {
        const double phi = CON_RSQRT2PI * exp(-0.5 * (z * z));
        if (z > 0.0) {
            const double Phic = 0.5 * erfc(z / CON_SQRT2);
            l = log1p(-Phic);
            rho = phi / (1.0 - Phic);
        } else {
            const double Phi = 0.5 * erfc(-z / CON_SQRT2);
            l = log(Phi);
            rho = phi / Phi;
        }
    } else {
        const double t = -z;
        double r = 0.0;
#pragma unroll 1
        for (int k = LOGEI_CF_DEPTH; k >= 2; --k) r = (double)k / (t + r);
        const double c1 = 1.0 / (t + r);
        rho = t + c1;
        l = (-0.5 * (z * z) - CON_C0) - log(rho);
    }
    dm = (s * rho) / sd;
    dv = -((z * rho) / (2.0 * s2));
}

// mu, var: (C + 1) rows of stride ldm.  pmu, pvar (GRAD): the partials of the score, same layout.  jmu, jvar (GRAD, nullable): the
// models' Jacobians, (C + 1) planes of stride jplane, each [r][d]; grad [r][d].
template <bool GRAD>
__global__ __launch_bounds__(256) void k_con_combine(ConParams cp, const double* __restrict__ mu, const double* __restrict__ var,
                                                     int64_t ldm, int64_t R, double* __restrict__ value, double* __restrict__ logfeas,
                                                     double* __restrict__ pmu, double* __restrict__ pvar,
                                                     const double* __restrict__ jmu, const double* __restrict__ jvar, int64_t jplane, int d,
                                                     double* __restrict__ grad, Best* __restrict__ block_best) {
#pragma clang fp contract(off)
    __shared__ Best shb[4];
    double v = -INFINITY;
    long long idx = -1;
    const AcqParams ap{cp.acq, cp.p0, 0.0};
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < R; j += (int64_t)gridDim.x * 256) {
        double L = 0.0;
#pragma unroll 1
        for (int c = 0; c < cp.C; ++c) {
            double l, dm, dv;
            con_term(mu[(int64_t)(c + 1) * ldm + j], var[(int64_t)(c + 1) * ldm + j], cp.thr[c], cp.sense[c], l, dm, dv);
            L += l;
            if (GRAD) { pmu[(int64_t)(c + 1) * ldm + j] = dm; pvar[(int64_t)(c + 1) * ldm + j] = dv; }
        }
        const bool product = cp.acq == ACQ_EI || cp.acq == ACQ_PI;
        double f, a = 0.0, e = 1.0;
        if (cp.acq == CON_FEAS) {
            f = L;
        } else {
            a = acq_eval(ap, mu[j], var[j]);
            if (product) { e = exp(L); f = a * e; }
            else f = a + L;
        }
        value[j] = f;
        if (logfeas) logfeas[j] = L;
        if (f > -INFINITY && better(f, (long long)j, v, idx)) { v = f; idx = j; }   // false for NaN and -Inf
        if (GRAD) {
            // the partials of the score: a dead score (-Inf, or a product whose feasibility underflowed to 0) has none, a NaN score has NaN
            const bool isnan_f = f != f;
            const bool dead = !isnan_f && (f == -INFINITY || (product && e == 0.0));
            double am = 0.0, av = 0.0;
            if (cp.acq != CON_FEAS) acq_partials(ap, mu[j], var[j], am, av);
            const double fo = product ? e : 1.0, fc = product ? f : 1.0;
            pmu[j] = isnan_f ? NAN : dead || cp.acq == CON_FEAS ? 0.0 : fo * am;
            pvar[j] = isnan_f ? NAN : dead || cp.acq == CON_FEAS ? 0.0 : fo * av;
#pragma unroll 1
            for (int c = 0; c < cp.C; ++c) {
                const int64_t o = (int64_t)(c + 1) * ldm + j;
                pmu[o] = isnan_f ? NAN : dead ? 0.0 : fc * pmu[o];
                pvar[o] = isnan_f ? NAN : dead ? 0.0 : fc * pvar[o];
            }
            if (grad) {
#pragma unroll 1
                for (int k = 0; k < d; ++k) {
                    double gk = 0.0;
#pragma unroll 1
                    for (int m = cp.acq == CON_FEAS ? 1 : 0; m <= cp.C; ++m) {
                        const int64_t o = (int64_t)m * ldm + j, q = (int64_t)m * jplane + j * d + k;
                        gk += pmu[o] * jmu[q];
                        if (var[o] > 0.0) gk += pvar[o] * jvar[q];
                    }
                    grad[j * d + k] = dead ? 0.0 : gk;
                }
            }
        }
    }
    if (block_best) {
        block_argmax(v, idx, shb);
        if (threadIdx.x == 0) { block_best[blockIdx.x].val = idx >= 0 ? v : -INFINITY; block_best[blockIdx.x].idx = idx; }
    }
}

}  // namespace bohip
