// kernels_pend_grad.hip -- the gradient of the acquisition under pending evaluations in the candidate (include/bohip_pend_grad.h,
// DESIGN.md 6y).  With kernels_pend.hip's mu_s = mu + b'z_s, s^2 = sigma^2 - |b|^2, A = W'V_p and u = W'W k*:
//     grad P(x) = sum_n dk(x, X_n)/dx e[n] + sum_i t_i dk(x, Xp_i)/dx,   e[n] = Omega alpha[n] - 2 gamma u[n] - sum_i A[n, i] t_i
//     Omega = sum_s omega_s,   w = sum_s omega_s z_s,   gamma = sum_s (weight_s) da/ds^2,   t = L_p^-T (w - 2 gamma b)
//   k_pend_basis       once per pending state: Bt [Npad][48] = [alpha[n] | A[n, 0 .. p) | 0 ...], K-major for the NT tile loop
//   k_pend_weights     ONE WAVE per candidate, four candidates a workgroup: the fantasies are spread over the 64 lanes (lane l takes
//                      s = l, l + 64, ... in ascending order) with Omega, gamma and the p sums of w in the lane's registers; Z and tau_s
//                      stream through LDS in tiles shared by the four waves, rows an odd number of doubles apart so that 64 lanes
//                      reading 64 rows spread over the banks; one xor halving tree over the lanes; lanes 0 .. p-1 then substitute
//                      t = L_p^-T (w - 2 gamma b) column by column against L_p in LDS.  Leaves Cf [r][48] = [Omega, -t, 0 ...] and gamma.
//   (the mix)          E = Cf Bt' - 2 gamma U' over U' in place is k_nei_mix (kernels_nei_grad.hip) with a contraction of 48, and the
//                      contraction of E with dk/dx is k_nei_grad_finish / _tiled: both are launched as they stand
//   k_pend_grad_direct thread = candidate: grad[r] += sum_i t_i dk(x_r, Xp_i)/dx in ascending i, after the stream's sum
// No atomics; every sum has one writer and a fixed order.
// Included by bohip.hip after kernels_pend.hip and kernels_nei_grad.hip (PEND_ZCAP, acq_eval / acq_partials).
#pragma once
#include "common.h"

namespace bohip {

constexpr int PEND_CF = 48;          // columns of Cf and Bt: 1 + PEND_PMAX padded to three 16-deep contraction steps
constexpr int PEND_W_WAVES = 4;      // candidates (waves) per workgroup of k_pend_weights
constexpr int PEND_LS = PEND_PMAX + 1;
static_assert(1 + PEND_PMAX <= PEND_CF && PEND_CF % KC == 0, "Cf holds Omega and t");
static_assert(PEND_PMAX * PEND_LS <= PEND_ZCAP, "L_p takes the Z tile's place after the fantasies");

// row stride of Z in LDS (odd) and fantasies per tile: all of them, or a multiple of 64 so that a fantasy's lane is s % 64
__host__ __device__ inline int pend_w_stride(int p) { return p | 1; }
__host__ __device__ inline int pend_w_tile(int p, int S1) {
    const int st = PEND_ZCAP / pend_w_stride(p) / 64 * 64;
    return st < S1 ? st : S1;
}

__global__ __launch_bounds__(256) void k_pend_basis(const double* __restrict__ alpha, const double* __restrict__ AT, int64_t ld, int64_t N,
                                                    int64_t Npad, int p, double* __restrict__ Bt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, n = e / PEND_CF;
    const int col = (int)(e % PEND_CF);
    if (n >= Npad) return;
    double v = 0.0;
    if (n < N) {
        if (col == 0) v = alpha[n];
        else if (col <= p) v = AT[(int64_t)(col - 1) * ld + n];   // A' = V_p'W, row i = pending column i
    }
    Bt[e] = v;
}

struct PendWeights {
    const double *mu, *var;   // [R] resident mean and (clamped) variance
    const double* B;          // [R][p]
    const double* Z;          // [S1][p]
    const double* tau;        // [S1]
    const double* L;          // [p][p] L_p
    int64_t r0, r1;           // the chunk's candidates; rows of Cf / gam count from r0
    int p, S1, tau_acq;
    AcqParams ap;
    double* Cf;               // [tiles 128][PEND_CF]
    double* gam;              // [tiles 128]
};

__device__ __forceinline__ double wave_sum(double a) {
    for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o);
    return a;
}

__global__ __launch_bounds__(64 * PEND_W_WAVES) void k_pend_weights(PendWeights a) {
#pragma clang fp contract(off)
    __shared__ double zl[PEND_ZCAP];
    __shared__ double tl[PEND_SMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = a.p, zs = pend_w_stride(p);
    const int64_t c = (int64_t)blockIdx.x * PEND_W_WAVES + wave, r = a.r0 + c;
    const bool live = r < a.r1;
    double b[PEND_PMAX], w[PEND_PMAX];
    double mu = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < PEND_PMAX; ++i) {
        b[i] = (live && i < p) ? a.B[r * p + i] : 0.0;
        w[i] = 0.0;
    }
    if (live) {   // k_pend_score's statements: the same s^2 bits
        mu = a.mu[r];
        double bb = 0.0;
#pragma unroll
        for (int i = 0; i < PEND_PMAX; ++i)
            if (i < p) bb = bb + b[i] * b[i];
        s2 = a.var[r] - bb;
        if (!(s2 >= 0.0) && s2 == s2) s2 = 0.0;
    }
    const int ST = pend_w_tile(p, a.S1);
    const bool lme = a.ap.acq == ACQ_LOGEI;   // pass 0: the largest value; pass 1: the weights exp(v - max), normalised at the end
    double vmax = -INFINITY, esum = 0.0, osum = 0.0, gsum = 0.0;
    for (int pass = lme ? 0 : 1; pass < 2; ++pass) {
        for (int s0 = 0; s0 < a.S1; s0 += ST) {
            const int ns = min(ST, a.S1 - s0);
            __syncthreads();
            for (int e = threadIdx.x; e < ns * p; e += 64 * PEND_W_WAVES) zl[(e / p) * zs + e % p] = a.Z[(int64_t)s0 * p + e];
            for (int e = threadIdx.x; e < ns; e += 64 * PEND_W_WAVES) tl[e] = a.tau[s0 + e];
            __syncthreads();
            if (!live) continue;
            for (int s = lane; s < ns; s += 64) {
                const double* z = zl + s * zs;
                double m = mu;
#pragma unroll
                for (int i = 0; i < PEND_PMAX; ++i)
                    if (i < p) m = m + b[i] * z[i];
                AcqParams ap = a.ap;
                if (a.tau_acq) ap.p0 = tl[s];
                double e = 1.0;
                if (lme) {
                    const double v = acq_eval(ap, m, s2);
                    if (pass == 0) {
                        vmax = (v > vmax || v != v) ? v : vmax;   // a NaN sticks
                        continue;
                    }
                    e = v == vmax ? 1.0 : exp(v - vmax);
                    esum = esum + e;
                }
                double dmu = 0.0, ds2 = 0.0;
                if (e != 0.0) acq_partials(ap, m, s2, dmu, ds2);   // (a fantasy of weight exactly 0 contributes 0)
                const double om = e * dmu;
                osum = osum + om;
                gsum = gsum + e * ds2;
#pragma unroll
                for (int i = 0; i < PEND_PMAX; ++i)
                    if (i < p) w[i] = w[i] + om * z[i];
            }
        }
        if (lme && pass == 0)
            for (int o = 32; o > 0; o >>= 1) {
                const double v = __shfl_xor(vmax, o);
                vmax = (v > vmax || v != v) ? v : vmax;
            }
    }
    // the lanes' sums: one halving tree each; the mean's weight 1 / S1 or the soft-max's 1 / sum is applied once, after the tree
    const bool dead = !live || (lme && vmax == -INFINITY);   // a score of -Inf has a zero gradient
    const double scale = dead ? 0.0 : lme ? 1.0 / wave_sum(esum) : 1.0 / (double)a.S1;
    const double Omega = dead ? 0.0 : wave_sum(osum) * scale;
    const double gamma = (dead || !(s2 > 0.0)) ? 0.0 : wave_sum(gsum) * scale;   // k_grad_finish's rule for a clamped variance
    double q = 0.0;   // lane i < p: (w - 2 gamma b)[i]
#pragma unroll
    for (int i = 0; i < PEND_PMAX; ++i)
        if (i < p) {
            const double wi = dead ? 0.0 : wave_sum(w[i]) * scale - 2.0 * gamma * b[i];
            if (lane == i) q = wi;
        }
    __syncthreads();   // the Z tile is dead: L_p takes its place
    for (int e = threadIdx.x; e < p * p; e += 64 * PEND_W_WAVES) zl[(e / p) * PEND_LS + e % p] = a.L[e];
    __syncthreads();
    // t = L_p^-T q, column by column from the last: t_i = q_i / L_ii, then q_l -= L[i][l] t_i for the lanes l < i
    double t = 0.0;
    for (int i = p - 1; i >= 0; --i) {
        const double ti = __shfl(q, i) / zl[i * PEND_LS + i];
        if (lane == i) t = ti;
        if (lane < i) q = q - zl[i * PEND_LS + lane] * ti;
    }
    double* cf = a.Cf + c * PEND_CF;
    if (lane == 0) {
        cf[0] = Omega;
        a.gam[c] = gamma;
    }
    if (lane < p) cf[1 + lane] = dead ? 0.0 : -t;
    else if (lane < PEND_CF - 1) cf[1 + lane] = 0.0;
}

template <bool LOW>
__device__ __forceinline__ double pend_fx(const KernelHyper& hp, double rr) {
#pragma clang fp contract(off)
    if constexpr (LOW) return matern_lo_fx(hp.fam, hp.sigma2, rr);
    if (hp.fam == FAM_M52) {
        const double s = sqrt(5.0) * sqrt(rr);
        return -(5.0 / 3.0) * hp.sigma2 * (1.0 + s) * exp(-s);
    }
    return -(hp.sigma2 * exp(-0.5 * rr));
}

// grad[r][k] += sum_i t_i fx(r_i) il2_k (x_k - Xp_ik), i ascending, t_i = -Cf[r - r0][1 + i]
template <int DT, bool LOW>
__global__ __launch_bounds__(64) void k_pend_grad_direct(const double* __restrict__ Xs, int64_t r0, int64_t r1, KernelHyper hp,
                                                         const double* __restrict__ Xp, int p, const double* __restrict__ Cf,
                                                         double* __restrict__ grad) {
#pragma clang fp contract(off)
    __shared__ double xp[PEND_PMAX * DT];
    const int d = hp.d;
    for (int e = threadIdx.x; e < p * DT; e += 64) xp[e] = (e % DT) < d ? Xp[(e / DT) * d + e % DT] : 0.0;
    __syncthreads();
    const int64_t r = r0 + (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= r1) return;
    double x[DT], ge[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) {
        x[k] = k < d ? Xs[r * d + k] : 0.0;
        ge[k] = k < d ? grad[r * d + k] : 0.0;
    }
    const double* cf = Cf + (r - r0) * PEND_CF;
    for (int i = 0; i < p; ++i) {
        double rr = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                const double t = x[k] - xp[i * DT + k];
                rr += hp.il2[k] * (t * t);
            }
        const double fac = pend_fx<LOW>(hp, rr), ti = -cf[1 + i];
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) ge[k] += fac * (x[k] - xp[i * DT + k]) * hp.il2[k] * ti;
    }
#pragma unroll
    for (int k = 0; k < DT; ++k)
        if (k < d) grad[r * d + k] = ge[k];
}

}  // namespace bohip
