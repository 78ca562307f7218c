// kernels_mo.hip -- two-objective optimisation (include/bohip_mo.h): the exact expected hypervolume improvement of R
// candidates over a front of n points, its four partials in the moments, the d gradient entries and the arg-max record.
//
//   k_ehvi<GRAD>   MO_G = 16 consecutive lanes take one candidate, whatever R is (a thread per candidate leaves the chip idle on the
//                  ascent's handful of candidates, a wave per candidate wastes lanes on short fronts).  The front's corners and
//                  heights are staged in LDS once per workgroup.  Lane g takes strips g, g + 16, g + 32, ... in ascending order into
//                  private accumulators; an xor butterfly (8, 4, 2, 1) finishes the sums.  Psi_1 is evaluated at each corner ONCE:
//                  consecutive strips sit on consecutive lanes, so a strip takes its lower corner from the lane below by a shuffle
//                  and lane 0 takes the previous sweep's lane 15.  The workgroup's arg-max record, then k_argmax_final.
// No atomics, no scratch, contraction off.  tests/mo_reference.py is the NumPy twin, operation for operation; exp and erfc are the
// device's.
#include "common.h"   // (`better` and block_argmax come from kernels_score.hip, CON_GRID_MAX from kernels_con.hip, included before)

namespace bohip {

constexpr int MO_FRONT_MAX = 1024;         // BOHIP_MO_FRONT_MAX
constexpr int MO_G = 16;                   // BOHIP_MO_GROUP: lanes per candidate
constexpr int MO_CAND = 256 / MO_G;        // candidates per workgroup and pass
constexpr int MO_GRID_MAX = CON_GRID_MAX;  // workgroups of k_ehvi (the records share k_con_combine's block): beyond that a group takes a second candidate
constexpr double MO_SQRT2 = 1.4142135623730951, MO_RSQRT2PI = 0.3989422804014327;

__device__ __forceinline__ bool mo_finite(double x) { return fabs(x) < INFINITY; }   // (false for NaN)

// Psi(t) = E[(f - t)+] of f ~ N(mu, s2) with Phi and phi at z = (mu - t) / sd: bohip_mo.h, section 1
__device__ __forceinline__ void mo_psi(double mu, double s2, double sd, double t, double& psi, double& Phi, double& phi) {
#pragma clang fp contract(off)
    if (t == INFINITY) { psi = 0.0; Phi = 0.0; phi = 0.0; return; }
    const double D = mu - t;
    if (s2 == 0.0) { psi = D > 0.0 ? D : 0.0; Phi = D > 0.0 ? 1.0 : 0.0; phi = 0.0; return; }
    const double z = D / sd;
    Phi = 0.5 * erfc(-z / MO_SQRT2);
    phi = MO_RSQRT2PI * exp(-0.5 * (z * z));
    psi = sd * phi + D * Phi;
}

// fr: the corners c[0 .. n + 1] (c[0] = r1, c[n + 1] = +Inf) followed by the heights b[0 .. n] (b[n] = r2); strip s = 0 .. n spans
// [c[s], c[s + 1]] above b[s].  mu, var: 2 rows of stride ldm.  pmu, pvar (GRAD): the four partials, same layout.  jmu, jvar (GRAD,
// nullable): the two models' Jacobians, 2 planes of stride jplane, each [r][d]; grad [r][d].
template <bool GRAD>
__global__ __launch_bounds__(256) void k_ehvi(const double* __restrict__ fr, int n, const double* __restrict__ mu,
                                              const double* __restrict__ var, int64_t ldm, int64_t R, double* __restrict__ value,
                                              double* __restrict__ pmu, double* __restrict__ pvar, const double* __restrict__ jmu,
                                              const double* __restrict__ jvar, int64_t jplane, int d, double* __restrict__ grad,
                                              Best* __restrict__ block_best) {
#pragma clang fp contract(off)
    __shared__ double sc[MO_FRONT_MAX + 2], sb[MO_FRONT_MAX + 1];
    __shared__ Best shb[4];
    for (int i = threadIdx.x; i < n + 2; i += 256) sc[i] = fr[i];
    for (int i = threadIdx.x; i < n + 1; i += 256) sb[i] = fr[n + 2 + i];
    __syncthreads();
    const int g = threadIdx.x & (MO_G - 1), grp = threadIdx.x / MO_G;
    double bv = -INFINITY;
    long long bidx = -1;
    // (the loop bound is uniform over the workgroup: every lane reaches every shuffle)
    for (int64_t j0 = (int64_t)blockIdx.x * MO_CAND; j0 < R; j0 += (int64_t)gridDim.x * MO_CAND) {
        const int64_t j = j0 + grp;
        const bool valid = j < R;
        const double m1 = valid ? mu[j] : 0.0, v1 = valid ? var[j] : 1.0, m2 = valid ? mu[ldm + j] : 0.0, v2 = valid ? var[ldm + j] : 1.0;
        const bool bad = !mo_finite(m1) || !mo_finite(v1) || v1 < 0.0 || !mo_finite(m2) || !mo_finite(v2) || v2 < 0.0;
        const double sd1 = sqrt(v1), sd2 = sqrt(v2);
        double cP, cF, cf;                                   // Psi_1, Phi_1, phi_1 at the sweep's first lower corner
        mo_psi(m1, v1, sd1, sc[0], cP, cF, cf);
        double av = 0.0, am1 = 0.0, as1 = 0.0, am2 = 0.0, as2 = 0.0;
        for (int s0 = 0; s0 <= n; s0 += MO_G) {
            const int s = s0 + g;
            const bool act = s <= n;
            double uP = 0.0, uF = 0.0, uf = 0.0, hP = 0.0, hF = 0.0, hf = 0.0;
            if (act) {
                mo_psi(m1, v1, sd1, sc[s + 1], uP, uF, uf);
                mo_psi(m2, v2, sd2, sb[s], hP, hF, hf);
            }
            double lP = __shfl_up(uP, 1, MO_G);
            const double nP = __shfl(uP, MO_G - 1, MO_G);
            if (g == 0) lP = cP;
            cP = nP;
            const double dlt = lP - uP;
            if (act) av += dlt * hP;
            if (GRAD) {
                double lF = __shfl_up(uF, 1, MO_G), lf = __shfl_up(uf, 1, MO_G);
                const double nF = __shfl(uF, MO_G - 1, MO_G), nf = __shfl(uf, MO_G - 1, MO_G);
                if (g == 0) { lF = cF; lf = cf; }
                cF = nF; cf = nf;
                if (act) {
                    am1 += (lF - uF) * hP;
                    as1 += (lf - uf) * hP;
                    am2 += dlt * hF;
                    as2 += dlt * hf;
                }
            }
        }
#pragma unroll
        for (int o = MO_G / 2; o > 0; o >>= 1) {
            av += __shfl_xor(av, o, MO_G);
            if (GRAD) {
                am1 += __shfl_xor(am1, o, MO_G);
                as1 += __shfl_xor(as1, o, MO_G);
                am2 += __shfl_xor(am2, o, MO_G);
                as2 += __shfl_xor(as2, o, MO_G);
            }
        }
        const double f = bad ? NAN : av;
        if (valid && g == 0) {
            value[j] = f;
            if (f > -INFINITY && better(f, (long long)j, bv, bidx)) { bv = f; bidx = j; }   // false for NaN
        }
        if (GRAD && valid) {
            const double p1 = bad ? NAN : am1, q1 = bad ? NAN : v1 > 0.0 ? as1 / (2.0 * sd1) : 0.0;
            const double p2 = bad ? NAN : am2, q2 = bad ? NAN : v2 > 0.0 ? as2 / (2.0 * sd2) : 0.0;
            if (g == 0) { pmu[j] = p1; pvar[j] = q1; pmu[ldm + j] = p2; pvar[ldm + j] = q2; }
            if (grad) {
                for (int k = g; k < d; k += MO_G) {
                    const int64_t q = j * d + k;
                    double gk = 0.0;
                    gk += p1 * jmu[q];
                    if (v1 > 0.0) gk += q1 * jvar[q];
                    gk += p2 * jmu[jplane + q];
                    if (v2 > 0.0) gk += q2 * jvar[jplane + q];
                    grad[q] = gk;
                }
            }
        }
    }
    if (block_best) {
        block_argmax(bv, bidx, shb);
        if (threadIdx.x == 0) { block_best[blockIdx.x].val = bidx >= 0 ? bv : -INFINITY; block_best[blockIdx.x].idx = bidx; }
    }
}

}  // namespace bohip
