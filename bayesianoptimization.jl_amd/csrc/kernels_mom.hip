// kernels_mom.hip -- two to four objectives (include/bohip_mom.h): the exact expected hypervolume improvement of R
// candidates as a sum over the boxes that partition the region no front point dominates, its 2M partials in the moments, the d
// gradient entries and the arg-max record.
//
//   k_ehvi_boxes<M, GRAD>   ONE wavefront takes one candidate, whatever R is; a workgroup holds 4 of them (value form) or 2 (GRAD
//                  form: three tables per objective, 2 x 4 x 3 x 258 doubles = 49.5 KB of LDS at M = 4).
//                  Stage 1: the wave fills its candidate's tables in LDS, T_m[level] = Psi_m (and Phi_m, phi_m) at the front's
//                  coordinate levels -- each level evaluated once, at most M x 258 erfc / exp pairs.
//                  Stage 2: lane g walks boxes g, g + 64, ... in ascending order; a box is M words (lo | hi << 16 per objective),
//                  read coalesced from global memory -- the same for every candidate, so they stay in L2 -- the factors are
//                  differences of two table entries; private accumulators, then an xor butterfly (32, 16, 8, 4, 2, 1).
//                  The workgroup's arg-max record, then k_argmax_final.  The grid is capped at MO_GRID_MAX with a stride loop.
// No atomics, no scratch, contraction off.  tests/mom_reference.py is the NumPy twin, operation for operation; exp and erfc are the
// device's.
#include "common.h"   // (mo_psi, mo_finite and MO_GRID_MAX come from kernels_mo.hip, `better` and block_argmax from kernels_score.hip, included before)

namespace bohip {

constexpr int MOM_OBJ_MAX = 4;                    // BOHIP_MOM_OBJ_MAX
constexpr int MOM_FRONT_MAX = 256;                // BOHIP_MOM_FRONT_MAX
constexpr int MOM_LEVELS = MOM_FRONT_MAX + 2;     // entries of a level array: ref, the front's distinct values, +Inf
constexpr int MOM_BOX_MAX = 65536;                // BOHIP_MOM_BOX_MAX
constexpr int MOM_LANES = 64;                     // BOHIP_MOM_LANES: one wavefront per candidate
constexpr int mom_cand(bool grad) { return grad ? 2 : 4; }   // candidates (wavefronts) per workgroup

struct MomLevels { int n[MOM_OBJ_MAX]; };         // entries in use per objective

// levels: M rows of stride MOM_LEVELS.  boxes: M rows of stride nbox, word = lo | hi << 16 (level indices).  mu, var: M rows of
// stride ldm.  pmu, pvar (GRAD): the 2M partials, same layout.  jmu, jvar (GRAD, nullable): the models' Jacobians, M planes of
// stride jplane, each [r][d]; grad [r][d].
template <int M, bool GRAD>
__global__ __launch_bounds__(64 * mom_cand(GRAD)) void k_ehvi_boxes(const double* __restrict__ levels, MomLevels nl,
                                                                     const unsigned* __restrict__ boxes, int nbox,
                                                                     const double* __restrict__ mu, const double* __restrict__ var,
                                                                     int64_t ldm, int64_t R, double* __restrict__ value,
                                                                     double* __restrict__ pmu, double* __restrict__ pvar,
                                                                     const double* __restrict__ jmu, const double* __restrict__ jvar,
                                                                     int64_t jplane, int d, double* __restrict__ grad,
                                                                     Best* __restrict__ block_best) {
#pragma clang fp contract(off)
    constexpr int W = mom_cand(GRAD), T = GRAD ? 3 : 1;
    __shared__ double tab[W][M][T][MOM_LEVELS];
    __shared__ Best shb[4];
    const int lane = threadIdx.x & (MOM_LANES - 1), wave = threadIdx.x / MOM_LANES;
    double bv = -INFINITY;
    long long bidx = -1;
    // (the loop bound is uniform over the workgroup: every wave reaches every barrier)
    for (int64_t j0 = (int64_t)blockIdx.x * W; j0 < R; j0 += (int64_t)gridDim.x * W) {
        const int64_t j = j0 + wave;
        const bool valid = j < R;
        double m_[M], v_[M], sd_[M];
        bool bad = false;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            m_[m] = valid ? mu[m * ldm + j] : 0.0;
            v_[m] = valid ? var[m * ldm + j] : 1.0;
            bad = bad || !mo_finite(m_[m]) || !mo_finite(v_[m]) || v_[m] < 0.0;
            sd_[m] = sqrt(v_[m]);
        }
        if (valid) {
#pragma unroll
            for (int m = 0; m < M; ++m)
                for (int i = lane; i < nl.n[m]; i += MOM_LANES) {
                    double P, F, f;
                    mo_psi(m_[m], v_[m], sd_[m], levels[m * MOM_LEVELS + i], P, F, f);
                    tab[wave][m][0][i] = P;
                    if (GRAD) { tab[wave][m][1][i] = F; tab[wave][m][2][i] = f; }
                }
        }
        __syncthreads();
        double av = 0.0, am[M], as[M];
#pragma unroll
        for (int m = 0; m < M; ++m) { am[m] = 0.0; as[m] = 0.0; }
        if (valid) {
            for (int b = lane; b < nbox; b += MOM_LANES) {
                double dP[M], dF[M], df[M];
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const unsigned w = boxes[(int64_t)m * nbox + b];
                    const int lo = (int)(w & 0xffffu), hi = (int)(w >> 16);
                    dP[m] = tab[wave][m][0][lo] - tab[wave][m][0][hi];
                    if (GRAD) {
                        dF[m] = tab[wave][m][1][lo] - tab[wave][m][1][hi];
                        df[m] = tab[wave][m][2][lo] - tab[wave][m][2][hi];
                    }
                }
                double p = dP[0];
#pragma unroll
                for (int l = 1; l < M; ++l) p = p * dP[l];
                av += p;
                if (GRAD) {
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        double pF = m == 0 ? dF[0] : dP[0], pf = m == 0 ? df[0] : dP[0];
#pragma unroll
                        for (int l = 1; l < M; ++l) {
                            pF = pF * (l == m ? dF[l] : dP[l]);
                            pf = pf * (l == m ? df[l] : dP[l]);
                        }
                        am[m] += pF;
                        as[m] += pf;
                    }
                }
            }
        }
#pragma unroll
        for (int o = MOM_LANES / 2; o > 0; o >>= 1) {
            av += __shfl_xor(av, o);
            if (GRAD) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    am[m] += __shfl_xor(am[m], o);
                    as[m] += __shfl_xor(as[m], o);
                }
            }
        }
        const double f = bad ? NAN : av;
        if (valid && lane == 0) {
            value[j] = f;
            if (f > -INFINITY && better(f, (long long)j, bv, bidx)) { bv = f; bidx = j; }   // false for NaN
        }
        if (GRAD && valid) {
            double p_[M], q_[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                p_[m] = bad ? NAN : am[m];
                q_[m] = bad ? NAN : v_[m] > 0.0 ? as[m] / (2.0 * sd_[m]) : 0.0;
                if (lane == 0) { pmu[m * ldm + j] = p_[m]; pvar[m * ldm + j] = q_[m]; }
            }
            if (grad) {
                for (int k = lane; k < d; k += MOM_LANES) {
                    const int64_t q = j * d + k;
                    double gk = 0.0;
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        gk += p_[m] * jmu[m * jplane + q];
                        if (v_[m] > 0.0) gk += q_[m] * jvar[m * jplane + q];
                    }
                    grad[q] = gk;
                }
            }
        }
        __syncthreads();   // (the tables are rewritten by the next pass)
    }
    if (block_best) {
        block_argmax(bv, bidx, shb);
        if (threadIdx.x == 0) { block_best[blockIdx.x].val = bidx >= 0 ? bv : -INFINITY; block_best[blockIdx.x].idx = bidx; }
    }
}

}  // namespace bohip
