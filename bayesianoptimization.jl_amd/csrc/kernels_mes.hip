// kernels_mes.hip -- max-value entropy search over a candidate set (include/bohip_mes.h; Wang & Jegelka 2017):
//     MES_j = (1/K) sum_k u(mu_j, s2_j, m_k),   u = gamma lambda / 2 - log Phi(gamma),   gamma = (m - mu) / sigma,
// m_0 .. m_{K-1} samples of the maximum of the posterior over the R candidates.
//   k_mes_bracket<FINISH>  lo = max_j (mu_j - 5 sigma_j), hi = max_j (mu_j + 5 sigma_j), max mu over the finite candidates: up to
//                  MES_BR_MAX workgroups stride the candidates and leave one partial each (<false>), ONE workgroup takes the
//                  maximum of the partials and writes the state of the search (<true>).  A maximum is exact, so no order matters.
//   k_mes_probe    one launch per 16-section pass, grid 45 x slices: workgroup (3 q + i - 1, slice) adds
//                  S(y) = sum_j log Phi((y - mu_j) / sigma_j) over its slice at probe i of quantile q.  A pass first NARROWS the
//                  bracket from the sums the pass before it left -- every workgroup does that for its own quantile, from the same
//                  numbers in the same order (slices ascending), so all agree without talking to each other -- and workgroup
//                  (q, probe 1, slice 0) records the bracket.  Sums and brackets are double-buffered between passes: a launch
//                  reads only what the launch before it wrote.  14 launches, no finishing launches between them.
//                  Slices: R <= 8192 is ONE workgroup per (quantile, probe) -- 32 candidates a thread at most; beyond, slices of
//                  8192 candidates, 64 at BOHIP_MES_RMAX (2880 workgroups).  Measured on an MI355X (N = 3000, d = 8, K = 16): the 14
//                  passes take 0.101 ms at R = 1024 (7 us a pass: launch latency) and 0.252 ms at R = 4096 (18 us a pass, 16
//                  candidates a thread), against 0.283 / 0.650 ms for the posterior of the same call.
//   k_mes_draw     one workgroup: the last narrowing, the three midpoints, the Gumbel fit (a, b) and the K samples with the floor
//   k_mes_rowmax   joint mode: one workgroup per draw walks its row of the S x R draws (as k_thompson walks its candidates)
//   k_mes_values<GRAD>  the K max values in LDS (8 KiB at KMAX), one thread per candidate runs the k loop in ascending order, one
//                  IEEE division by K; the workgroup's arg-max record, then k_argmax_final
// No atomics, no communication between workgroups inside a launch.  Contraction is off: tests/mes_reference.py is the NumPy twin,
// operation for operation; exp, erfc, log and log1p are the device's.
#include "common.h"   // (`better`, block_argmax, thompson's splitmix64 come from kernels_score.hip, included before)
#include "acq_log.h"

namespace bohip {

constexpr int MES_KMAX = 1024;             // BOHIP_MES_KMAX
constexpr int64_t MES_RMAX = 524288;       // BOHIP_MES_RMAX
constexpr int MES_PROBES = 15, MES_PASSES = 14, MES_NQ = 3;
constexpr int64_t MES_SLICE = 8192;
constexpr int MES_BR_MAX = 256;
constexpr int MES_STATE = 8;               // doubles per bracket record: lo[3], hi[3], pad[2]
constexpr double MES_C = 0.9189385332046728, MES_SQRT2 = 1.4142135623730951, MES_RSQRT2PI = 0.3989422804014327;
constexpr double MES_GUMBEL_DEN = 1.5725335836855193;   // log(log 4) - log(log(4/3))
constexpr double MES_LOGLOG2 = -0.36651292058166435;    // log(log 2)

// the state of the search: [0]: two bracket records, [2 MES_STATE ...]: lo0, hi0 (the first bracket), max mu
struct MesWs {
    double* st;      // [2 * MES_STATE + 4]
    double* br;      // [3 * MES_BR_MAX] partial maxima
    double* part;    // [2][45 * nsl] the sums of a pass
    int nsl;
};

__device__ __forceinline__ bool mes_finite(double x) { return fabs(x) < INFINITY; }   // (false for NaN)
__device__ __forceinline__ bool mes_cand_ok(double mu, double s2) { return mes_finite(mu) && mes_finite(s2) && s2 >= 0.0; }
__device__ __forceinline__ double mes_logp(int q) { return q == 0 ? -1.3862943611198906 : q == 1 ? -0.6931471805599453 : -0.2876820724517809; }

// Mills' ratio's continued fraction of acq_log.h: r = 2 / (t + 3 / (t + ...)), c1 = 1 / (t + r)
__device__ __forceinline__ void mes_cf(double t, double& r, double& c1) {
#pragma clang fp contract(off)
    r = 0.0;
#pragma unroll 1
    for (int k = LOGEI_CF_DEPTH; k >= 2; --k) r = (double)k / (t + r);
    c1 = 1.0 / (t + r);
}

// log Phi(g) in its three forms
__device__ __forceinline__ double mes_logcdf(double g) {
#pragma clang fp contract(off)
    if (g > 0.0) return log1p(-(0.5 * erfc(g / MES_SQRT2)));
    if (g > LOGEI_SWITCH) return log(0.5 * erfc(-g / MES_SQRT2));
    const double t = -g;
    double r, c1;
    mes_cf(t, r, c1);
    return (-0.5 * (g * g) - MES_C) - log(t + c1);
}

// one term u(mu, s2, m) and its partials; sd = sqrt(s2), ok = mes_cand_ok(mu, s2)
template <bool GRAD>
__device__ __forceinline__ void mes_term(double mu, double s2, double sd, bool ok, double m, double& u, double& dmu, double& ds2) {
#pragma clang fp contract(off)
    if (!ok || !mes_finite(m)) { u = NAN; dmu = NAN; ds2 = NAN; return; }
    if (s2 == 0.0) { u = 0.0; dmu = 0.0; ds2 = 0.0; return; }
    const double g = (m - mu) / sd;
    double d;
    if (g > LOGEI_SWITCH) {
        const double phi = MES_RSQRT2PI * exp(-0.5 * (g * g));
        double lam;
        if (g > 0.0) {
            const double Phic = 0.5 * erfc(g / MES_SQRT2);
            lam = phi / (1.0 - Phic);
            u = (g * lam) / 2.0 - log1p(-Phic);
        } else {
            const double Phi = 0.5 * erfc(-g / MES_SQRT2);
            lam = phi / Phi;
            u = (g * lam) / 2.0 - log(Phi);
        }
        if (GRAD) d = -((lam / 2.0) * ((1.0 + g * g) + g * lam));
    } else {
        const double t = -g;
        double r, c1;
        mes_cf(t, r, c1);
        const double lam = t + c1;
        u = (MES_C + log(lam)) - (0.5 * t) * c1;
        if (GRAD) d = -((lam / 2.0) * (r * c1));
    }
    if (GRAD) {
        dmu = (-d) / sd;
        ds2 = ((-d) * g) / (2.0 * s2);
    }
}

// the maximum of v over the workgroup (256 threads), in every thread.  sh: 4 doubles
__device__ __forceinline__ double mes_block_max(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    __syncthreads();
    return v;
}

template <bool FINISH>
__global__ __launch_bounds__(256) void k_mes_bracket(const double* __restrict__ mu, const double* __restrict__ var, int64_t R, int nparts,
                                                     MesWs w) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    double lo = -INFINITY, hi = -INFINITY, mm = -INFINITY;
    if (!FINISH) {
        for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < R; j += (int64_t)gridDim.x * 256) {
            const double m = mu[j], s2 = var[j];
            if (mes_cand_ok(m, s2)) {
                const double s5 = 5.0 * sqrt(s2);
                lo = fmax(lo, m - s5);
                hi = fmax(hi, m + s5);
                mm = fmax(mm, m);
            }
        }
    } else {
        for (int i = threadIdx.x; i < nparts; i += 256) {
            lo = fmax(lo, w.br[i]);
            hi = fmax(hi, w.br[MES_BR_MAX + i]);
            mm = fmax(mm, w.br[2 * MES_BR_MAX + i]);
        }
    }
    lo = mes_block_max(lo, sh);
    hi = mes_block_max(hi, sh);
    mm = mes_block_max(mm, sh);
    if (threadIdx.x != 0) return;
    if (!FINISH) {
        w.br[blockIdx.x] = lo;
        w.br[MES_BR_MAX + blockIdx.x] = hi;
        w.br[2 * MES_BR_MAX + blockIdx.x] = mm;
    } else {
        double* prev = w.st + MES_STATE;   // what pass 0 reads
        for (int q = 0; q < MES_NQ; ++q) { prev[q] = lo; prev[MES_NQ + q] = hi; }
        w.st[2 * MES_STATE] = lo;
        w.st[2 * MES_STATE + 1] = hi;
        w.st[2 * MES_STATE + 2] = mm;
    }
}

__device__ __forceinline__ double mes_probe_at(double lo, double hi, int i) {
#pragma clang fp contract(off)
    return lo + (hi - lo) * (double)i / 16.0;
}

// The bracket of quantile q after the pass whose sums sit in `part` (slices added in ascending order from +0.0): the first probe
// with S >= log p is the new hi, its predecessor the new lo.  Every thread of the workgroup gets the result.  sh: 16 doubles
__device__ __forceinline__ void mes_narrow(const double* __restrict__ st, const double* __restrict__ part, int nsl, int q, double& lo,
                                           double& hi, double* sh) {
#pragma clang fp contract(off)
    const double lo0 = st[q], hi0 = st[MES_NQ + q];
    if (threadIdx.x < MES_PROBES) {
        const double* p = part + (int64_t)(q * MES_PROBES + threadIdx.x) * nsl;
        double s = 0.0;
        for (int sl = 0; sl < nsl; ++sl) s += p[sl];
        sh[threadIdx.x] = s;
    }
    __syncthreads();
    const double logp = mes_logp(q);
    int first = MES_PROBES;
    for (int i = MES_PROBES - 1; i >= 0; --i)
        if (sh[i] >= logp) first = i;
    __syncthreads();
    // probe numbers are 1-based: sh[i] belongs to probe i + 1
    hi = first < MES_PROBES ? mes_probe_at(lo0, hi0, first + 1) : hi0;
    lo = first == 0 ? lo0 : mes_probe_at(lo0, hi0, first);
}

__global__ __launch_bounds__(256) void k_mes_probe(const double* __restrict__ mu, const double* __restrict__ var, int64_t R, int pass,
                                                   MesWs w) {
#pragma clang fp contract(off)
    __shared__ double sh[16];
    const int q = blockIdx.x / MES_PROBES, i = blockIdx.x % MES_PROBES + 1, sl = blockIdx.y, nsl = w.nsl;
    const double* st_prev = w.st + ((pass + 1) & 1) * MES_STATE;
    const double* part_prev = w.part + (int64_t)((pass + 1) & 1) * (MES_NQ * MES_PROBES) * nsl;
    double lo, hi;
    if (pass == 0) { lo = st_prev[q]; hi = st_prev[MES_NQ + q]; }
    else mes_narrow(st_prev, part_prev, nsl, q, lo, hi, sh);
    if (i == 1 && sl == 0 && threadIdx.x == 0) {
        double* st = w.st + (pass & 1) * MES_STATE;
        st[q] = lo;
        st[MES_NQ + q] = hi;
    }
    const double y = mes_probe_at(lo, hi, i);
    const int64_t per = (R + nsl - 1) / nsl, j0 = (int64_t)sl * per, j1 = min(R, j0 + per);
    double s = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        const double m = mu[j], s2 = var[j];
        if (!mes_cand_ok(m, s2)) continue;
        if (s2 == 0.0) s += y >= m ? 0.0 : -INFINITY;
        else s += mes_logcdf((y - m) / sqrt(s2));
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        w.part[(int64_t)(pass & 1) * (MES_NQ * MES_PROBES) * nsl + (int64_t)blockIdx.x * nsl + sl] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// the first uniform of thompson_normal(seed, k, 0), in (0, 1]
__host__ __device__ inline double mes_uniform(uint64_t seed, int64_t k) {
    const uint64_t h = splitmix64(seed ^ splitmix64((uint64_t)k * 0xD1B54A32D192ED03ull));
    return ((double)(h >> 11) + 1.0) * (1.0 / 9007199254740993.0);
}

__global__ __launch_bounds__(256) void k_mes_draw(MesWs w, int K, uint64_t seed, double floor_value, double* __restrict__ quantiles,
                                                  double* __restrict__ maxvals) {
#pragma clang fp contract(off)
    __shared__ double sh[16];
    const double* st_prev = w.st + ((MES_PASSES + 1) & 1) * MES_STATE;
    const double* part_prev = w.part + (int64_t)((MES_PASSES + 1) & 1) * (MES_NQ * MES_PROBES) * w.nsl;
    const double lo0 = w.st[2 * MES_STATE], hi0 = w.st[2 * MES_STATE + 1];
    double y[MES_NQ];
    for (int q = 0; q < MES_NQ; ++q) {
        double lo, hi;
        mes_narrow(st_prev, part_prev, w.nsl, q, lo, hi, sh);
        y[q] = lo + 0.5 * (hi - lo);
    }
    const bool flat = hi0 == lo0;   // every sigma is 0 (or no candidate is finite): the maximum is lo itself
    if (flat) { y[0] = lo0; y[1] = lo0; y[2] = lo0; }
    const double b = flat ? 0.0 : (y[2] - y[0]) / MES_GUMBEL_DEN;
    const double a = y[1] + b * MES_LOGLOG2;
    if (threadIdx.x < MES_NQ) quantiles[threadIdx.x] = y[threadIdx.x];
    for (int k = threadIdx.x; k < K; k += 256) {
        const double m = flat ? lo0 : a - b * log(-log(mes_uniform(seed, k)));
        maxvals[k] = m > floor_value ? m : floor_value;
    }
}

__global__ __launch_bounds__(256) void k_mes_rowmax(const double* __restrict__ F, int64_t R, double floor_value,
                                                    double* __restrict__ maxvals) {
    __shared__ double sh[4];
    const double* row = F + (int64_t)blockIdx.x * R;
    double v = -INFINITY;
    for (int64_t j = threadIdx.x; j < R; j += 256) {
        const double f = row[j];
        if (mes_finite(f)) v = fmax(v, f);
    }
    v = mes_block_max(v, sh);
    if (threadIdx.x == 0) maxvals[blockIdx.x] = v > floor_value ? v : floor_value;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void k_mes_values(const double* __restrict__ mu, const double* __restrict__ var, int64_t R,
                                                    const double* __restrict__ maxvals, int K, double* __restrict__ mes,
                                                    double* __restrict__ dmu, double* __restrict__ dvar, Best* __restrict__ block_best) {
#pragma clang fp contract(off)
    __shared__ double sm[MES_KMAX];
    __shared__ Best shb[4];
    for (int k = threadIdx.x; k < K; k += 256) sm[k] = maxvals[k];
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v = -INFINITY;
    long long idx = -1;
    if (j < R) {
        const double m = mu[j], s2 = var[j];
        const bool ok = mes_cand_ok(m, s2);
        const double sd = sqrt(ok ? s2 : 0.0);
        double su = 0.0, sa = 0.0, sb = 0.0;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            double u, a = 0.0, b = 0.0;
            mes_term<GRAD>(m, s2, sd, ok, sm[k], u, a, b);
            su += u;
            if (GRAD) { sa += a; sb += b; }
        }
        const double f = su / (double)K;
        mes[j] = f;
        if (GRAD) { dmu[j] = sa / (double)K; dvar[j] = sb / (double)K; }
        if (f > -INFINITY) { v = f; idx = j; }   // false for NaN and -Inf
    }
    if (block_best) {
        block_argmax(v, idx, shb);
        if (threadIdx.x == 0) { block_best[blockIdx.x].val = idx >= 0 ? v : -INFINITY; block_best[blockIdx.x].idx = idx; }
    }
}

}  // namespace bohip
