// kernels_batch.hip -- greedy batch selection (bohip_gp_select_batch): q picks from ONE contraction V = W K*.
// The reference proposes one point per iteration (src/BayesianOptimization.jl:185-196: one acquire_max, then `repetitions`
// evaluations of that point); a batch is an extension.  Conditioning the posterior on a fantasised observation (x_s, y_f) is a
// rank-one update of (mu, sigma^2) over the candidate set, so with V' (candidate-major, row r = L^-1 k*(x_r)) kept from the first
// pass every further pick is one sweep over V' -- the model is never touched:
//   c_r     = k(x_r, x_s) - v_r . v_s - sum_{i<t} u_i[r] u_i[s]        posterior covariance with pick t
//   S       = c_s + noise,   mu_r += c_r (y_f - mu_s) / S,   u_t[r] = c_r / sqrt(S),   sigma^2_r -= u_t[r]^2
//   k_batch_cond   one wave per candidate row: the dot product with v_s (staged in LDS), the update, the score, the workgroup's
//                  arg-max record.  The pick it conditions on is read from device memory: the host enqueues all rounds at once.
//   k_batch_final  one workgroup: reduces the records to pick t, stores it and the scalars of the next round.
#include "gemm_core.h"   // (d2; the functors, `better` and cov_from_r_fast come from kernels_score.hip, included before)

namespace bohip {

struct BatchRec {      // one pick, as it leaves the call
    double val;
    long long idx;     // -1: no candidate could win (val = -Inf, mu = var = NaN)
    double mu, var;    // the conditioned posterior at the pick, before its own fantasy
};
struct BatchScal {     // what round t + 1 needs of pick t
    double mu_s, S, yf, tau;
};
constexpr int BATCH_WG_MAX = 512;          // workgroups of k_batch_cond (= records k_batch_final reduces)
constexpr int BATCH_WAVES = 4;             // waves (= candidate rows in flight) per workgroup
constexpr int BATCH_LDS_MAX = 96 * 1024;   // v_s in LDS up to N = 12288; longer rows read it through L2

struct BatchCond {
    const double* VT;    // [R][ldv] V' of ALL candidates
    int64_t ldv, N;
    const double* Xs;    // [R][d]
    int64_t R;
    double *mu, *var;    // [R] the conditioned posterior (var is NOT clamped; the score sees max(var, 0))
    double* U;           // [q][ldu] u_i
    int64_t ldu;
    const int* picked;   // [R] 1: picked in an earlier round
    const BatchRec* rec; // rec[t]: the pick this round conditions on
    const BatchScal* scal;
    int t;
    int use_lds;
    AcqParams ap;        // p0 of EI / PI is replaced by scal->tau
    Best* block_best;    // [gridDim.x]
};

// sum_j a[j] b[j] over the P = N >> 1 pairs of a row, 16 bytes per lane and load, four independent chains per lane; then a fixed
// butterfly: the same bits whatever the grid.  (An odd last element is added by the caller's finishing lane.)
// Measured at N = 3000, R = 4096 (101 MB of V'): 25.4 us per launch = 4.0 TB/s.  Eight loads per lane in a branch-free loop with
// eight waves per workgroup: 28.3 us -- the bytes in flight are not what bounds it.
__device__ __forceinline__ double batch_row_dot(const d2* __restrict__ vr, const d2* vs, int64_t P, int lane) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t j = lane;
    for (; j + 192 < P; j += 256) {
        const d2 x0 = vr[j], x1 = vr[j + 64], x2 = vr[j + 128], x3 = vr[j + 192];
        const d2 y0 = vs[j], y1 = vs[j + 64], y2 = vs[j + 128], y3 = vs[j + 192];
        a0 += x0.x * y0.x + x0.y * y0.y;
        a1 += x1.x * y1.x + x1.y * y1.y;
        a2 += x2.x * y2.x + x2.y * y2.y;
        a3 += x3.x * y3.x + x3.y * y3.y;
    }
    for (; j < P; j += 64) {
        const d2 x0 = vr[j], y0 = vs[j];
        a0 += x0.x * y0.x + x0.y * y0.y;
    }
    return (a0 + a1) + (a2 + a3);
}

template <bool LOW>
__global__ __launch_bounds__(64 * BATCH_WAVES) void k_batch_cond(BatchCond bc, KernelHyper hp) {
    extern __shared__ __attribute__((aligned(16))) double bc_vs[];
    __shared__ Best sh[BATCH_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = bc.rec[bc.t].idx;   // (uniform)
    double bv = -INFINITY;
    long long bi = -1;
    if (s >= 0) {
        const BatchScal sc = *bc.scal;
        const int64_t N = bc.N, P = N >> 1;
        const double* vs_g = bc.VT + s * bc.ldv;
        if (bc.use_lds) {
            for (int64_t j = tid; j < P; j += 64 * BATCH_WAVES) reinterpret_cast<d2*>(bc_vs)[j] = reinterpret_cast<const d2*>(vs_g)[j];
            __syncthreads();
        }
        AcqParams ap = bc.ap;
        if (ap.acq == ACQ_EI || ap.acq == ACQ_PI || ap.acq == ACQ_LOGEI) ap.p0 = sc.tau;
        const double sqrtS = sqrt(sc.S), dy = sc.yf - sc.mu_s;
        const int d = hp.d;
        for (int64_t r = (int64_t)blockIdx.x * BATCH_WAVES + wave; r < bc.R; r += (int64_t)gridDim.x * BATCH_WAVES) {
            const double* vr = bc.VT + r * bc.ldv;
            double dot = bc.use_lds ? batch_row_dot(reinterpret_cast<const d2*>(vr), reinterpret_cast<const d2*>(bc_vs), P, lane)
                                    : batch_row_dot(reinterpret_cast<const d2*>(vr), reinterpret_cast<const d2*>(vs_g), P, lane);
            double uu = 0.0;
            for (int i = lane; i < bc.t; i += 64) uu += bc.U[(int64_t)i * bc.ldu + r] * bc.U[(int64_t)i * bc.ldu + s];
            for (int o = 32; o > 0; o >>= 1) {
                dot += __shfl_xor(dot, o);
                uu += __shfl_xor(uu, o);
            }
            if (lane != 0) continue;
            if (N & 1) dot += vr[N - 1] * vs_g[N - 1];
            double rr = 0.0;
            for (int k = 0; k < d; ++k) {
                const double t = bc.Xs[r * d + k] - bc.Xs[s * d + k];
                rr += hp.il2[k] * (t * t);
            }
            const double c = cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr) - dot - uu;
            const double u = c / sqrtS;
            const double mu = bc.mu[r] + c * dy / sc.S;
            const double var = bc.var[r] - u * u;
            bc.mu[r] = mu;
            bc.var[r] = var;
            bc.U[(int64_t)bc.t * bc.ldu + r] = u;
            if (bc.picked[r]) continue;
            const double f = acq_eval(ap, mu, var > 0.0 ? var : 0.0);
            if (f > -INFINITY && better(f, r, bv, bi)) { bv = f; bi = r; }   // false for NaN and -Inf
        }
    }
    if (lane == 0) { sh[wave].val = bv; sh[wave].idx = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < BATCH_WAVES; ++w)
            if (better(sh[w].val, sh[w].idx, bv, bi)) { bv = sh[w].val; bi = sh[w].idx; }
        bc.block_best[blockIdx.x].val = bi >= 0 ? bv : -INFINITY;
        bc.block_best[blockIdx.x].idx = bi;
    }
}

// pick t from the n records of round t; the scalars of round t + 1.  tau0: the caller's incumbent (read at t = 0).
struct BatchFinal {
    const Best* in;
    int n, t;
    const double *mu, *var;
    int* picked;
    BatchRec* rec;
    BatchScal* scal;
    int fantasy;        // 0 believer (y_f = mu_s), 1 constant
    double fantasy_value, noise, tau0;
    int raise_tau;      // EI / PI / LogEI: tau <- max(tau, y_f)
};
__global__ __launch_bounds__(256) void k_batch_final(BatchFinal bf) {
    __shared__ Best sh[4];
    double v = -INFINITY;
    long long idx = -1;
    for (int i = threadIdx.x; i < bf.n; i += 256)
        if (better(bf.in[i].val, bf.in[i].idx, v, idx)) { v = bf.in[i].val; idx = bf.in[i].idx; }
    block_argmax(v, idx, sh);
    if (threadIdx.x != 0) return;
    const double tau = bf.t == 0 ? bf.tau0 : bf.scal->tau;
    BatchRec rc{-INFINITY, -1, NAN, NAN};
    BatchScal sc{0.0, 1.0, 0.0, tau};
    if (idx >= 0) {
        const double mu = bf.mu[idx], var = bf.var[idx] > 0.0 ? bf.var[idx] : 0.0;
        rc.val = v; rc.idx = idx; rc.mu = mu; rc.var = var;
        sc.mu_s = mu;
        sc.S = var + bf.noise;
        sc.yf = bf.fantasy == 0 ? mu : bf.fantasy_value;
        if (bf.raise_tau && sc.yf > tau) sc.tau = sc.yf;
        bf.picked[idx] = 1;
    }
    bf.rec[bf.t] = rc;
    *bf.scal = sc;
}

}  // namespace bohip
