// kernels_qei.hip -- greedy Monte-Carlo q-EI over a resident S x R matrix of joint draws (include/bohip_qei.h):
//     qEI(B) = E[max(max_{j in B} f_j - tau, 0)]  ~  (1/S) sum_s max(max_{j in B} F_sj - tau, 0),
// maximised greedily: m_s = tau; every round scores every candidate by its sample-average gain over m, takes the first maximum
// and raises m by the winner's column.  F is row-major (draw s at F[s R + j]), so thread = candidate: consecutive lanes read
// consecutive doubles of one draw's row, and the s-ascending order of a block falls out of the loop.
//   k_qei_init   m = tau, idx = -1, gain = 0, the "nothing can win" word and the arrival counter cleared
//   k_qei_gain   grid ceil(R / QEI_COLS) x ceil(S / QEI_B): part_b(j) = sum_{s in block b} u(F_sj, m_s), s ascending from +0.0,
//                u(f, m) = (f > m) ? f - m : 0  (NaN and -Inf give 0; +Inf - finite = +Inf; no NaN is ever produced)
//   k_qei_pick   grid ceil(R / 256): tot(j) = sum_b part_b(j), b ascending; gain(j) = tot(j) / S; a record per workgroup; the
//                workgroup whose arrival completes the count reduces the records to the first maximum above 0 (value descending,
//                index ascending: `better` of kernels_score.hip with the floor at 0), writes idx[k] / gain[k] and raises m by
//                column j*; when nothing is above 0 it raises the word and the kernels of every later round return at once
// The summation order (QEI_B = 32 draws per block, blocks ascending, one division) is part of the ABI and restated by
// tests/qei_reference.py; the width of a column block is not (a column never meets another one before the arg-max).  No
// workgroup waits for another: the last arriver reads data that is complete (agent-scope release / acquire, as the rounds of
// the pruned arg-max in kernels_score.hip).  There is no multiply, so contraction has nothing to fuse; the pragma stays as a guard.
#include "common.h"   // (`better`, block_argmax come from kernels_score.hip, included before)

namespace bohip {

constexpr int QEI_B = 32;       // draws per block of the summation order (ABI)
constexpr int QEI_COLS = 128;   // candidates per workgroup of k_qei_gain: R = 4096, S = 256 is 32 x 8 = 256 workgroups, one per CU
constexpr int QEI_PICK = 256;   // candidates per workgroup of k_qei_pick

struct QeiWs {
    double* m;            // [S] the running maximum of every draw
    double* part;         // [ceil(S / QEI_B)][R]
    Best* tile;           // [ceil(R / QEI_PICK)] records of the round
    double* gain;         // [q]
    long long* idx;       // [q]
    unsigned* done;       // nothing can win any more
    unsigned* arrive;     // arrivals of the round's k_qei_pick workgroups (left at zero)
};

__global__ __launch_bounds__(256) void k_qei_init(QeiWs w, int64_t S, double tau, int64_t q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < S) w.m[i] = tau;
    if (i < q) { w.idx[i] = -1; w.gain[i] = 0.0; }
    if (i == 0) { *w.done = 0u; *w.arrive = 0u; }
}

__global__ __launch_bounds__(QEI_COLS) void k_qei_gain(const double* __restrict__ F, int64_t R, int64_t S, QeiWs w) {
#pragma clang fp contract(off)
    if (*w.done) return;
    const int64_t j = (int64_t)blockIdx.x * QEI_COLS + threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.y * QEI_B;
    if (j >= R) return;
    const double* __restrict__ m = w.m;
    const double* __restrict__ col = F + s0 * R + j;
    double acc = 0.0;
    if (s0 + QEI_B <= S) {   // a full block: the 32 loads are issued together
        double f[QEI_B];
#pragma unroll
        for (int i = 0; i < QEI_B; ++i) f[i] = col[(int64_t)i * R];
#pragma unroll
        for (int i = 0; i < QEI_B; ++i) {
            const double ms = m[s0 + i];
            acc += (f[i] > ms) ? f[i] - ms : 0.0;
        }
    } else {
        const int n = (int)(S - s0);
        for (int i = 0; i < n; ++i) {
            const double fi = col[(int64_t)i * R], ms = m[s0 + i];
            acc += (fi > ms) ? fi - ms : 0.0;
        }
    }
    w.part[(int64_t)blockIdx.y * R + j] = acc;
}

__global__ __launch_bounds__(QEI_PICK) void k_qei_pick(const double* __restrict__ F, int64_t R, int64_t S, int64_t k, QeiWs w) {
#pragma clang fp contract(off)
    __shared__ Best sh[QEI_PICK / 64];
    __shared__ Best win;
    __shared__ unsigned flag;
    if (*w.done) return;
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * QEI_PICK + tid;
    const int64_t NB = (S + QEI_B - 1) / QEI_B;
    double v = 0.0;
    long long idx = -1;
    if (j < R) {
        double tot = 0.0;
        for (int64_t b = 0; b < NB; ++b) tot += w.part[b * R + j];
        const double gn = tot / (double)S;
        if (gn > 0.0) { v = gn; idx = j; }
    }
    block_argmax(v, idx, sh);
    // the round's hand-over, agent-scope release / acquire: one lane publishes the workgroup's record, releases and adds to the
    // counter; the workgroup whose arrival completes the count acquires and finishes the round -- it waits for nobody
    if (tid == 0) {
        __hip_atomic_store(&w.tile[blockIdx.x].val, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&w.tile[blockIdx.x].idx, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const bool last = __hip_atomic_fetch_add(w.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
        if (last) __hip_atomic_store(w.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        flag = last;
    }
    __syncthreads();
    if (!flag) return;
    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __syncthreads();
    v = 0.0;
    idx = -1;
    for (unsigned t = tid; t < gridDim.x; t += QEI_PICK) {
        const double tv = __hip_atomic_load(&w.tile[t].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long ti = __hip_atomic_load(&w.tile[t].idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (better(tv, ti, v, idx)) { v = tv; idx = ti; }
    }
    block_argmax(v, idx, sh);
    if (tid == 0) {
        win.val = v;
        win.idx = idx;
        if (idx < 0) {
            *w.done = 1u;   // idx[k..] = -1 and gain[k..] = 0 are what k_qei_init left
        } else {
            w.idx[k] = idx;
            w.gain[k] = v;
        }
    }
    __syncthreads();
    const long long js = win.idx;
    if (js < 0) return;
    for (int64_t s = tid; s < S; s += QEI_PICK) {
        const double f = F[s * R + js];
        if (f > w.m[s]) w.m[s] = f;
    }
}

}  // namespace bohip
