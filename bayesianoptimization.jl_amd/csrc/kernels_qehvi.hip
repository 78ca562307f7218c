// kernels_qehvi.hip -- greedy Monte-Carlo q-EHVI for two objectives over two resident S x R matrices of joint draws
// (include/bohip_qehvi.h):
//     qEHVI(B) ~ (1/S) sum_s [HV(front + {(F0_sj, F1_sj), j in B}) - HV(front)],
// maximised greedily: every draw s keeps a staircase T_s that starts as the front; every round scores every candidate by the
// sample average of the area its point adds to T_s, takes the first maximum and folds the winner's point into every T_s.
// A staircase of L points is stored as L + 2 ELEMENTS of two doubles, element e = (c_e, b_{e+1}): c_0 = r1, c_{L+1} = +Inf,
// b_{L+1} = r2 (the second half of element L + 1 is r2 too and never read as a height).  Strip i = e + 1 spans [c_e, c_{e+1}] above
// b_{e+1}, so one 16-byte read per strip feeds the walk: the corner it brings closes the strip before, the height opens its own.
//   k_qehvi_init    every T_s = the front, lengths = n, idx = -1, gain = 0, the two control words cleared
//   k_qehvi_gain    grid ceil(R / QEHVI_COLS) x ceil(S / QEHVI_B), thread = candidate (consecutive lanes read consecutive doubles of a
//                   draw's row); the 32 + 32 entries of a full block are loaded together.  The staircase of the current draw is brought
//                   into LDS by LDS-DMA (16 bytes a lane, no VGPRs), two buffers: the next draw's copy is issued before this draw's walk
//                   and waited for after it.  (As compiled today the copy is not hidden: the compiler, which does not know the two
//                   buffers apart, waits for it before the walk's first LDS read; profiles/qehvi_times.txt.  Reading LDS through asm
//                   is the open step.)  In the walk every lane reads the SAME element: a broadcast, no bank conflict.  Heights
//                   descend and corners ascend, so the strips with a non-zero term form one interval per lane; NARROW walks the wave's
//                   union of them (two binary searches a lane, a wave min / max).  Zero terms are bit-neutral: both forms give the
//                   same bytes.  The full walk is the faster one at n = 64 and at n = 1024 (profiles/qehvi_times.txt has the two side
//                   by side: the union over 64 unrelated candidates covers most strips) and is what the library launches.
//   k_qehvi_pick    k_qei_pick's hand-over: tot, gain, a record per workgroup, agent-scope release / acquire, the last arriver
//                   reduces the records with `better`, writes idx[k] / gain[k] or raises the "nothing can win" word
//   k_qehvi_update  one wave per draw: p = column idx[k] of the draw; the old staircase goes to LDS, ballots over lanes striding it
//                   count the points left of p, the run p dominates and whether a point dominates p; the new staircase is written
//                   from the LDS copy (never an in-place shift).  Vector stores only.
// The summation order (QEHVI_B = 32 draws per block, blocks ascending, strips ascending inside a draw, one division) is part of
// the ABI and restated exactly by tests/qehvi_reference.py.  No workgroup waits for another.
#include "common.h"   // (`better`, block_argmax: kernels_score.hip; gbl_void_ptr / lds_void_ptr: gemm_core.h -- both included before)

namespace bohip {

constexpr int QEHVI_B = 32;       // draws per block of the summation order (ABI)
constexpr int QEHVI_COLS = 128;   // candidates per workgroup of k_qehvi_gain
constexpr int QEHVI_PICK = 256;   // candidates per workgroup of k_qehvi_pick
constexpr int QEHVI_QMAX = 16;
constexpr int QEHVI_ELEMS_MAX = MO_FRONT_MAX + QEHVI_QMAX + 2;   // elements of the longest staircase (1042)

struct QehviWs {
    double* st;           // [S][ST] elements of two doubles, rows 16-byte aligned
    double* front;        // [2 n + 3] c_0 .. c_{n+1}, b_1 .. b_{n+1} as mo_make_front lays them out
    int* len;             // [S] points of every staircase
    double* part;         // [ceil(S / QEHVI_B)][R]
    Best* tile;           // [ceil(R / QEHVI_PICK)] records of the round
    double* gain;         // [q]
    long long* idx;       // [q]
    unsigned* done;       // nothing can win any more
    unsigned* arrive;     // arrivals of the round's k_qehvi_pick workgroups (left at zero)
    int ST;               // elements a row holds: n + q + 2
    double r1, r2;
};

__global__ __launch_bounds__(256) void k_qehvi_init(QehviWs w, int64_t S, int n, int64_t q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < S * w.ST) {
        const int e = (int)(i % w.ST);
        w.st[2 * i] = e <= n + 1 ? w.front[e] : INFINITY;
        w.st[2 * i + 1] = e <= n ? w.front[n + 2 + e] : w.r2;
    }
    if (i < S) w.len[i] = n;
    if (i < q) { w.idx[i] = -1; w.gain[i] = 0.0; }
    if (i == 0) { *w.done = 0u; *w.arrive = 0u; }
}

// LDS doubles of one staging buffer: the elements rounded up to whole workgroup passes of the copy (a lane past the end re-reads
// the row's last element into the padding, so every lane of a pass is active and every global read is inside the row)
__host__ __device__ inline int qehvi_buf_doubles(int ST) { return 2 * ((ST + QEHVI_COLS - 1) / QEHVI_COLS * QEHVI_COLS); }

template <bool NARROW>
__global__ __launch_bounds__(QEHVI_COLS) void k_qehvi_gain(const double* __restrict__ F0, const double* __restrict__ F1, int64_t R, int64_t S,
                                                           QehviWs w) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double qehvi_stair[];   // [2][qehvi_buf_doubles(ST)]
    if (*w.done) return;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t j = (int64_t)blockIdx.x * QEHVI_COLS + tid;
    const int64_t jc = j < R ? j : R - 1;   // (a lane past R walks the last candidate and stores nothing: the barriers need it)
    const int64_t s0 = (int64_t)blockIdx.y * QEHVI_B;
    const int nd = (int)(S - s0 < QEHVI_B ? S - s0 : QEHVI_B);
    const int bufd = qehvi_buf_doubles(w.ST);
    const double r1 = w.r1, r2 = w.r2;
    const double* __restrict__ col0 = F0 + s0 * R + jc;
    const double* __restrict__ col1 = F1 + s0 * R + jc;

    // elements 0 .. len + 1 of draw s0 + i into buffer i & 1: asynchronous, waited for by `landed`
    auto stage = [&](int i) {
        const int64_t s = s0 + i;
        const int ne = min(w.len[s] + 2, w.ST);
        const double* row = w.st + s * 2 * w.ST;
        double* dst = qehvi_stair + (i & 1) * bufd + 2 * 64 * wave;
        for (int base = 0; base < ne; base += QEHVI_COLS) {
            const int e = min(base + tid, w.ST - 1);
            __builtin_amdgcn_global_load_lds((gbl_void_ptr)(row + 2 * e), (lds_void_ptr)(dst + 2 * base), 16, 0, 0);
        }
    };
    auto landed = [&] {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    // u_s of the point (a, b) over the staircase in buffer i & 1
    auto improvement = [&](int i, double a, double b) -> double {
        const int L = min(w.len[s0 + i], w.ST - 2);
        const double2* el = reinterpret_cast<const double2*>(qehvi_stair + (i & 1) * bufd);
        const bool ok = a - a == 0.0 && b - b == 0.0 && a > r1 && b > r2;   // (x - x == 0: x is finite)
        int e0 = 0, e1 = L;   // strips e0 + 1 .. e1 + 1
        if (NARROW) {
            // lane: lo_b = elements e in [0, L] with b_{e+1} >= b (heights descend: the first strip with h > 0 is lo_b + 1);
            //       lo_c = elements e in [0, L] with c_e < a (corners ascend: the last strip with w > 0 is lo_c)
            int lb = 0, hb = L + 1, lc = 0, hc = L + 1;
            while (__any(lb < hb || lc < hc)) {
                if (lb < hb) {
                    const int m = (lb + hb) >> 1;
                    if (el[m].y >= b) lb = m + 1; else hb = m;
                }
                if (lc < hc) {
                    const int m = (lc + hc) >> 1;
                    if (el[m].x < a) lc = m + 1; else hc = m;
                }
            }
            int lo = ok ? lb : L + 1, hi = ok ? lc - 1 : -1;
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, __shfl_xor(lo, o));
                hi = max(hi, __shfl_xor(hi, o));
            }
            e0 = __builtin_amdgcn_readfirstlane(lo);
            e1 = __builtin_amdgcn_readfirstlane(min(hi, L));
        }
        double u = 0.0;
        if (e0 <= e1) {
            double2 cur = el[e0];
            for (int e = e0; e <= e1; ++e) {
                const double2 nxt = el[e + 1];
                const double wd = (a > cur.x) ? fmin(a, nxt.x) - cur.x : 0.0;
                const double ht = (b > cur.y) ? b - cur.y : 0.0;
                const double t = (wd > 0.0 && ht > 0.0) ? wd * ht : 0.0;
                u += t;
                cur = nxt;
            }
        }
        return ok ? u : 0.0;
    };

    double acc = 0.0;
    if (nd == QEHVI_B) {   // a full block: the 32 + 32 loads are issued together, ahead of the first staircase
        double f0[QEHVI_B], f1[QEHVI_B];
#pragma unroll
        for (int i = 0; i < QEHVI_B; ++i) { f0[i] = col0[(int64_t)i * R]; f1[i] = col1[(int64_t)i * R]; }
        stage(0);
        landed();
#pragma unroll
        for (int i = 0; i < QEHVI_B; ++i) {
            if (i + 1 < QEHVI_B) stage(i + 1);
            acc += improvement(i, f0[i], f1[i]);
            landed();
        }
    } else {
        stage(0);
        landed();
        for (int i = 0; i < nd; ++i) {
            const double a = col0[(int64_t)i * R], b = col1[(int64_t)i * R];
            if (i + 1 < nd) stage(i + 1);
            acc += improvement(i, a, b);
            landed();
        }
    }
    if (j < R) w.part[(int64_t)blockIdx.y * R + j] = acc;
}

__global__ __launch_bounds__(QEHVI_PICK) void k_qehvi_pick(int64_t R, int64_t S, int64_t k, QehviWs w) {
#pragma clang fp contract(off)
    __shared__ Best sh[QEHVI_PICK / 64];
    __shared__ unsigned flag;
    if (*w.done) return;
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * QEHVI_PICK + tid;
    const int64_t NB = (S + QEHVI_B - 1) / QEHVI_B;
    double v = 0.0;
    long long idx = -1;
    if (j < R) {
        double tot = 0.0;
        for (int64_t b = 0; b < NB; ++b) tot += w.part[b * R + j];
        const double gn = tot / (double)S;
        if (gn > 0.0) { v = gn; idx = j; }
    }
    block_argmax(v, idx, sh);
    // the round's hand-over, agent-scope release / acquire (k_qei_pick): one lane publishes the workgroup's record, releases and adds
    // to the counter; the workgroup whose arrival completes the count acquires and finishes the round -- it waits for nobody
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
    for (unsigned t = tid; t < gridDim.x; t += QEHVI_PICK) {
        const double tv = __hip_atomic_load(&w.tile[t].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long ti = __hip_atomic_load(&w.tile[t].idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (better(tv, ti, v, idx)) { v = tv; idx = ti; }
    }
    block_argmax(v, idx, sh);
    if (tid == 0) {
        if (idx < 0) {
            *w.done = 1u;   // idx[k..] = -1 and gain[k..] = 0 are what k_qehvi_init left
        } else {
            w.idx[k] = idx;
            w.gain[k] = v;
        }
    }
}

// one wave per draw: fold the point of column idx[k] into the draw's staircase
__global__ __launch_bounds__(64) void k_qehvi_update(const double* __restrict__ F0, const double* __restrict__ F1, int64_t R, int64_t k,
                                                     QehviWs w) {
    extern __shared__ __attribute__((aligned(16))) double qehvi_old[];   // [ST] elements
    if (*w.done) return;
    const long long js = w.idx[k];
    if (js < 0) return;
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const double a = F0[s * R + js], b = F1[s * R + js];
    if (!(a - a == 0.0 && b - b == 0.0 && a > w.r1 && b > w.r2)) return;
    const int L = min(w.len[s], w.ST - 2);
    if (L + 1 > w.ST - 2) return;   // (no room: cannot happen, round k holds at most n + k points)
    double2* row = reinterpret_cast<double2*>(w.st + s * 2 * w.ST);
    double2* old = reinterpret_cast<double2*>(qehvi_old);
    for (int e = lane; e <= L + 1; e += 64) old[e] = row[e];
    __syncthreads();
    // point i = 1 .. L is (c_i, b_i) = (old[i].x, old[i - 1].y)
    int nleft = 0, ndom = 0;
    bool covered = false;
    for (int base = 0; base < L; base += 64) {
        const int i = base + lane + 1;
        const bool in = i <= L;
        const double ci = in ? old[i].x : 0.0, bi = in ? old[i - 1].y : 0.0;
        covered = covered || __ballot(in && ci >= a && bi >= b) != 0ull;
        nleft += __popcll(__ballot(in && ci < a && bi > b));
        ndom += __popcll(__ballot(in && ci <= a && bi <= b));
    }
    if (covered) return;
    // new point i' = 1 .. L': i' <= nleft the old point i'; nleft + 1 the point p; beyond it the old point i' - 1 + ndom
    const int Ln = L - ndom + 1;
    auto c_new = [&](int i) -> double {   // i = 0 .. Ln + 1
        if (i == 0) return w.r1;
        if (i > Ln) return INFINITY;
        return i <= nleft ? old[i].x : i == nleft + 1 ? a : old[i - 1 + ndom].x;
    };
    auto b_new = [&](int i) -> double {   // i = 1 .. Ln + 2
        if (i > Ln) return w.r2;
        return i <= nleft ? old[i - 1].y : i == nleft + 1 ? b : old[i - 2 + ndom].y;
    };
    for (int e = nleft + lane; e <= Ln + 1; e += 64) row[e] = make_double2(c_new(e), b_new(e + 1));
    if (lane == 0) w.len[s] = Ln;
}

}  // namespace bohip
