// kernels_score.hip -- the acquisition hot path (rows A4-A7, A9 of SURVEY.md section 8):
//   k_kstar        cross-covariance K*' chunk [Rc][Npad] (candidate-major, contraction index contiguous)
//   k_trigemm_sq   V = W K* on FP64 MFMA with the sum-of-squares epilogue fused: V is never stored.
//                  Row N of W carries alpha', so the same contraction also yields mu - beta.
//   k_score        sigma^2 = max(s_f^2 - sum v^2, 0), the reference's acquisition formulas verbatim,
//                  per-block arg-max;  k_argmax_final reduces to ONE 16-byte record.
//   k_thompson     S x R independent posterior draws with a counter-based normal generator.
// Reference call sites replaced: mean_var / predict_f (src/models/gp.jl:2-8), the functors of
// src/acquisitionfunctions.jl:24-27,47-50,96,111,141 with src/utils.jl:48-49, and the arg-max of
// acquire_max (src/acquisition.jl:54-68).
#include "gemm_core.h"
#include "acq_log.h"   // LogEI (ACQ_LOGEI)

namespace bohip {

// LOW: the Matérn 1/2 and 3/2 families, a compile-time choice as in kernels_linalg.hip's cov_from_r
template <bool LOW>
__device__ __forceinline__ double cov_from_r_fast(int fam, double sigma2, double r) {
    if constexpr (LOW) {
        return matern_lo_k(fam, sigma2, r);
    } else {
        if (fam == FAM_M52) {
            const double R = sqrt(r), s = sqrt(5.0) * R;
            return sigma2 * (1.0 + s + 5.0 / 3.0 * r) * exp(-s);
        }
        return sigma2 * exp(-0.5 * r);
    }
}

// ------------------------------------------------------------------------------------------------
// K*': thread = observation j (its coordinates live in registers), loop over the block's
// candidates whose coordinates are wave-uniform (scalar loads).  Stores are coalesced along j.
// KsT[r][j] = k(x_j, x*_r) for j < N, 0 for N <= j < Npad.  Xs is [R][d] (d contiguous).
// ------------------------------------------------------------------------------------------------
// PARTS (the pruned pass only, rb = 16): besides K*' the kernel leaves, per wave (64 observations) and candidate, the partial sums
// of p_j = alpha_j K*'_j and of |p_j| that k_prune_bound adds up -- the bound kernel then need not read K*' again.
//   parts[0][w][r] = sum of p over the observations 64 w .. 64 w + 63,  parts[1][w][r] = the same of |p|   (w < Npad / 64, r < ldp)
// Every partial has one writer and a fixed summation order (no atomics): the bounds are the same from run to run.
struct KstarParts {
    const double* alpha;     // the alpha row of W (zero past N), read for j < Npad
    double* parts;           // [2][Npad / 64][ldp]
    int64_t ldp;
};
// One value of K*': k(x_j, x*) from the observation's coordinates xj and weights w (registers; zero weight for d <= k < DT) and the
// candidate's coordinates xs (wave-uniform, in LDS); live = j < N, else the zero of the padding columns N <= j < Npad.  Every
// k_kstar instantiation goes through here, so a value does not depend on the instantiation that wrote it.
// (The PARTS launch stores all of K*', 100 MB a bench step, of which phase A and round 1 read 14 MB.  Storing only what is read and
// filling the tails of listed rows in two small launches was built and measured: the store is free -- the kernel is bound by
// VALU issue, ~85 instructions a value -- and the fills are 10 us on top.  profiles/prune_kstar_store_ab.txt)
template <int DT, bool LOW>
__device__ __forceinline__ double kstar_value(const double (&xj)[DT], const double (&w)[DT], const double* xs, bool live, int fam,
                                              double sigma2) {
    double rr = 0.0;
#pragma unroll
    for (int k = 0; k < DT; ++k) {
        const double t = xj[k] - xs[k];
        rr += w[k] * (t * t);
    }
    return live ? cov_from_r_fast<LOW>(fam, sigma2, rr) : 0.0;
}
// Sum over the wave's 64 lanes of 16 values per lane (one per candidate) by halving: a lane gives away half of what it holds and
// adds the other lane's half of the rest.  The candidates come four at a time (one group: their `exp`s overlap, and no more than
// a group's values are live): lane ^ 32 and ^ 16 take a group's 4 values to 1, lane ^ 8 two groups' values to 1 as soon as
// both are there, lane ^ 4 the two pairs' -- of candidate 8 b2 + 4 b3 + 2 b5 + b4 (b: the bits of the lane number), summed over the
// 16 lanes that share its bits 0 and 1; two plain steps finish.  17 exchanges for 16 sums instead of 16 x 6, and the first 8 of
// them move p itself: they serve the sum of p and the sum of |p| alike.
__device__ __forceinline__ void swap32(double a, double b, double& x, double& y) {
    // v_permlane32_swap: lanes 32-63 of the first operand change places with lanes 0-31 of the second.  Afterwards the lower half
    // holds (own a, the upper half's a) and the upper half (the lower half's b, own b): x + y is the sum of a in the lower and of b
    // in the upper half, |x| + |y| the same of the absolute values -- one exchange serves both.
    const unsigned long long ua = (unsigned long long)__double_as_longlong(a), ub = (unsigned long long)__double_as_longlong(b);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)ua, (unsigned)ub, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32), false, false);
    x = __longlong_as_double((long long)((unsigned long long)hi[0] << 32 | lo[0]));
    y = __longlong_as_double((long long)((unsigned long long)hi[1] << 32 | lo[1]));
}
template <int BIT>
__device__ __forceinline__ double halve_sum(double a, double b, int lane) {   // a where the lane's BIT is clear, b where it is set
    const bool up = lane & BIT;
    return (up ? b : a) + __shfl_xor(up ? a : b, BIT);
}
// a group's 4 products p -> the lane's sums of p and |p| of candidate 2 b5 + b4 of the group, over the lanes that share its bits 0-3
__device__ __forceinline__ void group_sum4(const double* p, int lane, double& sm, double& sa) {
    double x0, y0, x1, y1;
    swap32(p[0], p[2], x0, y0);
    swap32(p[1], p[3], x1, y1);
    sm = halve_sum<16>(x0 + y0, x1 + y1, lane);
    sa = halve_sum<16>(fabs(x0) + fabs(y0), fabs(x1) + fabs(y1), lane);
}
__device__ __forceinline__ double wave_finish(double s) {
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    return s;
}

template <int DT, bool LOW, bool PARTS = false>
__global__ __launch_bounds__(256) void k_kstar(const double* __restrict__ X, int64_t N, int64_t Npad,
                                               const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                               KernelHyper hp, double* __restrict__ KsT, int64_t ldk, int rb, KstarParts kp) {
    // the block's rb (<= 16) candidates are staged in LDS by one coalesced load (see k_build_cov: per-dimension scalar
    // loads behind `if (k < d)` made this kernel latency-bound); dimensions d <= k < DT carry zero weight
    __shared__ double xs_l[16 * DT];
    const int d = hp.d;
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    const int64_t r0 = r_begin + (int64_t)blockIdx.y * rb;
    const int64_t r1 = min(r0 + rb, r_end);
    for (int t = threadIdx.x; t < rb * DT; t += 256) {
        const int64_t r = r0 + t / DT;
        const int k = t % DT;
        xs_l[t] = (r < r1 && k < d) ? Xs[r * d + k] : 0.0;
    }
    double xj[DT], w[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) {
        xj[k] = (k < d && j < N) ? X[j * d + k] : 0.0;
        w[k] = k < d ? hp.il2[k] : 0.0;
    }
    __syncthreads();
    if (j >= Npad) return;
    const int nc = (int)(r1 - r0);
    if constexpr (PARTS) {
        // (Npad is a multiple of 64: a wave is either whole or gone at the return above)
        const double aj = kp.alpha[j];
        const int lane = threadIdx.x & 63;
        double um[2], ua[2], tm0 = 0.0, ta0 = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            double p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 4 * g + i;
                p[i] = 0.0;
                if (c < nc) {
                    const double v = kstar_value<DT, LOW>(xj, w, xs_l + c * DT, j < N, hp.fam, hp.sigma2);
                    KsT[(r0 + c - r_begin) * ldk + j] = v;
                    p[i] = aj * v;   // v exactly as stored
                }
            }
            double tm, ta;
            group_sum4(p, lane, tm, ta);
            if (g & 1) {
                um[g >> 1] = halve_sum<8>(tm0, tm, lane);
                ua[g >> 1] = halve_sum<8>(ta0, ta, lane);
            } else {
                tm0 = tm;
                ta0 = ta;
            }
            __builtin_amdgcn_sched_barrier(0);   // a group at a time: all 16 `exp`s scheduled together spill
        }
        const double sm = wave_finish(halve_sum<4>(um[0], um[1], lane)), sa = wave_finish(halve_sum<4>(ua[0], ua[1], lane));
        // of the four lanes that hold a candidate's sums, lane 4 q writes the sum of p and lane 4 q + 1 the sum of |p| (bit 1 clear:
        // a writer; bit 0: which sum): 16 doubles of one 128-B line per quantity and wave
        const int c = 8 * ((lane >> 2) & 1) + 4 * ((lane >> 3) & 1) + 2 * (lane >> 5) + ((lane >> 4) & 1);
        if ((lane & 3) < 2 && c < nc) {
            const int64_t P = Npad >> 6;
            kp.parts[((int64_t)(lane & 1) * P + (j >> 6)) * kp.ldp + (r0 + c - r_begin)] = (lane & 1) ? sa : sm;
        }
    } else {
        for (int c = 0; c < nc; ++c) {
            const double v = kstar_value<DT, LOW>(xj, w, xs_l + c * DT, j < N, hp.fam, hp.sigma2);
            KsT[(r0 + c - r_begin) * ldk + j] = v;   // plain stores: non-temporal ones evict K*' from L2/MALL and k_trigemm_sq
                                                       // then runs at 0.70 instead of 0.635 ms (measured)
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Full posterior covariance of R candidates (predict_f(gp, X; full_cov = true), the input of the reference's joint
// draw myrand(model, X::Matrix), src/models/gp.jl:7):  cov[r][s] = k(x*_r, x*_s) - (V'V)[r][s].
// VV holds the LOWER triangle of V'V (k_gemm_nt on the stored V'); both halves of cov are written from it so the
// result is exactly symmetric.  Thread = column s, block walks 16 rows.
// ------------------------------------------------------------------------------------------------
template <int DT, bool LOW>
__global__ __launch_bounds__(256) void k_post_cov(const double* __restrict__ Xs, int64_t R, KernelHyper hp,
                                                  const double* __restrict__ VV, int64_t ldv,
                                                  double* __restrict__ cov, int64_t ldc) {
    const int d = hp.d;
    const int64_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= R) return;
    double xs[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) xs[k] = (k < d) ? Xs[s * d + k] : 0.0;
    const int64_t r0 = (int64_t)blockIdx.y * 16, r1 = min(R, r0 + 16);
    for (int64_t r = r0; r < r1; ++r) {
        double rr = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                const double t = Xs[r * d + k] - xs[k];
                rr += hp.il2[k] * (t * t);
            }
        const double vv = (r >= s) ? VV[r * ldv + s] : VV[s * ldv + r];
        cov[r * ldc + s] = cov_from_r_fast<LOW>(hp.fam, hp.sigma2, rr) - vv;
    }
}

// ------------------------------------------------------------------------------------------------
// V = W K*, fused epilogue.  Tile (rt, ct): rows [128 rt, 128 rt + 128) of W against candidates
// [64 ct, 64 ct + 64) of the chunk; W is lower-triangular so the contraction stops at k = 128 (rt + 1).
// Job length is set by that K extent, so the candidate tile is only 64 wide: with 128-wide tiles the longest
// job (24 units at N=3000) exceeds the average load per workgroup slot (18.75) and list scheduling cannot
// balance.  Work per tile grows with rt, so tiles are issued heaviest-first; blocks are dealt to XCDs
// (block b runs on XCD b % 8) so that each XCD owns a fixed subset of candidate tiles and walks the
// row tiles together: the W row-tile stream is then shared through that XCD's L2.
// Output: q_part[rt][r] = sum over the tile's rows of v^2 (fixed summation order -> deterministic),
//         mu_raw[r] = alpha' k*_r taken from the row of W that stores alpha (alpha_row).
// ------------------------------------------------------------------------------------------------
struct AcqParams {
    int acq;
    double p0, p1;
};
// Fused finish of k_trigemm_sq (large batches, value-only scoring): the workgroup that delivers the LAST row tile of a
// candidate tile turns the T partial sums into sigma^2, the acquisition value and the tile's arg-max; the one that
// completes the last candidate tile reduces the per-tile records to the 16-byte result.  Replaces k_score +
// k_argmax_final (two launches, ~16 us of a 0.69 ms step).  Same summation order as k_score -> bit-identical scores.
// Cross-workgroup data (q_part, mu_raw, tile records) moves with agent-scope accesses; the counters are left at zero.
struct FuseParams {
    unsigned* tile_cnt;      // [candidate tiles of the whole batch]  arrivals per tile (nullptr: no fused finish)
    unsigned* total_cnt;     // [1] finished candidate tiles
    Best* tile_best;         // [candidate tiles]
    int tiles_total;         // candidate tiles of the whole batch (all chunks)
    int T;                   // row tiles (the finish adds two partial sums per tile)
    int64_t R_total;         // candidates of the whole batch
    double sigma2, beta;
    AcqParams ap;
    double *mu_out, *var_out, *score_out;   // nullable, indexed by the global candidate number
    Best* best_out;          // nullable: the batch's arg-max record
    long long best_off;      // added to the winner's index (sharded scoring)
    unsigned long long* clk; // nullable: [2] core-clock and 100 MHz wall-clock ticks summed over a sample of workgroups (timing runs)
    const unsigned* live;    // nullable: candidates of the chunk that exist, counted on the device (pruned scoring: the grid is sized
                             // for the worst case, candidate tiles at or past the count leave at once)
};
__device__ void trigemm_fused_finish(const FuseParams& fz, int tile_g, int T, const double* q_part, int64_t ldq,
                                     const double* mu_raw);

// BOHIP_TRACE (tools only, default 0 in gemm_core.h): per-workgroup start/end clocks of k_trigemm_sq (tools/trace_trigemm.py)
#if BOHIP_TRACE
__device__ unsigned long long g_trace[6 * 8192];   // per workgroup: wall start, wall end, HW_ID, XCC_ID, core-clock start, core-clock end
#endif
// ---- row pieces ------------------------------------------------------------------------------------------------------
// A job is one ROW PIECE of W against one 64-wide candidate tile.  A piece is a whole 128-row tile (job length = its K extent:
// rt + 1 units) or, for a last tile whose live rows all sit in its upper half (rows 64..127 are padding), those 64 rows alone, run
// in the loop's half mode (both wave rows work on the 64 rows, even / odd members of every contraction-index pair, partial sums
// added at the end).  The HOST lists the pieces heaviest-first (trigemm_pieces in bohip.hip; the list depends on the number of row
// tiles and the position of the alpha row ONLY, never on the batch: scores stay batch- and shard-independent) and the kernel reads
// its piece from that table.  Encoding: piece = rt | mode << 16.
// q_part holds TWO partial sums per row tile (rows 0..63 and 64..127, [2 rt + h][r]; a solo upper half writes zero for the lower
// one); the finish adds (q[2t] + q[2t+1]) tile by tile.
constexpr int PIECE_WHOLE = 0, PIECE_UPPER_SOLO = 3;

// The sum of squares of one 64-row half of V for one candidate, shared by k_trigemm_sq and k_trigemm_rows so that the two cannot
// differ in a bit (operand order, contraction of v * v + s): the lane of k = lane >> 4, b1 = (lane >> 3) & 1 adds the squares of
// rows 8 mi + 4 b1 + k of the half over mi = 0..7 in sequence (sq_step; the alpha row left out), then the butterflies over b1 and
// k (sq_tree) give every lane the half's sum.
__device__ __forceinline__ double sq_step(double s, double v) { return s + v * v; }
__device__ __forceinline__ double sq_tree(double s) {
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    return s;
}

// one job: row piece (rt, mode) of W against candidate tile ct of the chunk (all arguments wave-uniform)
__device__ __forceinline__ void trigemm_job(int rt, int mode, int ct, const double* __restrict__ W, int64_t ldw,
                                            const double* __restrict__ KsT, int64_t ldk, int NP, int64_t alpha_row,
                                            double* __restrict__ q_part, int64_t ldq, double* __restrict__ mu_raw, int64_t r_off,
                                            double* __restrict__ VT, int64_t ldv, const FuseParams& fz, double* smem, int tid) {
    constexpr int NJ = 4, CW = CTILE;
    double acc[8][NJ];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = 0.0;
    const int64_t row_base = (int64_t)rt * TILE;
    // rows past alpha' are padding; a half piece has at most 64 live rows (-> the loop's half mode)
    const int active_rows = (int)min((int64_t)(mode == PIECE_WHOLE ? TILE : TILE / 2), alpha_row + 1 - row_base);
    const int tri_kc = rt * (TILE / KC);                       // first chunk of the piece's triangular block
    const int kc_end = mode == PIECE_WHOLE ? (rt + 1) * (TILE / KC) : tri_kc + 4;
    gemm_tile_loop_glds3_ks<NJ, BOHIP_ABL, true>(W + row_base * ldw, ldw, KsT + (int64_t)ct * CW * ldk, ldk, 0, kc_end, smem, acc,
                                                 active_rows, tri_kc, tid);
    const int lane = tid & 63, wave = tid >> 6, wr = (wave & 3) >> 1, wc = wave & 1;
    __syncthreads();     // (the raw-barrier loops end on s_barrier; make the reuse of smem below explicit)
    double* red = smem;  // [2][CW]
    // half mode leaves the piece's 64 rows in wave row 0; wave row 1 holds zeros that belong to NO row of this piece
    const bool rows_mine = mode == PIECE_WHOLE || wr == 0;
    if (wave < 4) {
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
        double s = 0.0;
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            const int64_t grow = row_base + acc_row(lane, wr, mi);
            const double v = acc[mi][nj];
            if (grow == alpha_row && rows_mine) {
                __hip_atomic_store(mu_raw + r_off + (int64_t)ct * CW + acc_col<NJ>(lane, wc, nj), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                s = sq_step(s, v);
            }
            if (VT != nullptr && grow < alpha_row && rows_mine)
                VT[((int64_t)ct * CW + acc_col<NJ>(lane, wc, nj)) * ldv + grow] = v;
        }
        s = sq_tree(s);
        if (lane < 8) red[wr * CW + wc * 8 * NJ + 8 * nj + lane] = s;
    }
    }
    __syncthreads();
    if (tid < 2 * CW) {   // thread t < 64: the sum over the piece's first 64 rows; t >= 64: over rows 64..127 of a whole tile
        const int hh = tid >> 6, c = tid & (CW - 1);
        double* dst = q_part + (int64_t)(2 * rt + (mode == PIECE_WHOLE ? hh : 0)) * ldq + r_off + (int64_t)ct * CW + c;
        if (mode == PIECE_WHOLE || hh == 0) __hip_atomic_store(dst, red[hh * CW + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_store(dst + ldq, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // solo upper half: the lower one's slot is zero
    }
    if (fz.tile_cnt != nullptr) {
        __shared__ int s_last;
        const int tile_g = (int)(r_off / CW) + ct;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the agent-scope stores above have landed (a workgroup-scope fence emits no such wait)
        __syncthreads();
        if (tid == 0) s_last = atomicAdd(fz.tile_cnt + tile_g, 1u) == (unsigned)(NP - 1);
        __syncthreads();
        if (s_last && tid < 64) trigemm_fused_finish(fz, tile_g, fz.T, q_part, ldq, mu_raw);
    }
}

// 8 waves: the contraction index is halved inside the workgroup (gemm_tile_loop_glds3_ks)
__global__ __launch_bounds__(GEMM_THREADS_8, 4) void k_trigemm_sq(const double* __restrict__ W, int64_t ldw,
                                                                  const double* __restrict__ KsT, int64_t ldk,
                                                                  const int* __restrict__ pieces, int NP, int CT, int64_t alpha_row,
                                                                  double* __restrict__ q_part, int64_t ldq,
                                                                  double* __restrict__ mu_raw, int64_t r_off,
                                                                  double* __restrict__ VT, int64_t ldv, FuseParams fz) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
#if BOHIP_TRACE
    const unsigned long long t_start = wall_clock64(), c_start = clock64();
    struct TraceEnd {
        unsigned long long t0, c0;
        __device__ ~TraceEnd() {
            if (threadIdx.x == 0) {
                unsigned hw, xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                unsigned long long* t = g_trace + 6 * (size_t)blockIdx.x;
                t[0] = t0; t[1] = wall_clock64(); t[2] = hw; t[3] = xcc; t[4] = c0; t[5] = clock64();
            }
        }
    } trace_end{t_start, c_start};
#endif
    // blocks are dealt to XCDs round-robin (block b runs on XCD b % 8): an XCD owns the candidate tiles ct = xcd (mod 8) and
    // walks the row pieces together, heaviest first
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int n_local = (CT + 7) >> 3;
    const int ct = xcd + 8 * (slot % n_local);
    if (ct >= CT) return;
    if (fz.live != nullptr && ct * CTILE >= (int)*fz.live) return;
    const int piece = __builtin_amdgcn_readfirstlane(pieces[slot / n_local]);   // (uniform: a scalar load)
    // timing runs (bohip_gp_enable_timing): every 33rd workgroup reports how many core-clock cycles and 100 MHz ticks it lived --
    // their ratio is the clock the chip sustained UNDER THIS KERNEL (MI355X clocks to its power budget: ~2.0 of 2.4 GHz here)
    __shared__ unsigned long long s_clk[2];
    if (fz.clk != nullptr && blockIdx.x % 33 == 0 && threadIdx.x == 0) { s_clk[0] = clock64(); s_clk[1] = wall_clock64(); }
    trigemm_job(piece & 0xffff, piece >> 16, ct, W, ldw, KsT, ldk, NP, alpha_row, q_part, ldq, mu_raw, r_off, VT, ldv, fz, smem,
                    (int)threadIdx.x);
    if (fz.clk != nullptr && blockIdx.x % 33 == 0 && threadIdx.x == 0) {
        atomicAdd(fz.clk, (unsigned long long)clock64() - s_clk[0]);
        atomicAdd(fz.clk + 1, (unsigned long long)wall_clock64() - s_clk[1]);
    }
}

// ---- phase A of the pruned arg-max as 64-row jobs ----------------------------------------------------------------------------
// Phase A contracts the row tiles rt < m (m = 3 of 24 at N = 3000) against every candidate.  As whole-tile jobs that is 64 candidate
// tiles x 3 pieces = 192 workgroups on 256 CUs, and the launch lasts as long as its rt = m - 1 jobs, each alone on a CU and bound by
// the MFMA issue of two waves per SIMD.  Here every whole piece is cut into its two 64-row halves, each a workgroup of its own in
// the loop's WHOLE mode (gemm_tile_loop_glds3_ks<.., ROWS64>): the waves of wave row 0 compute what the waves of wave row hh of the
// whole-tile job compute -- same fragments, k-slot order, skip, khalf fold -- and sq_step / sq_tree run over the same lanes, so
// q_part[2 rt + hh] comes out bit for bit as k_trigemm_sq's (an element of an MFMA result depends on its own A row and B column
// only: the argument k_trigemm_rows rests on).  The upper half (hh = 0) ends at chunk 8 rt + 4: past it every row group of it is
// skipped.  A job of the prefix never holds the alpha row (m < T, checked by the host), so no mu is written.  No fused finish.
// jobs: rt | hh << 16 in launch order (host: phase_a_jobs); the XCD deal of k_trigemm_sq.
__device__ __forceinline__ void trigemm_job_rows64(int rt, int hh, int ct, const double* __restrict__ W, int64_t ldw,
                                                   const double* __restrict__ KsT, int64_t ldk, double* __restrict__ q_part,
                                                   int64_t ldq, double* smem, int tid) {
    constexpr int NJ = 4, CW = CTILE;
    double acc[8][NJ];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = 0.0;
    const int64_t row_base = (int64_t)rt * TILE + 64 * hh;
    const int tri_kc = rt * (TILE / KC);                       // first chunk of the tile's triangular block
    const int kc_end = tri_kc + (hh == 0 ? 4 : 8);
    gemm_tile_loop_glds3_ks<NJ, BOHIP_ABL, true, true, true>(W + row_base * ldw, ldw, KsT + (int64_t)ct * CW * ldk, ldk, 0, kc_end, smem,
                                                             acc, TILE / 2, tri_kc, tid, hh);
    const int lane = tid & 63, wave = tid >> 6, wc = wave & 1;
    __syncthreads();     // (the raw-barrier loops end on s_barrier; make the reuse of smem below explicit)
    double* red = smem;  // [CW]
    if (wave < 2) {      // khalf = 0, wave row 0: the half's 64 rows, folded
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) {
            double s = 0.0;
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) s = sq_step(s, acc[mi][nj]);
            s = sq_tree(s);
            if (lane < 8) red[wc * 8 * NJ + 8 * nj + lane] = s;
        }
    }
    __syncthreads();
    if (tid < CW)
        __hip_atomic_store(q_part + (int64_t)(2 * rt + hh) * ldq + (int64_t)ct * CW + tid, red[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(GEMM_THREADS_8, 4) void k_trigemm_sq_pa(const double* __restrict__ W, int64_t ldw,
                                                                     const double* __restrict__ KsT, int64_t ldk,
                                                                     const int* __restrict__ jobs, int CT, double* __restrict__ q_part,
                                                                     int64_t ldq, unsigned long long* clk) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
#if BOHIP_TRACE
    const unsigned long long t_start = wall_clock64(), c_start = clock64();
    struct TraceEnd {
        unsigned long long t0, c0;
        __device__ ~TraceEnd() {
            if (threadIdx.x == 0) {
                unsigned hw, xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                unsigned long long* t = g_trace + 6 * (size_t)blockIdx.x;
                t[0] = t0; t[1] = wall_clock64(); t[2] = hw; t[3] = xcc; t[4] = c0; t[5] = clock64();
            }
        }
    } trace_end{t_start, c_start};
#endif
    // an XCD owns the candidate tiles ct = xcd (mod 8) and walks the jobs together, in the table's order (see k_trigemm_sq)
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int n_local = (CT + 7) >> 3;
    const int ct = xcd + 8 * (slot % n_local);
    if (ct >= CT) return;
    const int job = __builtin_amdgcn_readfirstlane(jobs[slot / n_local]);   // (uniform: a scalar load)
    // timing runs: the sampled core clock, as in k_trigemm_sq
    __shared__ unsigned long long s_clk[2];
    if (clk != nullptr && blockIdx.x % 33 == 0 && threadIdx.x == 0) { s_clk[0] = clock64(); s_clk[1] = wall_clock64(); }
    trigemm_job_rows64(job & 0xffff, job >> 16, ct, W, ldw, KsT, ldk, q_part, ldq, smem, (int)threadIdx.x);
    if (clk != nullptr && blockIdx.x % 33 == 0 && threadIdx.x == 0) {
        atomicAdd(clk, (unsigned long long)clock64() - s_clk[0]);
        atomicAdd(clk + 1, (unsigned long long)wall_clock64() - s_clk[1]);
    }
}

// ---- split-K path for batches with too few candidate tiles to fill the chip (a few hundred candidates) -------------
// With one 64-wide candidate tile column per 64 candidates the longest job (the last row tile, K = N) runs alone on one
// CU: ~9 us per 128 of K, 215 us at N = 3000 whatever R.  Here the contraction index is cut into slices of kz chunks,
// k_gemm_nt computes the partial V' = K*' W' tiles of every slice in one batched launch (planes PT[s][r][i]), and this
// kernel adds the slices of a candidate in slice order, squares, and reduces: q[r], mu_raw[r], optionally V' itself.
// One workgroup per candidate; fixed summation order -> independent of the batch.
__global__ __launch_bounds__(256) void k_split_combine_v(const double* __restrict__ PT, int64_t plane, int64_t ldp, int kz,
                                                         int64_t N, double* __restrict__ q, double* __restrict__ mu_raw,
                                                         double* __restrict__ VT, int64_t ldv) {
    __shared__ double red[256];
    const int r = blockIdx.x;
    const double* base = PT + (int64_t)r * ldp;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i <= N; i += 256) {
        const int nsl = (int)(((i >> 7) + 1) * (TILE / KC) + kz - 1) / kz;   // slices that reach row tile i / 128
        double v = 0.0;
        for (int sl = 0; sl < nsl; ++sl) v += base[(int64_t)sl * plane + i];
        if (i < N) {
            s += v * v;
            if (VT) VT[(int64_t)r * ldv + i] = v;
        } else {
            mu_raw[r] = v;   // the alpha row
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) q[r] = red[0];
}
// U'[r][j] = sum over the slices that reach column tile j / 128 (i >= j) of the partial planes
__global__ __launch_bounds__(256) void k_split_combine_u(const double* __restrict__ PU, int64_t plane, int64_t ldp, int kz,
                                                         int nslices, int64_t N, double* __restrict__ UT, int64_t ldu) {
    const int r = blockIdx.x;
    const double* base = PU + (int64_t)r * ldp;
    for (int64_t j = threadIdx.x; j < N; j += 256) {
        const int s0 = (int)((j >> 7) * (TILE / KC)) / kz;   // first slice whose range ends beyond the start of the column tile
        double v = 0.0;
        for (int sl = s0; sl < nslices; ++sl) v += base[(int64_t)sl * plane + j];
        UT[(int64_t)r * ldu + j] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// Acquisition functors -- verbatim operation order of the reference, contraction OFF (Julia never
// fuses a*b+c).  normal_pdf / normal_cdf: src/utils.jl:48-49.
// ------------------------------------------------------------------------------------------------
// LOGEI = false compiles the LogEI call out: for the two kernel families that already spill (k_ascent_wg<16, .>, k_small_u<64, 4, .>),
// where even the call cost 4-12 bytes of scratch more; their LogEI work runs in instantiations of its own (profiles/logei_resources.txt).
template <bool LOGEI = true>
__device__ __forceinline__ double acq_eval(const AcqParams& a, double mu, double s2) {
#pragma clang fp contract(off)
    switch (a.acq) {
        case ACQ_EI: {  // src/acquisitionfunctions.jl:47-50  (D*Phi + sqrt(s2)*pdf  ==  D*Phi(z) + phi(z))
            const double tau = a.p0;
            if (s2 == 0.0) return mu > tau ? mu - tau : 0.0;
            const double D = mu - tau;
            const double cdf = 1.0 / 2.0 * (1.0 + erf(D / sqrt(2.0 * s2)));
            const double pdf = 1.0 / sqrt(2.0 * M_PI * s2) * exp(-(D * D) / (2.0 * s2));
            return D * cdf + sqrt(s2) * pdf;
        }
        case ACQ_PI: {  // :24-27
            const double tau = a.p0;
            if (s2 == 0.0) return mu > tau ? 1.0 : 0.0;
            return 1.0 / 2.0 * (1.0 + erf((mu - tau) / sqrt(2.0 * s2)));
        }
        case ACQ_UCB:  // :96
            return mu + a.p0 * sqrt(s2);
        case ACQ_MI:  // :141
            return mu + a.p0 * (sqrt(s2 + a.p1) - sqrt(a.p1));
        case ACQ_LOGEI:  // an extension (acq_log.h): log of the textbook EI, p0 = tau
            if constexpr (LOGEI) return logei_value(mu, s2, a.p0);
            else return NAN;   // (never launched with this id: a NaN never wins)
        default:  // MaxMean :111
            return mu;
    }
}

// (value desc, index asc); NaN never wins (reference: `f > maxf` is false for NaN).
__device__ __forceinline__ bool better(double v, long long i, double bv, long long bi) {
    if (i < 0) return false;
    if (bi < 0) return v > -INFINITY;
    return v > bv || (v == bv && i < bi);
}
__device__ __forceinline__ void block_argmax(double& v, long long& i, Best* sh) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const long long oi = __shfl_xor(i, o);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[wave].val = v; sh[wave].idx = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            if (better(sh[w].val, sh[w].idx, v, i)) { v = sh[w].val; i = sh[w].idx; }
    }
}

// one wave: the 64 candidates of tile tile_g (see FuseParams)
__device__ void trigemm_fused_finish(const FuseParams& fz, int tile_g, int T, const double* q_part, int64_t ldq,
                                     const double* mu_raw) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)tile_g * CTILE + lane;
    double v = -INFINITY;
    long long idx = -1;
    if (r < fz.R_total) {
        double q = 0.0;
        for (int t = 0; t < T; ++t)   // (upper half + lower half) tile by tile: what a whole-tile job used to store as ONE number
            q += __hip_atomic_load(q_part + (int64_t)(2 * t) * ldq + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) +
                 __hip_atomic_load(q_part + (int64_t)(2 * t + 1) * ldq + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double s2 = fz.sigma2 - q;
        if (s2 < 0.0) s2 = 0.0;  // predict_f: max(sigma2, 0)
        const double mu = fz.beta + __hip_atomic_load(mu_raw + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fz.mu_out) fz.mu_out[r] = mu;
        if (fz.var_out) fz.var_out[r] = s2;
        const double f = acq_eval(fz.ap, mu, s2);
        if (fz.score_out) fz.score_out[r] = f;
        if (f > -INFINITY) { v = f; idx = r; }  // false for NaN and -Inf
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const long long oi = __shfl_xor(idx, o);
        if (better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
    int last = 0;
    if (lane == 0) {
        fz.tile_cnt[tile_g] = 0u;   // ready for the next call
        if (fz.best_out) {
            __hip_atomic_store(&fz.tile_best[tile_g].val, idx >= 0 ? v : -INFINITY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&fz.tile_best[tile_g].idx, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile record stored before it is counted
            last = atomicAdd(fz.total_cnt, 1u) == (unsigned)(fz.tiles_total - 1);
        }
    }
    last = __shfl(last, 0);
    if (!last) return;
    v = -INFINITY;
    idx = -1;
    for (int i = lane; i < fz.tiles_total; i += 64) {
        const double bv = __hip_atomic_load(&fz.tile_best[i].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long bi = __hip_atomic_load(&fz.tile_best[i].idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (better(bv, bi, v, idx)) { v = bv; idx = bi; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const long long oi = __shfl_xor(idx, o);
        if (better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
    if (lane == 0) {
        *fz.total_cnt = 0u;
        fz.best_out->val = idx >= 0 ? v : -INFINITY;
        fz.best_out->idx = idx >= 0 ? idx + fz.best_off : -1;
    }
}

// T > 0: T row tiles with TWO partial sums each ([2 t], [2 t + 1]: k_trigemm_sq's layout); T = 0: q_part[r] is the finished sum
// (row-wise and split-K paths)
__global__ __launch_bounds__(256) void k_score(const double* __restrict__ q_part, int64_t ldq, int T,
                                               const double* __restrict__ mu_raw, int64_t R, double sigma2,
                                               double beta, AcqParams ap, double* __restrict__ mu_out,
                                               double* __restrict__ var_out, double* __restrict__ score_out,
                                               Best* __restrict__ block_best) {
#pragma clang fp contract(off)
    __shared__ Best sh[4];
    const int64_t r = blockIdx.x * 256 + threadIdx.x;
    double v = -INFINITY;
    long long idx = -1;
    if (r < R) {
        double q = 0.0;
        for (int t = 0; t < T; ++t) q += q_part[(int64_t)(2 * t) * ldq + r] + q_part[(int64_t)(2 * t + 1) * ldq + r];
        if (T == 0) q = q_part[r];
        double s2 = sigma2 - q;
        if (s2 < 0.0) s2 = 0.0;  // predict_f: max(sigma2, 0)
        const double mu = beta + mu_raw[r];
        if (mu_out) mu_out[r] = mu;
        if (var_out) var_out[r] = s2;
        const double f = acq_eval(ap, mu, s2);
        if (score_out) score_out[r] = f;
        if (f > -INFINITY) { v = f; idx = r; }  // false for NaN and -Inf
    }
    if (block_best) {
        block_argmax(v, idx, sh);
        if (threadIdx.x == 0) { block_best[blockIdx.x].val = idx >= 0 ? v : -INFINITY; block_best[blockIdx.x].idx = idx; }
    }
}

// idx_off: global column of this shard's first candidate (sharded scoring: the record leaves the kernel ready for the exchange)
__global__ __launch_bounds__(256) void k_argmax_final(const Best* __restrict__ in, int n, Best* __restrict__ out, long long idx_off) {
    __shared__ Best sh[4];
    double v = -INFINITY;
    long long idx = -1;
    for (int i = threadIdx.x; i < n; i += 256)
        if (better(in[i].val, in[i].idx, v, idx)) { v = in[i].val; idx = in[i].idx; }
    block_argmax(v, idx, sh);
    if (threadIdx.x == 0) { out->val = idx >= 0 ? v : -INFINITY; out->idx = idx >= 0 ? idx + idx_off : -1; }
}

// ---- pruned arg-max (value-only calls, bohip.hip pruned_pass) ---------------------------------------------------------------
// A call that returns only the winner need not contract the rows of candidates that provably cannot win.  After the first m row
// tiles (phase A: k_trigemm_sq_pa over the 64-row halves of the row pieces with rt < m, all candidates) every candidate gets an UPPER BOUND of the score
// the full pass would compute for it (k_prune_bound).  Round 1 scores the 64 candidates of highest bound exactly (k_prune_select:
// the first 64 in (bound desc, index asc) -- of the candidates that share the 64th bound, the lowest indices); its best value
// L is an exactly computed score.  Round 2 scores exactly every other candidate whose bound is not below L.  A dropped candidate
// has score <= bound < L, so it can neither win nor tie: the record equals the full pass's bit for bit (the exact rounds compute
// every element of V with k_trigemm_sq's MFMA chain -- k_trigemm_rows, or k_trigemm_sq itself on gathered K*' rows: a column of
// the contraction depends on its own K*' row only -- and add the partial sums in the fused finish's order).
//
// The bound, per candidate (u = 2^-53, n = Npad + 64 >= the number of terms of any summation of the alpha row):
//   s2_up = max(s_f^2 - sum_{t < m} (q[2t] + q[2t+1]), 0): every partial sum is >= 0 and rounded addition is monotone, so the prefix
//           done in the finish's order never exceeds the full q -- an upper bound of the computed sigma^2 with no margin.
//   mu_up = beta + up(mu~ + 4 gamma_n S) (rounded up by >= 1 ulp), mu~ = sum_j alpha_j K*'_j, S = sum_j |alpha_j K*'_j| (any order): the computed
//           mu_raw and mu~ both lie within gamma_n S(1 + gamma_n) of the exact dot product; beta + . is monotone.
//           mu~ and S are not summed over K*' here: k_kstar<.., PARTS> leaves the sums of every 64 observations (one wave; its
//           halving tree) and k_prune_bound adds those Npad / 64 partials in index order.  A two-level sum of the same Npad <= n
//           terms is one of the orders the argument covers (any summation of at most n terms lies within gamma_n S), so n stays.
//   functor f at (mu_up, s2_b), plus a slack for its evaluation where its operations are not exactly monotone:
//     EI  (the reference's D Phi(D/s) + phi(D/s)): in s it rises up to s = 1 and falls after; at s <= 1 it rises in D for D <= 0, at
//         s = 1 for every D.  So s2_b = min(s2_up, 1) when D_up <= 0, else 1 (a computed sigma^2 of 0 gives max(D, 0) <= both).
//         Slack 2^-38 (1 + s_f + max(D_up, 0) + |f|): erf / exp and the cancellation in 1 + erf err by ~1e-15 absolute in Phi
//         and relative in phi, times |D| <= 8 s_f where Phi is not negligible (Mills' ratio covers the rest) -- ~100x head-room.
//     PI  D_up >= 0: 1; else f(mu_up, s2_up) + 2^-38.
//     UCB, MI: s2_b = s2_up for p0 >= 0, 0 for p0 < 0; slack 2^-38 (|mu_up| + |p0| (sqrt terms)) for the square roots.
//     MaxMean: mu_up (one rounded addition: exact).
//     LogEI (acq_log.h): log sigma + log h(z) rises in mu and, its partial phi / (2 s2 h) being positive, in sigma^2: s2_b = s2_up,
//         which is never below the computed sigma^2 (above: no margin needed, the same fact UCB's bound rests on).  Slack
//         2^-38 (1 + |f|): the two logarithms err by a few ulp of at most 745 + |f| each, h by <= 20 ulp at the branch switch --
//         under 1e-12 absolute in all, ~4x head-room at f = 0 and more as |f| grows.  f = -inf (sigma^2 = 0, mu_up <= tau) stays -inf.
// A NaN bound is never below L: such a candidate is always scored.
struct PruneBound {
    const double* parts;     // k_kstar's partial sums [2][P][ldp]: of alpha_j K*'_j and of its absolute value, per 64 observations
    int64_t P, ldp, Npad;
    const double* q;         // k_trigemm_sq's partial sums [2 t + h][ldq], t < m filled by phase A
    int64_t ldq, R;
    int m;
    double sigma2, beta;
    AcqParams ap;
    double* ub;              // [R]
};
// thread = candidate (the partials are contiguous in r: every load is coalesced)
__global__ __launch_bounds__(64) void k_prune_bound(PruneBound pb) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= pb.R) return;
    double mu = 0.0, sa = 0.0;
    for (int64_t w0 = 0; w0 < pb.P; w0 += 16) {   // index order: a fixed two-level sum of the Npad terms; 32 loads in flight
        double a[16], b[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t w = min(w0 + i, pb.P - 1);
            a[i] = pb.parts[w * pb.ldp + r];
            b[i] = pb.parts[(pb.P + w) * pb.ldp + r];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (w0 + i < pb.P) { mu += a[i]; sa += b[i]; }
    }
    double qp = 0.0;
    for (int t = 0; t < pb.m; ++t) qp += pb.q[(int64_t)(2 * t) * pb.ldq + r] + pb.q[(int64_t)(2 * t + 1) * pb.ldq + r];
    double s2 = pb.sigma2 - qp;
    if (s2 < 0.0) s2 = 0.0;
    const double n = (double)(pb.Npad + 64), un = n * 0x1p-53, gam = un / (1.0 - un);
    double y = mu + (4.0 * gam * sa + 0x1p-1000);
    y += fabs(y) * 0x1p-52 + 0x1p-1000;   // at least one ulp up: y >= the exact mu~ + margin
    const double mu_up = pb.beta + y;
    const AcqParams& ap = pb.ap;
    double ub;
    switch (ap.acq) {
        case ACQ_EI: {
            const double D = mu_up - ap.p0;
            const double f = acq_eval(ap, mu_up, D <= 0.0 ? fmin(s2, 1.0) : 1.0);
            ub = f + 0x1p-38 * (1.0 + sqrt(pb.sigma2) + fmax(D, 0.0) + fabs(f));
            break;
        }
        case ACQ_PI:
            ub = (mu_up - ap.p0 >= 0.0 ? 1.0 : acq_eval(ap, mu_up, s2)) + 0x1p-38;
            break;
        case ACQ_UCB:
        case ACQ_MI: {
            const double sb = ap.p0 >= 0.0 ? s2 : 0.0;
            const double f = acq_eval(ap, mu_up, sb);
            const double roots = ap.acq == ACQ_UCB ? sqrt(sb) : sqrt(sb + fabs(ap.p1)) + sqrt(fabs(ap.p1));
            ub = f + 0x1p-38 * (fabs(mu_up) + fabs(ap.p0) * roots + 0x1p-1000);
            break;
        }
        case ACQ_LOGEI: {   // rises in mu and in sigma^2 (d/ds2 > 0); -inf (sigma^2 = 0, mu_up <= tau) stays -inf, not NaN
            const double f = acq_eval(ap, mu_up, s2);
            ub = f == -INFINITY ? f : f + 0x1p-38 * (1.0 + fabs(f));
            break;
        }
        default:
            ub = mu_up;
    }
    pb.ub[r] = ub;
}

// Round 1's list: the k1 candidates of highest bound in (bound desc, index asc), a NaN bound counting as +inf -- ONE workgroup, for
// R <= 8 x 1024.  A bound maps to a 64-bit key that orders as the doubles compare (-0 as +0); thread t holds the keys of the
// candidates t per .. t per + per - 1 in registers.  The k1-th largest key comes from a radix select, 8 bits a pass from the top:
//   * the leading bits that the largest and the smallest key share are skipped (bounds of one call share most of their exponent:
//     without the skip the first passes would add every key into one LDS word);
//   * a pass counts the digits of the keys that still agree with the threshold's known bits (integer LDS atomics), then EVERY wave
//     adds the 256 counts up from the top by itself and finds the digit at which the sum reaches the rank looked for -- no result
//     goes through LDS, and with three histograms in turn (the one of pass p + 2 is cleared during pass p) a pass has one barrier;
//   * when the rank looked for takes ALL keys of that digit, the bits below need not be resolved: keys compare by their bits
//     from that digit up.  Distinct bounds end there after about three passes; only ties at the threshold go down to bit 0.
// Membership: a key above the threshold is in; of the candidates AT the threshold, the first in ascending index until the list
// holds k1 -- the set the order above gives.  list1 holds the members in ascending index, mark[r] says whether r is one; the
// counters and the running record of the call are readied.
__device__ __forceinline__ double prune_key(double v) { return v != v ? INFINITY : v; }
__device__ __forceinline__ unsigned long long prune_key_bits(double v) {
    const double k = prune_key(v);
    const unsigned long long b = k == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(k);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;   // > 0 for every double: 0 marks "no candidate"
}
constexpr int SELECT_THREADS = 1024, SELECT_PER = 8;
constexpr int PRUNE_ARRIVE = 4;   // cnt[]: 0, 1 the rounds' list lengths, 2 k_trigemm_sq's count, 4, 5 the rounds' arrival counters
__global__ __launch_bounds__(SELECT_THREADS) void k_prune_select(const double* __restrict__ ub, int64_t R, int k1, int* __restrict__ list1,
                                                                 int* __restrict__ mark, unsigned* __restrict__ cnt, Best* __restrict__ rec) {
    __shared__ uint4 hist[3][64];   // [.][l]: the counts of the digits 4 l .. 4 l + 3
    __shared__ unsigned long long red[2 * SELECT_THREADS / 64];
    __shared__ unsigned tot[SELECT_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (int)((R + SELECT_THREADS - 1) / SELECT_THREADS);   // <= SELECT_PER
    unsigned long long key[SELECT_PER];
    unsigned long long kmax = 0ull, kmin = ~0ull;
#pragma unroll
    for (int i = 0; i < SELECT_PER; ++i) {
        const int64_t r = (int64_t)t * per + i;
        key[i] = (i < per && r < R) ? prune_key_bits(ub[r]) : 0ull;
        if (key[i]) { kmax = max(kmax, key[i]); kmin = min(kmin, key[i]); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        kmax = max(kmax, __shfl_xor(kmax, o));
        kmin = min(kmin, __shfl_xor(kmin, o));
    }
    if (lane == 0) { red[2 * wave] = kmax; red[2 * wave + 1] = kmin; }
    if (t < 128) (&hist[0][0])[t] = make_uint4(0u, 0u, 0u, 0u);   // (hist[0] and hist[1])
    __syncthreads();
    for (int w = 0; w < SELECT_THREADS / 64; ++w) { kmax = max(kmax, red[2 * w]); kmin = min(kmin, red[2 * w + 1]); }
    // the threshold agrees with `prefix` from bit hb up; k: its rank among the keys that do.  All of it is uniform over the workgroup.
    unsigned long long prefix = kmax;
    int hb = kmax == kmin ? 0 : 64 - __clzll((long long)(kmax ^ kmin)), k = k1;
    for (int pass = 0; hb > 0; ++pass) {
        const int wd = hb < 8 ? hb : 8, shift = hb - wd;
        unsigned* h = reinterpret_cast<unsigned*>(hist[pass % 3]);
#pragma unroll
        for (int i = 0; i < SELECT_PER; ++i)
            if (key[i] && (hb == 64 || (key[i] >> hb) == (prefix >> hb))) atomicAdd(h + ((unsigned)(key[i] >> shift) & ((1u << wd) - 1u)), 1u);
        __syncthreads();
        if (t < 64) hist[(pass + 2) % 3][t] = make_uint4(0u, 0u, 0u, 0u);
        // lane l: the digits 255 - 4 l down to 252 - 4 l; counts added from the top
        const uint4 c4 = hist[pass % 3][63 - lane];
        const unsigned c[4] = {c4.w, c4.z, c4.y, c4.x};
        unsigned incl = c[0] + c[1] + c[2] + c[3];
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        unsigned run = incl - (c[0] + c[1] + c[2] + c[3]);   // keys above this lane's digits
        int found = -1, knew = 0, all = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (run < (unsigned)k && (unsigned)k <= run + c[i]) { found = 255 - 4 * lane - i; knew = k - (int)run; all = knew == (int)c[i]; }
            run += c[i];
        }
        const unsigned long long who = __ballot(found >= 0);   // exactly one lane
        const int src = __ffsll((long long)who) - 1;
        const int digit = __shfl(found, src);
        k = __shfl(knew, src);
        all = __shfl(all, src);
        const unsigned long long low = hb == 64 ? ~0ull : (1ull << hb) - 1ull;
        prefix = (prefix & ~low) | (unsigned long long)digit << shift;
        hb = shift;
        if (all) break;   // every key of this digit is in: the bits below hb stay out of the comparison
    }
    // keys compare from bit hb up; the threshold is prefix >> hb, and k of the candidates that hold it are in (k >= 1)
    const unsigned long long thr = prefix >> hb;
    int ngt = 0, neq = 0;
#pragma unroll
    for (int i = 0; i < SELECT_PER; ++i) { ngt += key[i] && (key[i] >> hb) > thr; neq += key[i] && (key[i] >> hb) == thr; }
    const unsigned mine = (unsigned)ngt | (unsigned)neq << 16;   // ngt < 64 and neq <= 8192 in total: no carry between the halves
    unsigned incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) tot[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += tot[w];
    int g = (int)((incl - mine) & 0xffffu), e = (int)((incl - mine) >> 16);   // members above / ties at the threshold, before this thread
#pragma unroll
    for (int i = 0; i < SELECT_PER; ++i) {
        if (!key[i]) continue;
        const int64_t r = (int64_t)t * per + i;
        const bool gt = (key[i] >> hb) > thr, eq = (key[i] >> hb) == thr, in = gt || (eq && e < k);
        if (in) list1[g + min(e, k)] = (int)r;
        mark[r] = in;
        g += gt;
        e += eq;
    }
    if (t == 0) {
        cnt[0] = (unsigned)k1;
        cnt[1] = 0u;
        cnt[PRUNE_ARRIVE] = 0u;       // the rounds' arrival counters (k_trigemm_rows): their last arrivers leave them at zero, but a
        cnt[PRUNE_ARRIVE + 1] = 0u;   // call that died between two launches does not
        rec->val = -INFINITY;
        rec->idx = -1;
    }
}

// K*' rows of the listed candidates, packed (workgroup i: row list[i]; the grid is sized for the worst case)
// sq_min >= 0: a list of at most sq_min candidates is k_trigemm_rows's -- nothing is gathered and live_out (k_trigemm_sq's count) is 0
__global__ __launch_bounds__(256) void k_prune_gather(const int* __restrict__ list, const unsigned* __restrict__ cnt,
                                                      const double* __restrict__ src, int64_t ld, int64_t ncols, double* __restrict__ dst,
                                                      int sq_min, unsigned* __restrict__ live_out) {
    const int i = blockIdx.x, n = (int)*cnt;
    if (i == 0 && threadIdx.x == 0) *live_out = n > sq_min ? (unsigned)n : 0u;
    if (i >= n || n <= sq_min) return;
    const d2* s = reinterpret_cast<const d2*>(src + (int64_t)list[i] * ld);
    d2* d = reinterpret_cast<d2*>(dst + (int64_t)i * ld);
    for (int64_t j = threadIdx.x; j < ncols / 2; j += 256) d[j] = s[j];
}

// exact scores of the listed candidates: q in the fused finish's order (t < m from phase A at the candidate's index, t >= m from
// the round's own launch at its list position), mu from the round; the round's best is merged into the call's record.
struct PruneFinish {
    const int* list;
    const unsigned* cnt;
    const double *q, *q2, *mu2;
    int64_t ldq, ldq2;
    int m, T;
    double sigma2, beta;
    AcqParams ap;
    Best* rec;
    Best* best_out;       // nullable: the call's result.  The last round writes it; round 1 (list2 != nullptr) when it lists nobody for round 2
    long long best_off;
    unsigned* stat;       // nullable (pinned host word): round 2's list length, read by the host's path choice of a later call --
                          // written with best_out (by round 1: the 0 of its empty list)
    // round 1 only (list2 != nullptr): the tail that lists round 2
    const double* ub;     // [R] the bounds
    const int* mark;      // [R] k_prune_select's "in round 1"
    int64_t R;
    int* list2;
    unsigned* cnt2;
};
// One workgroup of NT threads, all of them: k_prune_finish's, or the workgroup of k_trigemm_rows that arrived last in its round.  The
// record is reduced by `better`, a total order, so it does not depend on NT.  sh: NT / 64 records, tail_L, tail_n: one word each (LDS).
template <int NT>
__device__ __forceinline__ void prune_finish_body(const PruneFinish& pf, Best* sh, double* tail_L, unsigned* tail_n) {
#pragma clang fp contract(off)
    const int n = (int)*pf.cnt;
    double v = -INFINITY;
    long long idx = -1;
    for (int i = threadIdx.x; i < n; i += NT) {
        const int64_t r = pf.list[i];
        double q = 0.0;
        for (int t0 = 0; t0 < pf.T; t0 += 8) {   // the sum in its order, sixteen loads in flight (a pair at a time: 8 us for 24 pairs, profiles/prune_select_ab.txt)
            double a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = min(t0 + u, pf.T - 1);
                const double* src = t < pf.m ? pf.q + r : pf.q2 + i;
                const int64_t ld = t < pf.m ? pf.ldq : pf.ldq2;
                a[u] = src[(int64_t)(2 * t) * ld];
                b[u] = src[(int64_t)(2 * t + 1) * ld];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (t0 + u < pf.T) q += a[u] + b[u];
        }
        double s2 = pf.sigma2 - q;
        if (s2 < 0.0) s2 = 0.0;  // predict_f: max(sigma2, 0)
        const double mu = pf.beta + pf.mu2[i];
        const double f = acq_eval(pf.ap, mu, s2);
        if (better(f, r, v, idx)) { v = f; idx = r; }
    }
    block_argmax(v, idx, sh);
    const bool last_round = !pf.list2;
    if (threadIdx.x == 0) {
        const Best b = *pf.rec;
        if (better(b.val, b.idx, v, idx)) { v = b.val; idx = b.idx; }
        pf.rec->val = idx >= 0 ? v : -INFINITY;
        pf.rec->idx = idx;
        if (pf.best_out && last_round) {
            pf.best_out->val = idx >= 0 ? v : -INFINITY;
            pf.best_out->idx = idx >= 0 ? idx + pf.best_off : -1;
        }
        if (pf.stat && last_round) *pf.stat = (unsigned)n;
        *tail_L = idx >= 0 ? v : -INFINITY;
        *tail_n = 0u;
    }
    // round 2's list: candidates outside round 1 whose bound is not below round 1's exact best (order is immaterial: every listed
    // candidate is scored on its own and the record is reduced by `better`).  The same workgroup, after its record: no other
    // workgroup waits on it, the next launch reads the list.
    if (last_round) return;
    __syncthreads();
    const double L = *tail_L;
    for (int64_t r0 = threadIdx.x; r0 < pf.R; r0 += 8 * NT) {   // eight loads of each in flight
        int mk[8];
        double u[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t r = min(r0 + NT * i, pf.R - 1);
            mk[i] = pf.mark[r];
            u[i] = pf.ub[r];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (r0 + NT * i < pf.R && !mk[i] && !(u[i] < L)) pf.list2[atomicAdd(tail_n, 1u)] = (int)(r0 + NT * i);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned n2 = *tail_n;
        *pf.cnt2 = n2;
        if (n2 == 0u) {   // nobody for round 2: round 1's record is the call's (v, idx are still the merged record here)
            if (pf.best_out) {
                pf.best_out->val = idx >= 0 ? v : -INFINITY;
                pf.best_out->idx = idx >= 0 ? idx + pf.best_off : -1;
            }
            if (pf.stat) *pf.stat = 0u;
        }
    }
}
__global__ __launch_bounds__(256) void k_prune_finish(PruneFinish pf) {
    __shared__ Best sh[4];
    __shared__ double tail_L;
    __shared__ unsigned tail_n;
    prune_finish_body<256>(pf, sh, &tail_L, &tail_n);
}

// ---- the exact rounds, row-split: k_trigemm_rows ------------------------------------------------------------------------------
// k_trigemm_sq runs a row piece against a 64-wide candidate tile as ONE job: for round 1 (64 candidates) that is one workgroup per
// row tile, and the job of the last tiles (K = N: ~190 chunks of 16) runs alone on one CU for ~0.2 ms.  Here a workgroup owns one
// 64-row HALF of a row tile against RS_COLS listed candidates and walks the half's whole contraction extent, so a round spreads over
// (halves x candidate groups) workgroups.  Every element of V comes out bit for bit as in k_trigemm_sq: an element of an
// MFMA's result depends on its own A row and B column only, so what changes is which rows and columns share an instruction, never an element's
// chain:
//   * v_mfma_f64_4x4x4 k-slot k of chunk kc carries contraction index 16 kc + 8 h + 2 k (the pair's even member), the next
//     instruction the odd one into the same accumulator (mma_row); h is the contraction half of the wave (khalf there);
//   * PIECE_WHOLE: kc < 8 (rt + 1), one chain per h, v = a0 + a1 (the loop's LDS fold).  The upper half stops at kc = 8 rt + 4: from
//     there on every row group of it is skipped there as well;
//   * PIECE_UPPER_SOLO (the loop's half mode): kc < 8 rt + 4, chains e_h (even members) and o_h (odd), v = (e0 + e1) + (o0 + o1);
//   * an 8-row group G of the tile skips chunk kc >= tri_kc = 8 rt when G < 2 (kc - tri_kc) + h (chunk_mma's skip);
//   * q of the half: sq_step over the rows of a lane in k_trigemm_sq's accumulator layout, then sq_tree (shared helpers).
// Sizing: a workgroup is 8 waves (h x four 16-row quarters: two waves per SIMD) against RS_COLS = 8 candidates, 2 accumulator chains
// of 8 x 8 per wave, 4 MFMAs per wave and chunk; round 1 of 64 candidates at T = 24 is 41 halves x 8 groups = 328 workgroups, two
// to a CU with 7 buffers of 9 KB, one with the RS_DEPTH = 8 kept (72 KB beside 12 KB of static LDS).  The operands come by LDS-DMA
// as whole 128-B rows, and the fragment reads of chunk kc + 1 are issued before the MFMAs of chunk kc into a second register set,
// so the LDS latency runs under the matrix pipe.  One vmcnt wait, one barrier and the DMA issue of two chunks per PAIR of chunks:
// at the pair (kc, kc + 1) chunks kc + 1 and kc + 2 have landed, every wave holds chunk kc in registers and is done with chunk
// kc - 1, so those two buffers are refilled (chunks kc + RS_DEPTH - 1 and kc + RS_DEPTH); RS_DEPTH - 4 chunks stay in flight
// under the pair's MFMAs.  RS_DEPTH is even: the ring turns in pairs.
// Measured on MI355X (round 1 at N = 3000, 64 candidates, 188 chunks in the longest half; profiles/prune_rows_pipeline_ab.txt):
//   operands loaded straight into VGPRs (16-B fragments, each fetched by two lanes, every 128-B row by two waves)   129 us
//     ... with 8 waves of 16 rows and more loads in flight (the per-CU fetch of scattered fragments bound it)        170 us
//   whole rows by DMA, loop serial per chunk (wait, barrier, DMA issue, six ds_read_b128, lgkmcnt(0), 16 MFMAs),
//     16 columns x 4 waves x 6 buffers, K*' pieces issued twice to keep the waves' wait counts equal                60.4 us
//     ... 9 / 12 buffers: 59.9 / 60.5 us (fetch latency is not on the path); without the DMA re-issue: 46.7 us
//   this loop (reads one chunk ahead, K*' issued once), columns x waves x buffers:
//     16 x 4 x 6: 51.8    16 x 4 x 12: 53.6    16 x 8 x 6: 49.2    16 x 8 x 12: 49.3
//      8 x 4 x 7: 45.4     8 x 4 x 12: 44.8     8 x 8 x 12: 42.8 (one workgroup a CU)     8 x 8 x 7: 42.6 us  <- kept then
//   with the round's finish in the launch (profiles/prune_round2_ab.txt; the parent's 8 x 8 x 7 kernel + its k_prune_finish launch
//   are 41.4 + 8.6 = 50.1 us there), 8 columns x 8 waves:
//     one barrier per chunk, 7 buffers                              54.9 us   (min 53.4, p90 56.3)
//     one barrier per pair of chunks, 6 buffers (two workgroups a CU) 50.8 us
//     one barrier per pair of chunks, 8 buffers (one workgroup a CU)  46.2 us  <- kept
// The column groups of a half run on one XCD: W's rows come from the Infinity Cache once per XCD.
// A workgroup takes the column groups grp0, grp0 + G, ... of its half until the list ends: round 1 (G = 8 for 64 candidates) and the
// long form of round 2 (G sized for the launch's cap) run one group per workgroup, the steady form of round 2 is a fixed grid of
// G = 8 groups for a list of any length (bohip.hip pruned_pass).  Between two groups the DMA is drained and a barrier stands before
// the ring, xch and vb are reused.
// The round finishes in the launch (RowsParams::finish): every workgroup that stored arrives at the round's counter, and the last
// one runs prune_finish_body -- the code of k_prune_finish -- on data that is complete; nothing waits on another workgroup.  The
// hand-over is the agent-scope release / acquire of the fused finish of k_trigemm_sq in its counter form (see the kernel's end).
// The expected count comes from the list's length on the device.  The counter is left at zero by the last arriver and zeroed by
// k_prune_select in every call (a call that died between two launches leaves it anywhere).
constexpr int RS_COLS = 8, RS_WAVES = 8, RS_THREADS = 64 * RS_WAVES, RS_DEPTH = 8;
constexpr int RS_RG = 16 / RS_WAVES;   // 8-row groups per wave
constexpr int RS_BUF = (64 + RS_COLS) * KC;                  // doubles of one chunk's operands in LDS
constexpr int RS_LDS_BYTES = RS_DEPTH * RS_BUF * 8;          // dynamic LDS of k_trigemm_rows
struct RowsParams {
    const double* W;
    int64_t ldw;
    const double* KsT;       // chunk [R][ldk]; column i of the round is row list[i]
    int64_t ldk;
    const int* list;
    const unsigned* cnt;     // the list's length (device)
    int cnt_max;             // the launch's worst case: a longer list is not this launch's (k_trigemm_sq takes it), every workgroup leaves
    const int* halves;       // rt | hh << 16 | solo << 17, heaviest first (host: rows_halves)
    int NH, G;               // halves in the table, candidate groups of RS_COLS
    int64_t alpha_row;
    double* q;               // [2 rt + hh][ldq] at the list position
    int64_t ldq;
    double* mu;              // [list position]
    // the round finishes in this launch (finish != 0): a workgroup that has stored arrives at *arrive, the last one scores and reduces
    int finish;
    unsigned* arrive;        // zero before the launch (k_prune_select) and after it (the last arriver)
    PruneFinish pf;
};
__global__ __launch_bounds__(RS_THREADS) void k_trigemm_rows(RowsParams rp) {
    __shared__ double xch[2 * 64 * RS_COLS];     // the h = 1 waves' chains
    __shared__ double vb[64 * RS_COLS];          // v of the half [row][column]
    // an XCD owns the halves x, x + 8, ... (block b runs on XCD b % 8) with all their candidate groups: W's rows are fetched once
    // per XCD, and the heaviest halves start first
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int hi = xcd + 8 * (slot / rp.G), grp0 = slot % rp.G;
    const int n = (int)*rp.cnt;
    if (hi >= rp.NH || n > rp.cnt_max || grp0 * RS_COLS >= n) return;
    const int code = __builtin_amdgcn_readfirstlane(rp.halves[hi]);
    const int rt = code & 0xffff, hh = (code >> 16) & 1;
    const bool solo = (code >> 17) & 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = wave / (RS_WAVES / 2), wq = wave % (RS_WAVES / 2);
    const int k = lane >> 4, b = (lane >> 2) & 3;
    const int tri_kc = 8 * rt, kc_end = tri_kc + (hh == 0 ? 4 : 8);   // (even)
    const int g0 = 8 * hh + RS_RG * wq;          // row group (8 rows) of the tile behind this wave's acc[0]
    // operands: LDS-DMA (global_load_lds, 16 B per lane) of whole 128-B rows, RS_DEPTH chunks deep.  Per chunk 8 pieces of 8 rows of
    // W and one of K*' (rows through the list): wave w issues W piece w and wave 0 the K*' piece as well -- so a wave counts one
    // load per chunk, wave 0 two (has_b picks the wait's count).  LDS row r holds the row's
    // 16-B segment s at slot s ^ (r & 7) (gemm_core.h's swizzle).  Fragments as the loop's: lane (k, b, t) reads A rows 4 (b >> 1) + t
    // of each row group and B column 4 (b & 1) + t, segment 4 h + k = the pair 16 kc + 8 h + 2 k.
    extern __shared__ __attribute__((aligned(16))) double rs_ring[];   // [RS_DEPTH][64 + RS_COLS rows][16]
    const int prow = lane >> 3, sseg = (lane & 7) ^ prow;
    const bool has_b = wave == 0;
    const double* a_src0 = rp.W + ((int64_t)rt * TILE + 64 * hh + 8 * wave + prow) * rp.ldw + 2 * sseg;
    const double* b_src = nullptr;   // (per column group, below)
    auto issue = [&](int kc, int buf) {
        kc = min(kc, kc_end - 1);   // (past the end: a harmless re-read into a free buffer that keeps the wait counts straight)
        double* d = rs_ring + buf * RS_BUF;
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)(a_src0 + (int64_t)kc * KC), (lds_void_ptr)(d + 8 * wave * KC), 16, 0, 0);
        if (has_b)
            __builtin_amdgcn_global_load_lds((gbl_void_ptr)(b_src + (int64_t)kc * KC), (lds_void_ptr)(d + 64 * KC), 16, 0, 0);
    };
    // all but the `left` youngest chunks of this wave's loads have landed
    auto wait_left = [&](auto left) {
        constexpr int L = decltype(left)::value;
        if (has_b) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * L) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
    };
    const int rr = 4 * (b >> 1) + (lane & 3), cc = 4 * (b & 1) + (lane & 3), S = 4 * h + k;
    const uint32_t ring0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const double*)rs_ring;
    const uint32_t fa = ring0 + (uint32_t)(((8 * RS_RG * wq + rr) * KC + 2 * (S ^ rr)) * 8);
    const uint32_t fb = ring0 + (uint32_t)(((64 + cc) * KC + 2 * (S ^ cc)) * 8);
    // the fragment reads of a chunk are issued one chunk AHEAD of their MFMAs, into the register set the MFMAs of the chunk before
    // last used: the LDS latency runs under the matrix pipe.  `landed` is the wait that ends the chunk.  The vmcnt wait, the barrier
    // and the DMA issue come once per PAIR of chunks.
    // INVARIANT (the compiler does not know that the asm reads of `frags` complete later): between a set's `frags` and its `landed`
    // no instruction may read, copy or spill a register of the set.  The source keeps it by touching the set in those two asm
    // statements only, by ending every chunk with `landed` (no set is in flight across the loop's back edge or a phi) and by the
    // sched_barriers around them.  To re-check after a compiler or flag change: in the gfx950 assembly of this kernel (hipcc -S or
    // --save-temps), between each group of three ds_read_b128 and the next s_waitcnt lgkmcnt(0) there must be nothing but
    // v_mfma_f64_4x4x4 on OTHER registers, scalar instructions and branches -- no v_mov / v_accvgpr / scratch_ of the three destinations;
    // tests/test_prune_rows_gpu.py fails on a stale fragment (every element is compared bit for bit).
    auto frags = [&](int buf, d2 (&av)[RS_RG], d2 (&bv)[1]) {
        const uint32_t off = (uint32_t)(buf * RS_BUF * 8);
        av[0] = ds_read128<0>(fa + off);
        av[1] = ds_read128<1024>(fa + off);
        bv[0] = ds_read128<0>(fb + off);
    };
    auto landed = [&](d2 (&av)[RS_RG], d2 (&bv)[1]) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[0]), "+v"(av[1]), "+v"(bv[0]));
    };
    double acc[RS_RG][1], acc2[RS_RG][1];   // WHOLE: acc (both members); SOLO: acc the even members, acc2 the odd ones
    auto run = [&](auto solo_tag) {
        constexpr bool SOLO = decltype(solo_tag)::value;
#pragma unroll
        for (int i = 0; i < RS_RG; ++i)
#pragma unroll
            for (int j = 0; j < 1; ++j) acc[i][j] = acc2[i][j] = 0.0;
        // the MFMAs of chunk kc on the registers `av`, `bv`
        auto mmas = [&](int kc, const d2 (&av)[RS_RG], const d2 (&bv)[1]) {
            const int skip = kc >= tri_kc ? 2 * (kc - tri_kc) + h - g0 : 0;   // row groups g0 + i, i < skip: all-zero in the block
#pragma unroll
            for (int i = 0; i < RS_RG; ++i) {
                if (skip > i) continue;
                if constexpr (SOLO) {
                    mma_row<1, 1>(av[i], bv, acc[i]);
                    mma_row<1, 2>(av[i], bv, acc2[i]);
                } else {
                    mma_row<1, 0>(av[i], bv, acc[i]);
                }
            }
        };
        static_assert(RS_DEPTH % 2 == 0, "a pair of chunks per barrier: the ring turns in pairs");
#pragma unroll
        for (int p = 0; p < RS_DEPTH - 1; ++p) issue(p, p);
        d2 av0[RS_RG], bv0[1], av1[RS_RG], bv1[1];
        wait_left(std::integral_constant<int, RS_DEPTH - 2>{});
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        frags(0, av0, bv0);
        landed(av0, bv0);
        __builtin_amdgcn_sched_barrier(0);
        int cur = 0;   // buffer of chunk kc
        for (int kc = 0; kc < kc_end; kc += 2) {   // (kc_end is even; the last pair reads ahead into a buffer that holds a re-read)
            // ONE wait and ONE barrier per pair: chunks kc + 1 and kc + 2 have landed (the RS_DEPTH - 4 later ones stay in flight);
            // after the barrier every wave's pieces of them are in LDS, every wave holds chunk kc in registers and is done with
            // chunk kc - 1: the two issues refill those two buffers
            wait_left(std::integral_constant<int, RS_DEPTH - 4>{});
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            const int prev = cur == 0 ? RS_DEPTH - 1 : cur - 1, b1 = cur + 1, b2 = cur + 2 == RS_DEPTH ? 0 : cur + 2;
            issue(kc + RS_DEPTH - 1, prev);
            issue(kc + RS_DEPTH, cur);
            frags(b1, av1, bv1);
            __builtin_amdgcn_sched_barrier(0);
            mmas(kc, av0, bv0);
            landed(av1, bv1);
            __builtin_amdgcn_sched_barrier(0);
            frags(b2, av0, bv0);
            __builtin_amdgcn_sched_barrier(0);
            mmas(kc + 1, av1, bv1);
            landed(av0, bv0);
            __builtin_amdgcn_sched_barrier(0);
            cur = b2;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    // the column groups grp0, grp0 + G, ... of this half until the list ends (round 1 and the long form's launch: one group)
    for (int grp = grp0; grp * RS_COLS < n; grp += rp.G) {
    const int ib = grp * RS_COLS + prow;
    b_src = rp.KsT + (int64_t)(ib < n ? rp.list[ib] : rp.list[0]) * rp.ldk + 2 * sseg;
    if (solo) run(std::true_type{});
    else run(std::false_type{});
    // fold the contraction halves in the loop's order, then v into vb in the rows' order
    if (h == 1) {
#pragma unroll
        for (int i = 0; i < RS_RG; ++i)
#pragma unroll
            for (int j = 0; j < 1; ++j) {
                xch[((wq * RS_RG + i)  + j) * 64 + lane] = acc[i][j];
                xch[64 * RS_COLS + ((wq * RS_RG + i)  + j) * 64 + lane] = acc2[i][j];
            }
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
        for (int i = 0; i < RS_RG; ++i)
#pragma unroll
            for (int j = 0; j < 1; ++j) {
                const double a1 = xch[((wq * RS_RG + i)  + j) * 64 + lane];
                double v = acc[i][j] + a1;
                if (solo) {
                    const double o1 = xch[64 * RS_COLS + ((wq * RS_RG + i)  + j) * 64 + lane];
                    v = v + (acc2[i][j] + o1);
                }
                const int row = 8 * (RS_RG * wq + i) + 4 * (b >> 1) + k, col = 8 * j + 4 * (b & 1) + (lane & 3);
                vb[row * RS_COLS + col] = v;
            }
    }
    __syncthreads();
    if (wave == 0) {
    // wave 0: the 8 candidate columns in k_trigemm_sq's accumulator layout (lane (k, b, t): column 4 (b & 1) + t)
    const int col = 8 * wave + 4 * (b & 1) + (lane & 3), i_list = grp * RS_COLS + col;
    const int64_t row_base = (int64_t)rt * TILE + 64 * hh;
    double s = 0.0;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        const int row = 8 * mi + 4 * (b >> 1) + k;
        const double v = vb[row * RS_COLS + col];
        if (row_base + row == rp.alpha_row) {
            if (i_list < n) rp.mu[i_list] = v;
        } else {
            s = sq_step(s, v);
        }
    }
    s = sq_tree(s);
    if (lane < 8 && i_list < n) {
        rp.q[(int64_t)(2 * rt + hh) * rp.ldq + i_list] = s;
        if (solo) rp.q[(int64_t)(2 * rt + 1) * rp.ldq + i_list] = 0.0;   // no sibling half: its slot is zero
    }
    // the storing wave drains its stores: before the next group's loads (the ring's waits count loads only) and before the arrival
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // the next group reuses the ring, xch and vb: every wave's DMA has landed (run's last wait) and vb has been read
    __syncthreads();
    }
    if (!rp.finish) return;
    // The round's hand-over, agent-scope release / acquire: the stores above are drained and behind a barrier; one lane releases,
    // waits, and adds to the round's counter.  The workgroup whose arrival completes the count (the halves in the table x the column
    // groups that have work: padding workgroups and groups past the list never arrive) acquires and finishes the round -- it waits
    // for nobody: everything it reads is complete.  The flag goes through xch (a further __shared__ object beside the DMA ring can
    // make the compiler drain vmcnt before every fragment read); xch is free after the barrier that ends the last group.
    unsigned* flag = reinterpret_cast<unsigned*>(xch + 64);
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned want = (unsigned)rp.NH * (unsigned)min(rp.G, (n + RS_COLS - 1) / RS_COLS);
        const bool last = __hip_atomic_fetch_add(rp.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want - 1u;
        if (last) __hip_atomic_store(rp.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = last;
    }
    __syncthreads();
    if (!*flag) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // (inlined: the kernel then has 101 VGPRs -- still 4 waves a SIMD -- and its SGPR spills lie outside the main loops; behind a
    // noinline call the callee takes 248 VGPRs and the kernel drops to 2 waves a SIMD)
    prune_finish_body<RS_THREADS>(rp.pf, reinterpret_cast<Best*>(xch), xch + 32, reinterpret_cast<unsigned*>(xch + 40));
}

// The exchange step of sharded scoring: `all` holds nrec records per draw-slot layout [rec][S] gathered
// from every shard (global indices); thread s reduces slot s over the records in (value desc, index asc) order -- the
// same rule on every rank, so every rank holds the same winner, and it equals the unsharded arg-max (first maximum wins,
// reference src/acquisition.jl:62).
__global__ __launch_bounds__(256) void k_reduce_records(const Best* __restrict__ all, int nrec, int S, Best* __restrict__ out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    double v = -INFINITY;
    long long idx = -1;
    for (int r = 0; r < nrec; ++r) {
        const Best b = all[(int64_t)r * S + s];
        if (better(b.val, b.idx, v, idx)) { v = b.val; idx = b.idx; }
    }
    out[s].val = idx >= 0 ? v : -INFINITY;
    out[s].idx = idx;
}

// ------------------------------------------------------------------------------------------------
// A8: gradient of the acquisition w.r.t. the candidate (role of ForwardDiff in wrap_gradient,
// reference src/acquisition.jl:11-17), analytic:
//     d k*_j / d x_k = fac(r_j) il2_k (x_k - X_jk)      fac = -k (SE), -(5/3) s2 (1+s) e^-s (Mat52)
//     grad mu  = sum_j alpha_j dk*_j          grad s2 = -2 sum_j u_j dk*_j,   u = K^-1 k* = W'(W k*)
// U' = V' W is a second triangular contraction on the MFMA engine (k_gemm, B = W in N-major form);
// this kernel finishes: one wave per candidate, lanes stride the observations, 2d butterfly sums,
// then the chain rule through the REFERENCE's acquisition formulas (not the textbook EI).
// ------------------------------------------------------------------------------------------------
template <bool LOGEI = true>
__device__ __forceinline__ void acq_partials(const AcqParams& a, double mu, double s2, double& dmu, double& ds2) {
    const double inv_sqrt_2pi = 0.3989422804014327;
    switch (a.acq) {
        case ACQ_EI: {
            if (s2 == 0.0) { dmu = mu > a.p0 ? 1.0 : 0.0; ds2 = 0.0; return; }
            const double D = mu - a.p0, s = sqrt(s2), z = D / s;
            const double Phi = 0.5 * (1.0 + erf(z / sqrt(2.0))), phi = inv_sqrt_2pi * exp(-0.5 * z * z);
            dmu = Phi + D * phi / s - z * phi / s;
            ds2 = (D * phi - z * phi) * (-z / (2.0 * s2));
            return;
        }
        case ACQ_PI: {
            if (s2 == 0.0) { dmu = 0.0; ds2 = 0.0; return; }
            const double D = mu - a.p0, s = sqrt(s2), z = D / s, phi = inv_sqrt_2pi * exp(-0.5 * z * z);
            dmu = phi / s;
            ds2 = phi * (-z / (2.0 * s2));
            return;
        }
        case ACQ_UCB: dmu = 1.0; ds2 = s2 > 0.0 ? a.p0 / (2.0 * sqrt(s2)) : 0.0; return;
        case ACQ_MI: dmu = 1.0; ds2 = a.p0 / (2.0 * sqrt(s2 + a.p1)); return;
        case ACQ_LOGEI:
            if constexpr (LOGEI) { const LogEIPartials g = logei_partials(mu, s2, a.p0); dmu = g.dmu; ds2 = g.ds2; }
            else { dmu = NAN; ds2 = NAN; }
            return;
        default: dmu = 1.0; ds2 = 0.0; return;
    }
}

// bohip_acq_eval (include/bohip_acq.h): the functor and its partials on n (mu, sigma^2) pairs, thread = element
__global__ __launch_bounds__(256) void k_acq_eval(AcqParams ap, int64_t n, const double* __restrict__ mu, const double* __restrict__ var,
                                                  double* __restrict__ value, double* __restrict__ dmu, double* __restrict__ dvar) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    value[i] = acq_eval(ap, mu[i], var[i]);
    if (dmu) acq_partials(ap, mu[i], var[i], dmu[i], dvar[i]);
}

// The posterior of one candidate from q = sum_j V'[r][j]^2 and the alpha row's product mu_raw, without contraction: the reference's
// clamp and formulas, shared by the small-batch kernels (kernels_small.hip) so that the value path and the gradient path agree on
// the scores bit for bit (tests/test_parity_gpu.py test_score_grad_vs_oracle)
__device__ __forceinline__ void posterior_like_small_finish(double sigma2, double beta, double q, double mu_raw, double& mu, double& s2) {
#pragma clang fp contract(off)
    s2 = sigma2 - q;
    if (s2 < 0.0) s2 = 0.0;  // predict_f: max(sigma2, 0)
    mu = beta + mu_raw;
}
// Waves per SIMD every instantiation has had, as its second launch bound: left free, the scheduler interleaves the coordinates'
// accumulate chains of the SE / Matern 5/2 body at 22 VGPRs more (DT = 8: 118 for 96) and one wave fewer.
constexpr int grad_finish_waves(int DT, bool LOW) { return DT <= 2 ? 8 : DT <= 4 ? 7 - LOW : DT <= 8 ? 5 - LOW : DT <= 16 ? 3 : DT <= 32 ? 2 : 1; }
template <int DT, bool LOW>
__global__ __launch_bounds__(256, grad_finish_waves(DT, LOW)) void k_grad_finish(const double* __restrict__ X, int64_t N,
                                                     const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                                     KernelHyper hp, const double* __restrict__ alpha,
                                                     const double* __restrict__ UT, int64_t ldu,
                                                     const double* __restrict__ mu, const double* __restrict__ var,
                                                     AcqParams ap, double* __restrict__ grad,
                                                     double* __restrict__ parts, unsigned* __restrict__ counters) {
    // workgroup (r, sp): candidate r, observations [sp len, (sp + 1) len): 256 threads stride them, 2d sums reduced in
    // a fixed order.  gridDim.y = 1 for large batches (one workgroup per candidate is plenty); for a handful of
    // candidates the observations are split over gridDim.y workgroups (a single workgroup walking N = 10^4
    // observations is latency-bound: 140 us), the LAST one to finish adds the partial sums in split order -- the
    // result depends on (N, gridDim.y) only, never on the batch -- and leaves the counter at zero for the next call.
    __shared__ double red[4][2 * DT];
    __shared__ int is_last;
    constexpr int PS = 2 * DT;   // partial record of one split: 2 DT gradient sums
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
        // agent-scope stores + an explicit wait instead of __threadfence(): the fence is an L2 write-back on this chip (7-60 us for
        // a device-wide hand-over, tools/ubench_gridbar.hip), the write-through stores cost nothing beside it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
        double dmu, ds2;
        const double m = mu[r], v = var[r];
        acq_partials(ap, m, v, dmu, ds2);
        // a clamped variance (sigma^2 == 0 exactly) has zero gradient, like max(., 0) under ForwardDiff
        grad[r * d + k] = dmu * a + (v > 0.0 ? ds2 * (-2.0 * b) : 0.0);
    }
}

// Large batches: one workgroup per GC = 2 candidates.  With one candidate per workgroup every workgroup streams the
// whole observation block X and alpha through L2 (R x 216 KB = 0.9 GB at R = 4096, N = 3000: 180 us); two candidates
// share each X row and alpha element in registers (0.11 ms).  Same per-candidate summation order as k_grad_finish with one split.
constexpr int GC = 2;   // 4 needs 259 VGPRs (320 with the coordinates in LDS) and is slower: 0.16 vs 0.11 ms at R = 4096
template <int DT, bool LOW>
__global__ __launch_bounds__(256) void k_grad_finish_tiled(const double* __restrict__ X, int64_t N,
                                                           const double* __restrict__ Xs, int64_t r_begin, int64_t r_end,
                                                           KernelHyper hp, const double* __restrict__ alpha,
                                                           const double* __restrict__ UT, int64_t ldu,
                                                           const double* __restrict__ mu, const double* __restrict__ var,
                                                           AcqParams ap, double* __restrict__ grad) {
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
            double dmu, ds2;
            const double m = mu[r], v = var[r];
            acq_partials(ap, m, v, dmu, ds2);
            grad[r * d + k] = dmu * a + (v > 0.0 ? ds2 * (-2.0 * b) : 0.0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// A9: counter-based standard normals.  z(seed, s, j) = Box-Muller of two splitmix64-derived
// uniforms keyed on (seed, s, j); identical on host and device, independent of sharding.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ inline double thompson_normal(uint64_t seed, int64_t s, int64_t j) {
    const uint64_t h = splitmix64(seed ^ splitmix64((uint64_t)s * 0xD1B54A32D192ED03ull + (uint64_t)j));
    const uint64_t h2 = splitmix64(h);
    const double u1 = ((double)(h >> 11) + 1.0) * (1.0 / 9007199254740993.0);  // (0,1)
    const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);         // [0,1)
    return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

// one workgroup per draw s; threads stride the candidates; never materialises S x R.
__global__ __launch_bounds__(256) void k_thompson(const double* __restrict__ mu, const double* __restrict__ var,
                                                  int64_t R, uint64_t seed, int64_t j0, Best* __restrict__ out,
                                                  long long idx_off) {
#pragma clang fp contract(off)
    __shared__ Best sh[4];
    const int64_t s = blockIdx.x;
    double v = -INFINITY;
    long long idx = -1;
    for (int64_t r = threadIdx.x; r < R; r += 256) {
        const double f = mu[r] + sqrt(var[r]) * thompson_normal(seed, s, j0 + r);
        if (better(f, r, v, idx)) { v = f; idx = r; }
    }
    block_argmax(v, idx, sh);
    if (threadIdx.x == 0) { out[s].val = idx >= 0 ? v : -INFINITY; out[s].idx = idx >= 0 ? idx + idx_off : -1; }
}

}  // namespace bohip
