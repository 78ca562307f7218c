// kernels_fit.hip -- the log marginal likelihood, and its gradient, at H hyper-parameter settings of one model in ONE launch
// (bohip_gp_mll_grad_batch in include/bohip_fit.h).  One workgroup of 512 threads owns one setting theta_h from its
// row of theta to its row of the result; the resident model is only read (X, y).  What a workgroup computes depends on (model,
// theta_h) alone -- no atomics, no cross-workgroup traffic, every reduction in a fixed order -- so a row's bits depend neither
// on H, nor on the row's position, nor on what happens to other rows.
//
// Per workgroup, with M = round_up(N, 16) (rows / columns N..M-1 are identity padding, so every block is a full 16 x 16 one),
// two slabs of global workspace A [(M + 1)][ld] and B [M][ld], ld = M + 8, and 16-wide panels in LDS:
//   decode   theta_h -> il2, sigma2, noise = exp(2 logNoise) + eps, beta (make_hyper's rule: an iso kernel fills il2 with one length);
//            a setting with a non-finite entry fails at once as pivot 1
//   build    lower triangle of cK_h into A (k_build_cov's expressions), row M of A = (y - beta)': the AUGMENTED row -- it rides
//            through the factorisation like any row below the panel and comes out as z' = (L^-1 r)'
//   chol     right-looking, per 16-column panel: wave 0 factors the 16 x 16 diagonal block in registers (lane = row, columns by
//            shuffles), one thread per row solves the panel below it, the trailing lower triangle takes its rank-16 update on the
//            matrix pipe (v_mfma_f64_4x4x4 as 8 x 8 x 4, wave task = 16 x 16 outputs) from the LDS panel.
//            A pivot that is not a finite positive number is recorded (1-based) by wave 0, published through LDS behind the
//            panel's barrier, and every wave leaves the loop at that same barrier.
//   value    mll = -1/2 z'z - sum log L_ii - N/2 log 2 pi   (r'alpha = z'z; nothing else is formed for a value-only call)
//   inverse  (gradient only) row block K of W = L^-1 exists only in LDS: W_K = L_KK^-1 [ -S_K | I ], S_K = sum_{J<K} L_KJ W_J the
//            sums pending in B.  From the transposed LDS image Wt of W_K:  alpha += Wt z_K,  pending sums of the rows below
//            += L_IK W_K  and  cK^-1 (lower, rows <= K) += W_K' W_K -- the last two as rank-16 MFMA updates of B, which holds pending
//            sums below row block K and cK^-1 above: a row block turns from one into the other when it is consumed.
//   grad     the single pass 1/2 sum (alpha_i alpha_j - cK^-1_ij) dcK_ij/dtheta of k_dmll_parts (same expressions per family),
//            thread = column, row phases by wave group, then shuffles and a fixed tree over the 8 waves; output in get_params
//            order [logNoise, mean, ll..., logsig], an iso kernel folds its d length entries into one.
//
// k_mll_batch<DT, LOW, true> is the leave-one-out objective at the same H settings (bohip_gp_loo_grad_batch in
// include/bohip_loo_batch.h): the same stages up to and including the inverse (which a value-only call needs too:
// kappa = diag cK^-1), then, with alpha in LDS, cK^-1 in the lower triangle of B and slab A dead,
//   finish   kappa_i = B[i][i], q_i = alpha_i / kappa_i (into zs), c_i = 1/2 (1 / kappa_i + q_i^2) (sqrt c into PB[0 .. M)),
//            logp_i = 1/2 log kappa_i - 1/2 alpha_i q_i - 1/2 log 2 pi, total = sum_{i < N} logp_i in a fixed order; the padding rows
//            i >= N are masked by index: q_i = c_i = 0.  A value-only call ends here.
//   b        b = cK^-1 q (into PB[M .. 2 M)): one thread per row, row i left of the diagonal then column i below it, j ascending
//   product  Mm = cK^-1 diag(c) cK^-1, lower triangle into slab A: per 16-column block K the panel P[i][k] = cK^-1(i, 16 K + k)
//            sqrt c_{16 K + k} (B read at (max, min)) is staged in PA and applied as a rank-16 update of every lower 16 x 16 block,
//            the one panel as both operands
//   grad     the gradient pass with the weight G_ij = 1/2 (b_i alpha_j + alpha_i b_j) - Mm_ij, the mean slot sum_i b_i: what
//            k_dloo_parts (kernels_loo.hip) states for the whole chip
#include "gemm_core.h"   // mfma444

namespace bohip {

constexpr int FIT_THREADS = 512;
constexpr int FIT_NB = 16;          // panel width = block size
constexpr int FIT_LP = FIT_NB + 1;  // row stride of every LDS panel image (fragment reads and row writes conflict-free)
constexpr int FIT_XROWS = 32;       // rows of X staged per chunk of the build / gradient passes
constexpr int FIT_STAGES = 7;       // stage stamps of workgroup 0 (tools): start, build, chol, value, inverse, grad; leave-one-out:
                                    // ..., inverse, product (finish, b and Mm), grad

struct FitArgs {
    const double* X;       // [N][d]
    const double* y;       // [N]
    const double* theta;   // [H][P]
    double* ws;            // [H][slab]
    double* mll;           // [H]  (leave-one-out: the total)
    double* grad;          // [H][P] or null
    double* logp;          // [H][N] or null: leave-one-out only
    long long* pivot;      // [H]
    unsigned long long* stamps;   // [FIT_STAGES] wall-clock ticks of workgroup 0, or null
    long long slab;        // doubles per setting = (2 M + 1) ld
    int N, M, ld, d, fam, iso, P;
};

__host__ __device__ inline int fit_panel_doubles(int M, int DT) {
    const int a = M * FIT_LP, b = FIT_XROWS * DT;
    return a > b ? a : b;
}
// LDS of one workgroup in doubles: [PA | PB | D 16x17 | Wi 16x17 | zs M | alpha M | red 8 x (DMAX + 3) | il2 DMAX | idg 16 | flag]
__host__ __device__ inline size_t fit_lds_bytes(int M, int DT) {
    return (size_t)(fit_panel_doubles(M, DT) + M * FIT_LP + 2 * FIT_NB * FIT_LP + 2 * M + 8 * (DMAX + 3) + DMAX + FIT_NB + 2) * 8;
}

// One wave: C[16 x 16 at (0, 0)] (+)= sgn sum_{k < 16} Pa[i][k] Pb[j][k], Pa / Pb LDS images of row stride FIT_LP.
// Lane layout of the 8 x 8 x 4 arrangement (gemm_core.h): A element (row 4 (bb >> 1) + t, k kq), B element (k kq, col 4 (bb & 1) + t),
// D element (row 4 (bb >> 1) + (lane >> 4), col 4 (bb & 1) + (lane & 3)).  Written are the elements with row <= row_max (rows are
// numbered from the task's first) and, where tri, col <= row.  init: the old value of C is not read.
__device__ __forceinline__ void fit_task16(double* __restrict__ C, int ldc, const double* Pa, const double* Pb, int lane, double sgn,
                                           bool init, bool tri, int row_max) {
    const int kq = lane >> 4, bb = (lane >> 2) & 3, t = lane & 3;
    const int ar = 4 * (bb >> 1) + t, bc = 4 * (bb & 1) + t;
    const int dr = 4 * (bb >> 1) + (lane >> 4), dc = 4 * (bb & 1) + (lane & 3);
    double old[2][2], acc[2][2];
    bool on[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int r = 8 * rb + dr, c = 8 * cb + dc;
            on[rb][cb] = r <= row_max && (!tri || c <= r);
            old[rb][cb] = (on[rb][cb] && !init) ? C[(int64_t)r * ldc + c] : 0.0;
            acc[rb][cb] = 0.0;
        }
#pragma unroll
    for (int k0 = 0; k0 < FIT_NB; k0 += 4) {
        const int k = k0 + kq;
        double av[2], bv[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) av[rb] = Pa[(8 * rb + ar) * FIT_LP + k];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) bv[cb] = Pb[(8 * cb + bc) * FIT_LP + k];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = mfma444(av[rb], bv[cb], acc[rb][cb]);
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
            if (on[rb][cb]) C[(int64_t)(8 * rb + dr) * ldc + 8 * cb + dc] = old[rb][cb] + sgn * acc[rb][cb];
}

// (row, column) of entry t of a lower triangle walked row by row: t = row (row + 1) / 2 + col
__device__ __forceinline__ void fit_tri_decode(int t, int& row, int& col) {
    int r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    row = r;
    col = t - r * (r + 1) / 2;
}

// fixed-order sum over the workgroup: shuffles inside a wave, then the 8 wave leaders as ((0+1)+(2+3))+((4+5)+(6+7)); red: 8 doubles
__device__ __forceinline__ double fit_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double fit_tree8(const double* r, int stride) {
    return ((r[0] + r[stride]) + (r[2 * stride] + r[3 * stride])) + ((r[4 * stride] + r[5 * stride]) + (r[6 * stride] + r[7 * stride]));
}

// a row that failed: the value, the pivot, a zero gradient row and (leave-one-out) a NaN row of logp
template <bool LOO>
__device__ __forceinline__ void fit_fail_row(const FitArgs& a, int64_t h, int tid, long long pivot) {
    if (tid == 0) { a.mll[h] = -INFINITY; a.pivot[h] = pivot; }
    if (a.grad != nullptr && tid < a.P) a.grad[h * a.P + tid] = 0.0;
    if constexpr (LOO) {
        if (a.logp != nullptr)
            for (int i = tid; i < a.N; i += FIT_THREADS) a.logp[h * a.N + i] = __builtin_nan("");
    }
}

template <int DT, bool LOW, bool LOO = false>
__global__ __launch_bounds__(FIT_THREADS) void k_mll_batch(FitArgs a) {
    extern __shared__ double fit_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, M = a.M, ld = a.ld, d = a.d, P = a.P;
    const int nb = M / FIT_NB;
    const int64_t h = blockIdx.x;
    double* const PA = fit_smem;
    double* const PB = PA + fit_panel_doubles(M, DT);
    double* const D = PB + M * FIT_LP;
    double* const Wi = D + FIT_NB * FIT_LP;
    double* const zs = Wi + FIT_NB * FIT_LP;
    double* const alpha = zs + M;
    double* const red = alpha + M;
    double* const il2s = red + 8 * (DMAX + 3);
    double* const idg = il2s + DMAX;
    int* const flag = reinterpret_cast<int*>(idg + FIT_NB);
    double* const A = a.ws + h * a.slab;
    double* const B = A + (int64_t)(M + 1) * ld;
    const double* th = a.theta + h * P;
    const bool want_grad = a.grad != nullptr;
    double* const gout = want_grad ? a.grad + h * P : nullptr;
    const bool stamp = a.stamps != nullptr && h == 0 && tid == 0;
    if (stamp) a.stamps[0] = wall_clock64();

    // ---- decode ------------------------------------------------------------------------------------------------------------
    const int nl = a.iso ? 1 : d;
    bool finite = true;
    for (int k = 0; k < P; ++k) finite = finite && (fabs(th[k]) < INFINITY);   // (false for NaN too)
    if (!finite) {   // the same for every thread: nobody has met a barrier yet
        fit_fail_row<LOO>(a, h, tid, 1);
        return;
    }
    const double noise_var = exp(2.0 * th[0]);
    const double noise = noise_var + 2.220446049250313e-16, beta = th[1];
    const double sigma2 = exp(2.0 * th[2 + nl]);
    if (tid < DMAX) il2s[tid] = tid < d ? exp(-2.0 * th[2 + (a.iso ? 0 : tid)]) : 0.0;

    // column / row-phase mapping of the build and gradient passes: the narrowest of 64, 128, 256, 512 columns that holds M
    const int CW = M <= 64 ? 64 : M <= 128 ? 128 : M <= 256 ? 256 : 512, RP = FIT_THREADS / CW;
    const int tx = tid % CW, ty = tid / CW;

    // ---- build -------------------------------------------------------------------------------------------------------------
    {
#pragma clang fp contract(off)
        double xj[DT];   // (loaded again for the gradient pass: not kept in registers through the factorisation)
#pragma unroll
        for (int k = 0; k < DT; ++k) xj[k] = (k < d && tx < N) ? a.X[(int64_t)tx * d + k] : 0.0;
        for (int i0 = 0; i0 < M; i0 += FIT_XROWS) {
            __syncthreads();   // (the first: il2s; later ones: the previous chunk has been read)
            for (int t = tid; t < FIT_XROWS * DT; t += FIT_THREADS) {
                const int i = i0 + t / DT, k = t % DT;
                PA[t] = (i < N && k < d) ? a.X[(int64_t)i * d + k] : 0.0;
            }
            __syncthreads();
            for (int c = ty; c < FIT_XROWS; c += RP) {
                const int i = i0 + c, j = tx;
                if (i >= M || j > i) continue;
                double v;
                if (i < N) {   // (j <= i < N)
                    double r = 0.0;
#pragma unroll
                    for (int k = 0; k < DT; ++k) {
                        const double t = PA[c * DT + k] - xj[k];
                        r += il2s[k] * (t * t);
                    }
                    v = cov_from_r<LOW>(a.fam, sigma2, r);
                    if (i == j) v += noise;
                } else {
                    v = (i == j) ? 1.0 : 0.0;
                }
                A[(int64_t)i * ld + j] = v;
            }
        }
        for (int j = tid; j < M; j += FIT_THREADS) A[(int64_t)M * ld + j] = j < N ? a.y[j] - beta : 0.0;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();
    if (stamp) a.stamps[1] = wall_clock64();

    // ---- Cholesky ----------------------------------------------------------------------------------------------------------
    int bad = 0;
    for (int p = 0; p < nb; ++p) {
        const int k0 = FIT_NB * p, w = k0 + FIT_NB;
        if (wave == 0) {
            // lane r < 16 holds row r of the diagonal block; column J of the factor is finished at step J
            const int r = lane & 15;
            double v[FIT_NB];
#pragma unroll
            for (int c = 0; c < FIT_NB; ++c) v[c] = (lane < FIT_NB && c <= r) ? A[(int64_t)(k0 + r) * ld + k0 + c] : (c == r ? 1.0 : 0.0);
            int wbad = 0;
#pragma unroll
            for (int J = 0; J < FIT_NB; ++J) {
                const double dj = __shfl(v[J], J, 64);
                if (!(dj > 0.0 && dj < INFINITY) && wbad == 0) wbad = k0 + J + 1;
                const double lj = sqrt(dj);
                v[J] = (r == J) ? lj : v[J] / lj;
#pragma unroll
                for (int c = J + 1; c < FIT_NB; ++c) {
                    const double lc = __shfl(v[J], c, 64);
                    v[c] -= v[J] * lc;
                }
            }
            if (lane < FIT_NB) {
#pragma unroll
                for (int c = 0; c < FIT_NB; ++c) {
                    const double x = c <= r ? v[c] : 0.0;
                    D[r * FIT_LP + c] = x;
                    if (c <= r) A[(int64_t)(k0 + r) * ld + k0 + c] = x;
                    if (c == r) idg[r] = 1.0 / x;
                }
            }
            if (lane == 0) *flag = wbad;
        }
        __syncthreads();
        bad = *flag;
        if (bad != 0) break;   // the same word for every thread: all waves leave here
        // panel solve: rows w .. M (the last is the augmented row), one thread per row:  x L11' = a
        const int cnt = M - w + 1;
        for (int li = tid; li < cnt; li += FIT_THREADS) {
            double* row = A + (int64_t)(w + li) * ld + k0;
            double x[FIT_NB];
#pragma unroll
            for (int c = 0; c < FIT_NB; ++c) x[c] = row[c];
#pragma unroll
            for (int j = 0; j < FIT_NB; ++j) {
                double s = x[j];
#pragma unroll
                for (int c = 0; c < j; ++c) s -= x[c] * D[j * FIT_LP + c];
                x[j] = s * idg[j];
            }
#pragma unroll
            for (int c = 0; c < FIT_NB; ++c) {
                row[c] = x[c];
                PA[li * FIT_LP + c] = x[c];
            }
        }
        // (the 15 rows behind the augmented one are read by its tasks and masked on the way out: keep them defined)
        if (tid < (FIT_NB - 1) * FIT_NB) {
            const int li = cnt + tid / FIT_NB;
            if (li < M) PA[li * FIT_LP + tid % FIT_NB] = 0.0;
        }
        __syncthreads();
        // trailing update: row blocks I = 0 .. nbt (nbt: the augmented row alone), column blocks Jb <= min(I, nbt - 1)
        const int nbt = nb - p - 1, ntri = nbt * (nbt + 1) / 2, ntask = ntri + nbt;
        for (int t = wave; t < ntask; t += FIT_THREADS / 64) {
            int I, Jb;
            if (t < ntri) fit_tri_decode(t, I, Jb);
            else { I = nbt; Jb = t - ntri; }
            fit_task16(A + (int64_t)(w + FIT_NB * I) * ld + w + FIT_NB * Jb, ld, PA + FIT_NB * I * FIT_LP, PA + FIT_NB * Jb * FIT_LP,
                       lane, -1.0, false, I == Jb, I == nbt ? 0 : FIT_NB - 1);
        }
        __syncthreads();
    }
    if (bad != 0) {
        fit_fail_row<LOO>(a, h, tid, bad);
        return;
    }
    if (stamp) a.stamps[2] = wall_clock64();

    // ---- value -------------------------------------------------------------------------------------------------------------
    {
        double s = 0.0;
        for (int i = tid; i < M; i += FIT_THREADS) {
            const double z = A[(int64_t)M * ld + i];
            zs[i] = z;
            alpha[i] = 0.0;
            if constexpr (!LOO)
                if (i < N) s += -0.5 * z * z - log(A[(int64_t)i * ld + i]);
        }
        if constexpr (!LOO) {
            s = fit_wave_sum(s);
            if (lane == 0) red[wave] = s;
            __syncthreads();
            if (tid == 0) a.mll[h] = fit_tree8(red, 1) - 0.5 * (double)N * log(2.0 * M_PI);
        }
        if (tid == 0) a.pivot[h] = 0;
    }
    if (stamp) a.stamps[3] = wall_clock64();
    if (!LOO && !want_grad) return;

    // ---- W = L^-1 row block by row block, alpha and cK^-1 on the way ---------------------------------------------------------
    for (int K = 0; K < nb; ++K) {
        const int k0 = FIT_NB * K, w = k0 + FIT_NB;
        __syncthreads();   // (the previous block's tasks have read PA / PB; the value stage has read red)
        // the diagonal block of L, and the pending sums S_K transposed: St[j][k] = B[k0 + k][j], j < k0
        if (tid < FIT_NB * FIT_NB) {
            const int r = tid / FIT_NB, c = tid % FIT_NB;
            D[r * FIT_LP + c] = c <= r ? A[(int64_t)(k0 + r) * ld + k0 + c] : 0.0;
        }
        for (int idx = tid; idx < FIT_NB * k0; idx += FIT_THREADS) {
            const int k = idx / k0, j = idx - k * k0;
            PA[j * FIT_LP + k] = B[(int64_t)(k0 + k) * ld + j];
        }
        __syncthreads();
        if (tid < FIT_NB) {   // column c of L_KK^-1 by forward substitution, statically unrolled (the guards are per lane)
            const int c = tid;
            double x[FIT_NB];
#pragma unroll
            for (int i = 0; i < FIT_NB; ++i) {
                const double inv = 1.0 / D[i * FIT_LP + i];
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < i; ++m) s += (m >= c) ? D[i * FIT_LP + m] * x[m] : 0.0;
                x[i] = i < c ? 0.0 : (i == c ? inv : -s * inv);
                Wi[i * FIT_LP + c] = x[i];
            }
        }
        __syncthreads();
        // Wt[j][k] = W_K[k][j]:  j < k0: -sum_{m <= k} Wi[k][m] St[j][m];  j = k0 + c: Wi[k][c].   alpha_j += sum_k Wt[j][k] z_{k0 + k}
        for (int j = tid; j < w; j += FIT_THREADS) {
            double o[FIT_NB];
            if (j < k0) {
                double s[FIT_NB];
#pragma unroll
                for (int m = 0; m < FIT_NB; ++m) s[m] = PA[j * FIT_LP + m];
#pragma unroll
                for (int k = 0; k < FIT_NB; ++k) {
                    double q = 0.0;
#pragma unroll
                    for (int m = 0; m <= k; ++m) q += Wi[k * FIT_LP + m] * s[m];
                    o[k] = -q;
                }
            } else {
#pragma unroll
                for (int k = 0; k < FIT_NB; ++k) o[k] = Wi[k * FIT_LP + (j - k0)];
            }
            double al = alpha[j];
#pragma unroll
            for (int k = 0; k < FIT_NB; ++k) {
                PB[j * FIT_LP + k] = o[k];
                al += o[k] * zs[k0 + k];
            }
            alpha[j] = al;
        }
        __syncthreads();   // St has been read: PA takes the column panel K of L, rows w .. M - 1
        for (int li = tid; li < M - w; li += FIT_THREADS) {
            const double* row = A + (int64_t)(w + li) * ld + k0;
#pragma unroll
            for (int c = 0; c < FIT_NB; ++c) PA[li * FIT_LP + c] = row[c];
        }
        __syncthreads();
        // tasks: pending sums of the row blocks below, B[w + 16 I][16 Jb] (+)= L_IK W_K (first touched when Jb == K), then
        //        cK^-1 blocks (I2 >= J2) <= K, B[16 I2][16 J2] (+)= W_K' W_K (row block K first touched now)
        const int nbelow = nb - K - 1, nacc = nbelow * (K + 1), nkinv = (K + 1) * (K + 2) / 2;
        for (int t = wave; t < nacc + nkinv; t += FIT_THREADS / 64) {
            if (t < nacc) {
                const int I = t / (K + 1), Jb = t - I * (K + 1);
                fit_task16(B + (int64_t)(w + FIT_NB * I) * ld + FIT_NB * Jb, ld, PA + FIT_NB * I * FIT_LP, PB + FIT_NB * Jb * FIT_LP, lane, 1.0,
                           Jb == K, false, FIT_NB - 1);
            } else {
                int I2, J2;
                fit_tri_decode(t - nacc, I2, J2);
                fit_task16(B + (int64_t)(FIT_NB * I2) * ld + FIT_NB * J2, ld, PB + FIT_NB * I2 * FIT_LP, PB + FIT_NB * J2 * FIT_LP, lane, 1.0,
                           I2 == K, I2 == J2, FIT_NB - 1);
            }
        }
    }
    __syncthreads();
    if (stamp) a.stamps[4] = wall_clock64();

    [[maybe_unused]] double* const bv = PB + M;   // leave-one-out: b, M doubles behind sqrt c
    if constexpr (LOO) {
        double* const q = zs;    // (z is dead after the inverse)
        double* const sc = PB;   // sqrt c, M doubles
        // ---- finish: per point from kappa = diag cK^-1, and the total ------------------------------------------------------------
        {
            double s = 0.0;
            for (int i = tid; i < M; i += FIT_THREADS) {
                double qi = 0.0, ci = 0.0;
                if (i < N) {   // (rows N .. M - 1 are padding: masked by index)
                    const double kp = B[(int64_t)i * ld + i], al = alpha[i], v = 1.0 / kp;
                    qi = al * v;
                    ci = 0.5 * (v + qi * qi);
                    const double lp = 0.5 * log(kp) - 0.5 * al * qi - 0.5 * log(2.0 * M_PI);
                    if (a.logp != nullptr) a.logp[h * N + i] = lp;
                    s += lp;
                }
                q[i] = qi;
                sc[i] = sqrt(ci);
            }
            s = fit_wave_sum(s);
            if (lane == 0) red[wave] = s;
            __syncthreads();
            if (tid == 0) a.mll[h] = fit_tree8(red, 1);
        }
        if (!want_grad) return;
        // ---- b = cK^-1 q from the lower storage -----------------------------------------------------------------------------------
        for (int i = tid; i < M; i += FIT_THREADS) {
            double s = 0.0;
            if (i < N) {
                for (int j = 0; j < i; ++j) s += B[(int64_t)i * ld + j] * q[j];
                for (int j = i; j < N; ++j) s += B[(int64_t)j * ld + i] * q[j];
            }
            bv[i] = s;
        }
        // ---- Mm = cK^-1 diag(c) cK^-1, lower triangle into A ------------------------------------------------------------------------
        const int nlow = nb * (nb + 1) / 2;
        for (int K = 0; K < nb; ++K) {
            const int k0 = FIT_NB * K;
            __syncthreads();   // (the previous panel's tasks have read PA; the first: sc is written, the inverse's tasks have read PA)
            // rows above the block: cK^-1(i, k0 + k) = B[k0 + k][i], i fastest; rows from the block on: B[i][k0 + k], the block itself at (max, min)
            for (int idx = tid; idx < FIT_NB * k0; idx += FIT_THREADS) {
                const int k = idx / k0, i = idx - k * k0, c = k0 + k;
                PA[i * FIT_LP + k] = (i < N && c < N) ? B[(int64_t)c * ld + i] * sc[c] : 0.0;
            }
            for (int idx = tid; idx < FIT_NB * (M - k0); idx += FIT_THREADS) {
                const int i = k0 + idx / FIT_NB, k = idx % FIT_NB, c = k0 + k;
                const int hi = i > c ? i : c, lo = i > c ? c : i;
                PA[i * FIT_LP + k] = (i < N && c < N) ? B[(int64_t)hi * ld + lo] * sc[c] : 0.0;
            }
            __syncthreads();
            for (int t = wave; t < nlow; t += FIT_THREADS / 64) {
                int I, Jb;
                fit_tri_decode(t, I, Jb);
                fit_task16(A + (int64_t)(FIT_NB * I) * ld + FIT_NB * Jb, ld, PA + FIT_NB * I * FIT_LP, PA + FIT_NB * Jb * FIT_LP, lane, 1.0,
                           K == 0, I == Jb, FIT_NB - 1);
            }
        }
        __syncthreads();
        if (stamp) a.stamps[5] = wall_clock64();
    }

    // ---- gradient: sum_ij G_ij dcK_ij / dtheta over the lower triangle, G = 1/2 (alpha alpha' - cK^-1), or for leave-one-out
    //      1/2 (b alpha' + alpha b') - Mm ----------------------------------------------------------------------------------------
    double xj[DT], acc[DT], a_sig = 0.0, a_noise = 0.0, a_mean = 0.0;
#pragma unroll
    for (int k = 0; k < DT; ++k) {
        xj[k] = (k < d && tx < N) ? a.X[(int64_t)tx * d + k] : 0.0;
        acc[k] = 0.0;
    }
    const double aj = tx < N ? alpha[tx] : 0.0;
    double bj = 0.0;
    if constexpr (LOO) bj = tx < N ? bv[tx] : 0.0;
    for (int i0 = 0; i0 < N; i0 += FIT_XROWS) {
        __syncthreads();
        for (int t = tid; t < FIT_XROWS * DT; t += FIT_THREADS) {
            const int i = i0 + t / DT, k = t % DT;
            PA[t] = (i < N && k < d) ? a.X[(int64_t)i * d + k] : 0.0;
        }
        __syncthreads();
        for (int c = ty; c < FIT_XROWS; c += RP) {
            const int i = i0 + c, j = tx;
            if (i >= N || j > i) continue;   // (j <= i < N)
            const double ai = alpha[i];
            double G, bi = 0.0;
            if constexpr (LOO) {   // (the triangle is walked once: an off-diagonal entry counts twice)
                bi = bv[i];
                const double m = A[(int64_t)i * ld + j];
                G = i == j ? ai * bi - m : (bi * aj + ai * bj) - 2.0 * m;
            } else {
                G = (ai * aj - B[(int64_t)i * ld + j]) * (i == j ? 0.5 : 1.0);
            }
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < DT; ++k) {
                const double dx = PA[c * DT + k] - xj[k];
                r += il2s[k] * (dx * dx);
            }
            double Kij, fac;
            if constexpr (LOW) {
                Kij = matern_lo_k(a.fam, sigma2, r);
                fac = -matern_lo_fx(a.fam, sigma2, r);   // 0 on the diagonal for M12, whose limit there is 0
            } else if (a.fam == FAM_M52) {
                const double sq = sqrt(5.0) * sqrt(r), e = exp(-sq);
                Kij = sigma2 * (1.0 + sq + 5.0 / 3.0 * r) * e;
                fac = 5.0 / 3.0 * sigma2 * (1.0 + sq) * e;
            } else {
                Kij = sigma2 * exp(-0.5 * r);
                fac = Kij;
            }
            const double gf = G * fac;
#pragma unroll
            for (int k = 0; k < DT; ++k) {
                const double dx = PA[c * DT + k] - xj[k];
                acc[k] += gf * (il2s[k] * (dx * dx));
            }
            a_sig += G * 2.0 * Kij;
            if (i == j) {
                a_noise += G * 2.0 * noise_var;   // G carries the 1/2
                a_mean += LOO ? bi : ai;
            }
        }
    }
    constexpr int RS = DMAX + 3;
    a_noise = fit_wave_sum(a_noise); a_mean = fit_wave_sum(a_mean); a_sig = fit_wave_sum(a_sig);
#pragma unroll
    for (int k = 0; k < DT; ++k) acc[k] = fit_wave_sum(acc[k]);
    if (lane == 0) {
        red[wave * RS + 0] = a_noise; red[wave * RS + 1] = a_mean;
#pragma unroll
        for (int k = 0; k < DT; ++k) if (k < d) red[wave * RS + 2 + k] = acc[k];
        red[wave * RS + 2 + d] = a_sig;
    }
    __syncthreads();
    if (tid < d + 3) PB[tid] = fit_tree8(red + tid, RS);   // PB[0 .. d + 2]: {noise, mean, ll_0.., logsig}
    __syncthreads();
    if (tid < P) {
        double v;
        if (tid < 2) v = PB[tid];
        else if (!a.iso) v = PB[tid];
        else if (tid == 2) { v = 0.0; for (int k = 0; k < d; ++k) v += PB[2 + k]; }
        else v = PB[2 + d];
        gout[tid] = v;
    }
    if (stamp) a.stamps[LOO ? 6 : 5] = wall_clock64();
}

}  // namespace bohip
