// kernels_ens.hip -- one acquisition averaged over H hyper-parameter settings of one model (bohip_gp_score_ens in
// include/bohip_ens.h): a(x) = sum_h w_h a(x; theta_h), the integrated acquisition of Snoek, Larochelle & Adams 2012.
// The resident model is only read (X, y).  Three stages, every stage boundary a launch boundary:
//   k_ens_factor  one workgroup of 512 threads per setting: decode, build and right-looking panel Cholesky exactly as k_mll_batch
//                 (kernels_fit.hip) states them -- restated here, so that kernel's code and bits do not move -- then the fit's inverse
//                 stage with the row blocks of W = L^-1 WRITTEN to the setting's second slab B (a row block of B turns from the pending
//                 sums S_K into W_K when it is consumed; the diagonal block's upper triangle is written as exact zeros).  Left behind:
//                 W in B, z = L^-1 (y - beta) in row M of A (the augmented row), pivot[h] (0, or the 1-based failing pivot).
//   k_ens_score   grid (candidate tiles of 16) x (settings), 256 threads.  K*' tile [16][M + 1] in LDS from X, xs and theta_h
//                 (k_mll_batch's expressions), then V = W K* over the lower triangle on v_mfma_f64_4x4x4 (8 x 8 x 4 arrangement, a wave
//                 owns a 16-row block of V and walks its column blocks J <= I in ascending order; W fragments come straight from global,
//                 32 B per lane and block).  V never leaves registers: a finished block gives per candidate sum V^2 and sum V z over its
//                 16 rows (two rows in the lane, then three xor shuffles), the blocks are added in ascending order by one thread per
//                 candidate: sigma^2 = max(s_f^2 - sum, 0), mu = beta + sum, a_h = acq_eval.  A failed setting's rows are NaN.
//   k_ens_weights, k_ens_reduce   w~ = w / (sum of the surviving w) in ascending h; scores[j] = sum_h w~_h a_h(x_j) sequentially in
//                 ascending h from 0.0, settings with w~ = 0 skipped; per-workgroup arg-max records for k_argmax_final.
// What is computed for (theta_h, x_j) depends on (model, theta_h, x_j) alone: a candidate's column of the MFMA products, its shuffles
// and its sums see the same operations at every position of a tile, for every R, H and split into launches.
//
// The gradient (bohip_gp_score_ens_grad in include/bohip_ens_grad.h) adds
//   k_ens_alpha   one workgroup per setting behind k_ens_factor: alpha = W' z, column j summed over the rows i >= j in ascending order,
//                 into a block of its own ([settings of the launch][M]).
//   k_ens_grad    k_ens_score instantiated with the gradient's arguments (ONE text for the K*' tile, the V stage and the finish: the
//                 value path and the gradient path agree bit for bit; the value-only instantiation compiles to the code it had) with V
//                 kept in a second 16 x (M + 1) LDS tile; then U = W' V on the matrix pipe (a wave owns a 16-row block J of U and
//                 walks I >= J in ascending order, W's fragments read transposed) into the tile K*' has left; then the final stage: r and fx = 2 dk/dr
//                 again from X, the candidates and il2 (rolled over d), fx alpha and fx U over the two tiles, and per (candidate,
//                 coordinate) the sums  sum_j fx_j alpha_j il2_k (x_k - X_jk)  and  sum_j fx_j U_j il2_k (x_k - X_jk)  over the
//                 observations in ascending order by ONE thread, so the order is the same at every position of a tile;
//                 g_h = da/dmu grad mu + (sigma^2 > 0 ? da/dsigma^2 (-2 sum) : 0), k_grad_finish's rule for a clamped variance.
//   k_ens_reduce_grad   grad[j][k] = sum_h w~_h g_h[j][k], sequentially in ascending h from 0.0, settings with w~ = 0 skipped.
#include "gemm_core.h"   // mfma444

namespace bohip {

constexpr int ENS_THREADS = 256;   // k_ens_score
constexpr int ENS_TC = 16;         // candidates per tile

struct EnsFactorArgs {
    const double* X;       // [N][d]
    const double* y;       // [N]
    const double* theta;   // [H][P]
    double* ws;            // [H][slab]
    long long* pivot;      // [H]
    long long slab;        // doubles per setting = (2 M + 1) ld  (the fit's two slabs A [(M + 1)][ld], B [M][ld])
    int N, M, ld, d, fam, iso, P;
};

struct EnsScoreArgs {
    const double* X;           // [N][d]
    const double* theta;       // [H][P]
    const double* ws;          // [H][slab]
    const long long* pivot;    // [H]
    const double* xs;          // [R][d] candidates of this chunk
    double *each, *mu, *var;   // [H][ldr]
    long long slab, ldr, R;
    AcqParams ap;
    int N, M, ld, d, fam, iso, P;
    static constexpr bool GRAD = false;
};

struct EnsGradArgs : EnsScoreArgs {
    const double* alpha;   // [settings of the launch][M]  W' z (k_ens_alpha)
    double* geach;         // [H][ldr][d] per-setting gradients
    static constexpr bool GRAD = true;
};

// LDS of k_ens_score in doubles: [Ks 16 x (M + 1) | z M | il2 DMAX | xs tile 16 x DT, later the block sums 2 x 16 per row block]
__host__ __device__ inline size_t ens_score_lds_bytes(int M, int DT) {
    const int a = ENS_TC * DT, b = 2 * ENS_TC * (M / FIT_NB);
    return (size_t)(ENS_TC * (M + 1) + M + DMAX + (a > b ? a : b)) * 8;
}

// LDS of k_ens_grad in doubles: [Ks, later U and fx U 16 x (M + 1) | V, later fx alpha 16 x (M + 1) | z M | alpha M | il2 DMAX |
// xs tile 16 x DT | block sums 2 x 16 per row block | da/dmu, da/dsigma^2, sigma^2 per candidate]: 156 800 B at M = 512, DT = 64
__host__ __device__ inline size_t ens_grad_lds_bytes(int M, int DT) {
    return (size_t)(2 * ENS_TC * (M + 1) + 2 * M + DMAX + ENS_TC * DT + 2 * ENS_TC * (M / FIT_NB) + 3 * ENS_TC) * 8;
}

template <int DT, bool LOW>
__global__ __launch_bounds__(FIT_THREADS) void k_ens_factor(EnsFactorArgs a) {
    extern __shared__ double fit_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, M = a.M, ld = a.ld, d = a.d, P = a.P;
    const int nb = M / FIT_NB;
    const int64_t h = blockIdx.x;
    double* const PA = fit_smem;
    double* const PB = PA + fit_panel_doubles(M, DT);
    double* const D = PB + M * FIT_LP;
    double* const Wi = D + FIT_NB * FIT_LP;
    double* const il2s = Wi + FIT_NB * FIT_LP + 2 * M + 8 * (DMAX + 3);   // (k_mll_batch's layout: fit_lds_bytes sizes it)
    double* const idg = il2s + DMAX;
    int* const flag = reinterpret_cast<int*>(idg + FIT_NB);
    double* const A = a.ws + h * a.slab;
    double* const B = A + (int64_t)(M + 1) * ld;
    const double* th = a.theta + h * P;

    // ---- decode (k_mll_batch's) ----------------------------------------------------------------------------------------------
    const int nl = a.iso ? 1 : d;
    bool finite = true;
    for (int k = 0; k < P; ++k) finite = finite && (fabs(th[k]) < INFINITY);   // (false for NaN too)
    if (!finite) {   // the same for every thread: nobody has met a barrier yet
        if (tid == 0) a.pivot[h] = 1;
        return;
    }
    const double noise = exp(2.0 * th[0]) + 2.220446049250313e-16, beta = th[1];
    const double sigma2 = exp(2.0 * th[2 + nl]);
    if (tid < DMAX) il2s[tid] = tid < d ? exp(-2.0 * th[2 + (a.iso ? 0 : tid)]) : 0.0;
    const int CW = M <= 64 ? 64 : M <= 128 ? 128 : M <= 256 ? 256 : 512, RP = FIT_THREADS / CW;
    const int tx = tid % CW, ty = tid / CW;

    // ---- build (k_mll_batch's) -----------------------------------------------------------------------------------------------
    {
#pragma clang fp contract(off)
        double xj[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) xj[k] = (k < d && tx < N) ? a.X[(int64_t)tx * d + k] : 0.0;
        for (int i0 = 0; i0 < M; i0 += FIT_XROWS) {
            __syncthreads();
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

    // ---- Cholesky (k_mll_batch's) --------------------------------------------------------------------------------------------
    int bad = 0;
    for (int p = 0; p < nb; ++p) {
        const int k0 = FIT_NB * p, w = k0 + FIT_NB;
        if (wave == 0) {
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
        if (tid < (FIT_NB - 1) * FIT_NB) {
            const int li = cnt + tid / FIT_NB;
            if (li < M) PA[li * FIT_LP + tid % FIT_NB] = 0.0;
        }
        __syncthreads();
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
    if (tid == 0) a.pivot[h] = bad;
    if (bad != 0) return;

    // ---- W = L^-1 row block by row block into B (k_mll_batch's inverse stage without alpha and cK^-1) ---------------------------
    for (int K = 0; K < nb; ++K) {
        const int k0 = FIT_NB * K, w = k0 + FIT_NB;
        __syncthreads();   // (the previous block's tasks have read PA / PB)
        if (tid < FIT_NB * FIT_NB) {
            const int r = tid / FIT_NB, c = tid % FIT_NB;
            D[r * FIT_LP + c] = c <= r ? A[(int64_t)(k0 + r) * ld + k0 + c] : 0.0;
        }
        for (int idx = tid; idx < FIT_NB * k0; idx += FIT_THREADS) {   // St[j][k] = B[k0 + k][j], j < k0: the pending sums S_K
            const int k = idx / k0, j = idx - k * k0;
            PA[j * FIT_LP + k] = B[(int64_t)(k0 + k) * ld + j];
        }
        __syncthreads();
        if (tid < FIT_NB) {   // column c of L_KK^-1 by forward substitution
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
        // Wt[j][k] = W_K[k][j]:  j < k0: -sum_{m <= k} Wi[k][m] St[j][m];  j = k0 + c: Wi[k][c] (0 above the diagonal).  Row block K of B <- W_K
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
#pragma unroll
            for (int k = 0; k < FIT_NB; ++k) {
                PB[j * FIT_LP + k] = o[k];
                B[(int64_t)(k0 + k) * ld + j] = o[k];
            }
        }
        __syncthreads();   // St has been read: PA takes the column panel K of L, rows w .. M - 1
        for (int li = tid; li < M - w; li += FIT_THREADS) {
            const double* row = A + (int64_t)(w + li) * ld + k0;
#pragma unroll
            for (int c = 0; c < FIT_NB; ++c) PA[li * FIT_LP + c] = row[c];
        }
        __syncthreads();
        // pending sums of the row blocks below: B[w + 16 I][16 Jb] (+)= L_IK W_K, Jb <= K (first touched when Jb == K)
        const int nbelow = nb - K - 1, nacc = nbelow * (K + 1);
        for (int t = wave; t < nacc; t += FIT_THREADS / 64) {
            const int I = t / (K + 1), Jb = t - I * (K + 1);
            fit_task16(B + (int64_t)(w + FIT_NB * I) * ld + FIT_NB * Jb, ld, PA + FIT_NB * I * FIT_LP, PB + FIT_NB * Jb * FIT_LP, lane, 1.0,
                       Jb == K, false, FIT_NB - 1);
        }
    }
}

// fx = 2 dk/dr of the final stage: k_grad_finish's expressions (common.h for the Matérn 1/2 and 3/2 families: 0 at r = 0 for 1/2)
template <bool LOW>
__device__ __forceinline__ double ens_fx(int fam, double sigma2, double r) {
#pragma clang fp contract(off)
    if constexpr (LOW) {
        return matern_lo_fx(fam, sigma2, r);
    } else if (fam == FAM_M52) {
        const double s = sqrt(5.0) * sqrt(r);
        return -(5.0 / 3.0) * sigma2 * (1.0 + s) * exp(-s);
    } else {
        return -(sigma2 * exp(-0.5 * r));
    }
}

// Args = EnsScoreArgs: the value kernel, the code it has always had.  Args = EnsGradArgs: k_ens_grad (below) -- ONE text for the K*'
// tile, the V stage and the finish, so the two give the same mu, sigma^2 and a_h bit for bit; what the gradient adds sits behind
// `if constexpr (GRAD)`.  (The body stays in the kernel: as an inlined device function the value-only code came out different.)
template <int DT, bool LOW, class Args = EnsScoreArgs>
__global__ __launch_bounds__(ENS_THREADS) void k_ens_score(Args a) {
    constexpr bool GRAD = Args::GRAD;
    extern __shared__ double ens_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, M = a.M, ld = a.ld, d = a.d, P = a.P;
    const int nb = M / FIT_NB, kld = M + 1;
    const int64_t h = blockIdx.y, j0 = (int64_t)blockIdx.x * ENS_TC;
    const int nc = (int)(a.R - j0 < ENS_TC ? a.R - j0 : ENS_TC);
    double* const Ks = ens_smem;
    double* const Vs = Ks + ENS_TC * kld;                    // (GRAD)
    double* const zs = GRAD ? Vs + ENS_TC * kld : Ks + ENS_TC * kld;
    double* const als = zs + M;                              // (GRAD)
    double* const il2s = GRAD ? als + M : zs + M;
    double* const xt = il2s + DMAX;
    // value only: the candidates are read for the last time before the barrier behind the K*' tile; the gradient's final stage reads them again
    double* const part = GRAD ? xt + ENS_TC * DT : xt;
    double* const pd = part + 2 * ENS_TC * nb;               // (GRAD) [da/dmu | da/dsigma^2 | sigma^2] x 16
    const int64_t o = h * a.ldr + j0;
    if (a.pivot[h] != 0) {   // the same for every thread
        if (tid < nc) { a.each[o + tid] = NAN; a.mu[o + tid] = NAN; a.var[o + tid] = NAN; }
        if constexpr (GRAD)
            for (int t = tid; t < nc * d; t += ENS_THREADS) a.geach[o * d + t] = NAN;
        return;
    }
    const double* th = a.theta + h * P;
    const int nl = a.iso ? 1 : d;
    const double beta = th[1], sigma2 = exp(2.0 * th[2 + nl]);
    const double* const A = a.ws + h * a.slab;
    const double* const W = A + (int64_t)(M + 1) * ld;
    if (tid < DMAX) il2s[tid] = tid < d ? exp(-2.0 * th[2 + (a.iso ? 0 : tid)]) : 0.0;
    for (int t = tid; t < ENS_TC * DT; t += ENS_THREADS) {
        const int c = t / DT, k = t % DT;
        xt[t] = (c < nc && k < d) ? a.xs[(j0 + c) * d + k] : 0.0;
    }
    for (int i = tid; i < M; i += ENS_THREADS) zs[i] = A[(int64_t)M * ld + i];
    if constexpr (GRAD)
        for (int i = tid; i < M; i += ENS_THREADS) als[i] = a.alpha[h * M + i];
    __syncthreads();

    // ---- K*' tile: Ks[c][i] = k(x_i, xs_c; theta_h), 0 on the padding rows ------------------------------------------------------
    {
#pragma clang fp contract(off)
        for (int i = tid; i < M; i += ENS_THREADS) {
            double r[ENS_TC];
#pragma unroll
            for (int c = 0; c < ENS_TC; ++c) r[c] = 0.0;
            if (i < N) {
                // (the build's sum runs to DT with il2 = 0 beyond d: those terms add +0.0 to a sum that is >= 0, so stopping at d gives
                // the same bits; not unrolled -- 16 running sums per thread are the register budget, DT x 16 unrolled terms spilled)
#pragma unroll 1
                for (int k = 0; k < d; ++k) {
                    const double x = a.X[(int64_t)i * d + k];
                    const double l = il2s[k];
#pragma unroll
                    for (int c = 0; c < ENS_TC; ++c) {
                        const double t = x - xt[c * DT + k];
                        r[c] += l * (t * t);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < ENS_TC; ++c) Ks[c * kld + i] = i < N ? cov_from_r<LOW>(a.fam, sigma2, r[c]) : 0.0;
        }
    }
    __syncthreads();

    // ---- V = W K* block row by block row; per block and candidate sum V^2 and sum V z -------------------------------------------
    {
#pragma clang fp contract(off)
        // lane layout of the 8 x 8 x 4 arrangement (gemm_core.h); the contraction index of instruction s is 4 kq + s, so a lane's four
        // W entries of a block are adjacent in memory
        const int kq = lane >> 4, bb = (lane >> 2) & 3, t = lane & 3;
        const int ar = 4 * (bb >> 1) + t, bc = 4 * (bb & 1) + t;
        const int dr = 4 * (bb >> 1) + (lane >> 4);
        for (int I = nb - 1 - wave; I >= 0; I -= ENS_THREADS / 64) {
            double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
            const double* wrow0 = W + (int64_t)(FIT_NB * I + ar) * ld + 4 * kq;
            const double* wrow1 = wrow0 + (int64_t)8 * ld;
            const double* krow0 = Ks + bc * kld + 4 * kq;
            const double* krow1 = krow0 + 8 * kld;
            for (int J = 0; J <= I; ++J) {
                double av[2][4], bv[2][4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    av[0][s] = wrow0[FIT_NB * J + s];
                    av[1][s] = wrow1[FIT_NB * J + s];
                    bv[0][s] = krow0[FIT_NB * J + s];
                    bv[1][s] = krow1[FIT_NB * J + s];
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = mfma444(av[rb][s], bv[cb][s], acc[rb][cb]);
            }
            const double z0 = zs[FIT_NB * I + dr], z1 = zs[FIT_NB * I + 8 + dr];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                double q = acc[0][cb] * acc[0][cb] + acc[1][cb] * acc[1][cb];
                double m = acc[0][cb] * z0 + acc[1][cb] * z1;
                for (int x = 8; x <= 32; x <<= 1) {   // the lanes that hold the other rows of this column
                    q += __shfl_xor(q, x, 64);
                    m += __shfl_xor(m, x, 64);
                }
                if (lane < 8) {
                    part[(2 * I) * ENS_TC + 8 * cb + lane] = q;
                    part[(2 * I + 1) * ENS_TC + 8 * cb + lane] = m;
                }
            }
            if constexpr (GRAD) {   // V outlives its block: the lane's four entries into the second tile, candidate-major as K*'
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) Vs[(8 * cb + bc) * kld + FIT_NB * I + 8 * rb + dr] = acc[rb][cb];
            }
        }
    }
    __syncthreads();
    if (tid < nc) {
#pragma clang fp contract(off)
        double q = 0.0, m = 0.0;
        for (int I = 0; I < nb; ++I) {
            q += part[(2 * I) * ENS_TC + tid];
            m += part[(2 * I + 1) * ENS_TC + tid];
        }
        double s2 = sigma2 - q;
        if (s2 < 0.0) s2 = 0.0;  // predict_f: max(sigma2, 0)
        const double mu = beta + m;
        a.mu[o + tid] = mu;
        a.var[o + tid] = s2;
        a.each[o + tid] = acq_eval(a.ap, mu, s2);
        if constexpr (GRAD) {
            double dmu, ds2;
            acq_partials(a.ap, mu, s2, dmu, ds2);
            pd[tid] = dmu;
            pd[ENS_TC + tid] = ds2;
            pd[2 * ENS_TC + tid] = s2;
        }
    }
    if constexpr (GRAD) {
        double* const Us = Ks;   // (every wave has read K*' for the last time before the barrier above)
        // ---- U = W' V: block J of U is the sum over I >= J of W_IJ' V_I, I ascending; the arrangement of the V stage with W read transposed
        {
#pragma clang fp contract(off)
            const int kq = lane >> 4, bb = (lane >> 2) & 3, t = lane & 3;
            const int ar = 4 * (bb >> 1) + t, bc = 4 * (bb & 1) + t;
            const int dr = 4 * (bb >> 1) + (lane >> 4);
            for (int J = wave; J < nb; J += ENS_THREADS / 64) {
                double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
                const double* wcol0 = W + (int64_t)(4 * kq) * ld + FIT_NB * J + ar;   // A[r][m] = W[16 I + m][16 J + r], m = 4 kq + s
                const double* vrow0 = Vs + bc * kld + 4 * kq;
                const double* vrow1 = vrow0 + 8 * kld;
                for (int I = J; I < nb; ++I) {
                    double av[2][4], bv[2][4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        av[0][s] = wcol0[(int64_t)(FIT_NB * I + s) * ld];
                        av[1][s] = wcol0[(int64_t)(FIT_NB * I + s) * ld + 8];
                        bv[0][s] = vrow0[FIT_NB * I + s];
                        bv[1][s] = vrow1[FIT_NB * I + s];
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                            for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = mfma444(av[rb][s], bv[cb][s], acc[rb][cb]);
                }
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) Us[(8 * cb + bc) * kld + FIT_NB * J + 8 * rb + dr] = acc[rb][cb];
            }
        }
        __syncthreads();
        // ---- final stage, first half: r and fx again per (observation, candidate); the tiles become fx alpha (V's) and fx U (in place)
        {
#pragma clang fp contract(off)
            for (int i = tid; i < N; i += ENS_THREADS) {
                double r[ENS_TC];
#pragma unroll
                for (int c = 0; c < ENS_TC; ++c) r[c] = 0.0;
#pragma unroll 1
                for (int k = 0; k < d; ++k) {   // (rolled, as the K*' tile and for its reason; the same r bit for bit)
                    const double x = a.X[(int64_t)i * d + k];
                    const double l = il2s[k];
#pragma unroll
                    for (int c = 0; c < ENS_TC; ++c) {
                        const double t = x - xt[c * DT + k];
                        r[c] += l * (t * t);
                    }
                }
                const double al = als[i];
#pragma unroll
                for (int c = 0; c < ENS_TC; ++c) {
                    const double fx = ens_fx<LOW>(a.fam, sigma2, r[c]);
                    Vs[c * kld + i] = fx * al;
                    Us[c * kld + i] = fx * Us[c * kld + i];
                }
            }
        }
        __syncthreads();
        // ---- final stage, second half: thread (candidate c, coordinates k = t, t + 16, ...) adds its two sums over the observations in
        // ascending order -- the order does not depend on the candidate's slot -- and applies the chain rule
        {
#pragma clang fp contract(off)
            constexpr int KPT = (DT + 15) / 16;
            const int c = tid >> 4, t = tid & 15;
            double gm[KPT], gv[KPT], xc[KPT], il[KPT];
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const int k = t + 16 * q;
                gm[q] = 0.0;
                gv[q] = 0.0;
                xc[q] = k < d ? xt[c * DT + k] : 0.0;
                il[q] = k < d ? il2s[k] : 0.0;
            }
            if (t < d) {
                const double* pa = Vs + c * kld;
                const double* pu = Us + c * kld;
#pragma unroll 8
                for (int j = 0; j < N; ++j) {
                    const double p = pa[j], u = pu[j];
#pragma unroll
                    for (int q = 0; q < KPT; ++q) {
                        const int k = t + 16 * q;
                        const double dx = (xc[q] - (k < d ? a.X[(int64_t)j * d + k] : 0.0)) * il[q];
                        gm[q] += p * dx;
                        gv[q] += u * dx;
                    }
                }
                if (c < nc) {
                    const double dmu = pd[c], ds2 = pd[ENS_TC + c], s2 = pd[2 * ENS_TC + c];
#pragma unroll
                    for (int q = 0; q < KPT; ++q) {
                        const int k = t + 16 * q;
                        // a clamped variance (sigma^2 == 0 exactly) has zero gradient (k_grad_finish)
                        if (k < d) a.geach[(o + c) * d + k] = dmu * gm[q] + (s2 > 0.0 ? ds2 * (-2.0 * gv[q]) : 0.0);
                    }
                }
            }
        }
    }
}


template <int DT, bool LOW>
constexpr auto k_ens_grad = &k_ens_score<DT, LOW, EnsGradArgs>;

// alpha_h = W' z of every setting of a launch, behind k_ens_factor: one workgroup per setting, thread = column j, the rows i >= j added
// in ascending order.  A failed setting's block is left as it is (k_ens_grad does not read it).
__global__ __launch_bounds__(256) void k_ens_alpha(const double* __restrict__ ws, const long long* __restrict__ pivot, double* __restrict__ alpha,
                                                   long long slab, int M, int ld) {
#pragma clang fp contract(off)
    const int64_t h = blockIdx.x;
    if (pivot[h] != 0) return;   // the same for every thread
    const double* const A = ws + h * slab;
    const double* const W = A + (int64_t)(M + 1) * ld;
    const double* const z = A + (int64_t)M * ld;
    for (int j = threadIdx.x; j < M; j += 256) {
        double s = 0.0;
#pragma unroll 8
        for (int i = j; i < M; ++i) s += W[(int64_t)i * ld + j] * z[i];
        alpha[h * M + j] = s;
    }
}

// w~_h = w_h / (sum of w over the settings whose factorisation succeeded, ascending h); 0 for a failed setting.  w null: equal weights.
__global__ void k_ens_weights(const double* __restrict__ w, const long long* __restrict__ pivot, long long H, double* __restrict__ wt) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (long long h = 0; h < H; ++h)
        if (pivot[h] == 0) s += w ? w[h] : 1.0;
    for (long long h = 0; h < H; ++h) wt[h] = pivot[h] == 0 ? (w ? w[h] : 1.0) / s : 0.0;
}

// scores[j] = sum_h w~_h each[h][j], sequentially in ascending h; a setting of weight 0 takes no part (so 0 x -Inf never appears)
__global__ __launch_bounds__(256) void k_ens_reduce(const double* __restrict__ each, long long ldr, const double* __restrict__ wt, long long H,
                                                    long long R, long long j_off, double* __restrict__ scores, Best* __restrict__ block_best) {
#pragma clang fp contract(off)
    __shared__ Best sh[4];
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    double v = -INFINITY;
    long long idx = -1;
    if (j < R) {
        double s = 0.0;
        for (long long h = 0; h < H; ++h) {
            const double w = wt[h];
            if (w != 0.0) s += w * each[h * ldr + j];
        }
        scores[j_off + j] = s;
        if (s > -INFINITY) { v = s; idx = j_off + j; }   // false for NaN and -Inf
    }
    block_argmax(v, idx, sh);
    if (threadIdx.x == 0) { block_best[blockIdx.x].val = idx >= 0 ? v : -INFINITY; block_best[blockIdx.x].idx = idx; }
}

// grad[j][k] = sum_h w~_h geach[h][j][k] with k_ens_reduce's rule; thread = one of the n = R d entries of the chunk (rows are contiguous)
__global__ __launch_bounds__(256) void k_ens_reduce_grad(const double* __restrict__ geach, long long plane, const double* __restrict__ wt,
                                                         long long H, long long n, double* __restrict__ grad) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (long long h = 0; h < H; ++h) {
        const double w = wt[h];
        if (w != 0.0) s += w * geach[h * plane + e];
    }
    grad[e] = s;
}

}  // namespace bohip
