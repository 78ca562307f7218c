// kernels_qei_joint.hip -- the joint q-EI of B batches of q points and its gradient in every point (include/bohip_qei_joint.h,
// DESIGN.md 6z).  Per group b (rows b q .. b q + q - 1 of the one K*' chunk), with V' and U' = V'W of the posterior pass:
//     Sigma = K(X_b, X_b) - V_b V_b',   L L' = Sigma + jitter I,   f_s = mu + L z_s,   value = (1 / S) sum_s [f_s,j* > tau] (f_s,j* - tau)
//     grad_j = sum_n dk(x_j, X_n)/dx e_j[n] + 2 sum_{i != j} Sbar_ji dk(x_j, x_i)/dx_j,   e_j = mubar_j alpha - 2 sum_i Sbar_ji u_i
//   k_qeij_normals   Z [S][16] = bohip_thompson_normal(seed, s, i), once per call, shared by every group
//   k_qeij_cov       ONE WORKGROUP per group, a batched small SYRK: the group's q rows of V' stream through LDS in panels of 256
//                    observations (rows q .. 15 zero), each of the four waves takes its 64 columns of every panel and accumulates the
//                    16 x 16 tile as four v_mfma_f64_4x4x4 accumulators (instruction m: rows 4m .. 4m + 3 against all 16 rows, one
//                    4 x 4 block of the output a block of the instruction); the four partial tiles are added in wave order in LDS
//   k_qeij_core      ONE WORKGROUP per group: thread (j, i) of the lower triangle factors Sigma in LDS, right-looking, a barrier a
//                    column, with the update written c_j (c_i / d) so that a repeated point cancels to a pivot that is never positive;
//                    then thread = sample over tiles of 256 samples of Z in LDS (f_s, j*_s, a_s: one byte and one gain a sample);
//                    then thread (j, i) walks the tile's samples in ascending s and adds g z_s,i where j*_s = j (no lane indexes a
//                    register array by j*: nothing goes to scratch); then L^-1, Phi(L'Lbar) and Sbar = sym(L^-T Phi L^-1) in LDS
//   k_qeij_mix       E over U' in place: a wave takes the group's 16 rows x 16 columns of U' into registers (the lane that reads
//                    U'[4k + l / 16][c + l % 16] writes the same four places), multiplies by -2 Sbar with sixteen MFMAs on top of
//                    mubar_j alpha[n], and writes its rows back; rows >= q are neither read nor written, columns >= N leave as zero
//   k_qeij_direct    thread = point: grad[r] += 2 sum_{i != j} Sbar_ji dk(x_j, x_i)/dx_j in ascending i, after the stream's sum
// The contraction of E with dk/dx is k_nei_grad_finish, launched as it stands.  Contraction is off, no atomics, every sum has one
// writer and a fixed order; a group's bytes depend on its own rows alone.
// Included by bohip.hip after kernels_nei_grad.hip (mfma444, thompson_normal, cov_from_r, pend_fx).
#pragma once
#include "common.h"
#include "gemm_core.h"

namespace bohip {

constexpr int QEIJ_Q = 16;          // BOHIP_QEIJ_QMAX: rows of a group's padded tile
constexpr int QEIJ_SMAX = 1024;     // BOHIP_QEIJ_SMAX
constexpr int QEIJ_TRI = QEIJ_Q * (QEIJ_Q + 1) / 2;   // 136 threads of the lower triangle
constexpr int QEIJ_PANEL = 256;     // observations per LDS panel of k_qeij_cov: 64 per wave
constexpr int QEIJ_PLS = QEIJ_PANEL + 4;   // its row stride: rows 8 banks apart, 16-byte aligned
constexpr int QEIJ_LS = QEIJ_Q + 1;        // row stride of the 16 x 16 matrices of k_qeij_core
constexpr int QEIJ_ST = 256;        // samples per tile of k_qeij_core: one per thread
static_assert(QEIJ_TRI <= 256 && QEIJ_Q * QEIJ_Q == 256, "one thread per entry of the tile");

__global__ __launch_bounds__(256) void k_qeij_normals(uint64_t seed, int S, double* __restrict__ Z) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < S * QEIJ_Q) Z[e] = thompson_normal(seed, e / QEIJ_Q, e % QEIJ_Q);
}

template <bool LOW>
__global__ __launch_bounds__(256) void k_qeij_cov(const double* __restrict__ VT, int64_t ld, int64_t N, const double* __restrict__ Xs, int q,
                                                  KernelHyper hp, double* __restrict__ Sig) {
#pragma clang fp contract(off)
    __shared__ double vl[QEIJ_Q * QEIJ_PLS];
    __shared__ double part[4][QEIJ_Q * QEIJ_Q];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * q;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t n0 = 0; n0 < N; n0 += QEIJ_PANEL) {
        __syncthreads();
        for (int e = threadIdx.x; e < QEIJ_Q * QEIJ_PANEL; e += 256) {   // a row of the panel is 256 consecutive doubles of V'
            const int row = e / QEIJ_PANEL, col = e % QEIJ_PANEL;
            vl[row * QEIJ_PLS + col] = (row < q && n0 + col < N) ? VT[(r0 + row) * ld + n0 + col] : 0.0;
        }
        __syncthreads();
        const double* v = vl + wave * 64 + (lane >> 4);
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            const double b = v[(lane & 15) * QEIJ_PLS + 4 * kk];
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (4 * m < q) acc[m] = mfma444(v[(4 * m + (lane & 3)) * QEIJ_PLS + 4 * kk], b, acc[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) part[wave][(4 * m + (lane >> 4)) * QEIJ_Q + (lane & 15)] = acc[m];
    __syncthreads();
    const int t = threadIdx.x, j = t / QEIJ_Q, i = t % QEIJ_Q;
    double out = 0.0;
    if (j < q && i < q) {
        const double vv = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
        const double *xj = Xs + (r0 + j) * hp.d, *xi = Xs + (r0 + i) * hp.d;
        double rr = 0.0;
        for (int k = 0; k < hp.d; ++k) {
            const double dx = xj[k] - xi[k];
            rr += hp.il2[k] * (dx * dx);
        }
        out = cov_from_r<LOW>(hp.fam, hp.sigma2, rr) - vv;
    }
    Sig[(int64_t)blockIdx.x * (QEIJ_Q * QEIJ_Q) + t] = out;
}

struct QeijCore {
    const double* Sig;    // [B][16][16]
    const double* mu;     // [R] latent posterior mean
    const double* Z;      // [S][16]
    int q, S;
    double tau, jitter;   // jitter = jitter_rel sigma_f^2
    double* value;        // [B]
    long long* pivot;     // [B]
    double* mubar;        // [R]
    double* Sbar;         // [B][16][16]
};

__global__ __launch_bounds__(256) void k_qeij_core(QeijCore a) {
#pragma clang fp contract(off)
    __shared__ double A[QEIJ_Q * QEIJ_LS], L[QEIJ_Q * QEIJ_LS], Lb[QEIJ_Q * QEIJ_LS], Li[QEIJ_Q * QEIJ_LS], P[QEIJ_Q * QEIJ_LS],
        T[QEIJ_Q * QEIJ_LS];
    __shared__ double zl[QEIJ_ST * QEIJ_LS];
    __shared__ double gain[QEIJ_ST];
    __shared__ unsigned char code[QEIJ_ST];
    __shared__ double mul[QEIJ_Q];
    const int t = threadIdx.x, q = a.q, S = a.S;
    const int64_t b = blockIdx.x;
    // thread t < 136 owns (j, i), j >= i, of the lower triangle; every thread also owns (fj, fi) of the full tile
    int j = 0;
    while ((j + 1) * (j + 2) / 2 <= t) ++j;
    const int i = t - j * (j + 1) / 2;
    const bool tri = t < QEIJ_TRI && j < q;
    const int fj = t / QEIJ_Q, fi = t % QEIJ_Q;
    {
        const double s = a.Sig[b * (QEIJ_Q * QEIJ_Q) + t];
        A[fj * QEIJ_LS + fi] = fj == fi && fj < q ? s + a.jitter : s;
        L[fj * QEIJ_LS + fi] = 0.0; Lb[fj * QEIJ_LS + fi] = 0.0; Li[fj * QEIJ_LS + fi] = 0.0;
        P[fj * QEIJ_LS + fi] = 0.0; T[fj * QEIJ_LS + fi] = 0.0;   // (upper triangles and padding stay zero)
        if (t < QEIJ_Q) mul[t] = t < q ? a.mu[b * q + t] : 0.0;
    }
    __syncthreads();
    // right-looking: at column k every (j, i) with i > k takes c_j (c_i / d) off; column k itself is left unscaled until the end
    int bad = 0;
    for (int k = 0; k < q; ++k) {
        const double d = A[k * QEIJ_LS + k];
        if (!(d > 0.0) || d == INFINITY) { bad = k + 1; break; }   // (the same word for every thread)
        if (tri && i > k) A[j * QEIJ_LS + i] = A[j * QEIJ_LS + i] - A[j * QEIJ_LS + k] * (A[i * QEIJ_LS + k] / d);
        __syncthreads();
    }
    if (bad) {   // flagged: -Inf, a zero gradient
        if (t == 0) { a.value[b] = -INFINITY; a.pivot[b] = bad; }
        if (t < q) a.mubar[b * q + t] = 0.0;
        a.Sbar[b * (QEIJ_Q * QEIJ_Q) + t] = 0.0;
        return;
    }
    if (tri) L[j * QEIJ_LS + i] = A[j * QEIJ_LS + i] / sqrt(A[i * QEIJ_LS + i]);
    const double g = 1.0 / (double)S;
    double lbar = 0.0, mb = 0.0, vsum = 0.0;   // thread (j, i): Lbar_ji; i == j: mubar_j as well; thread 255: the value
    for (int s0 = 0; s0 < S; s0 += QEIJ_ST) {
        const int ns = min(QEIJ_ST, S - s0);
        __syncthreads();
        for (int e = t; e < ns * QEIJ_Q; e += 256) zl[(e / QEIJ_Q) * QEIJ_LS + e % QEIJ_Q] = a.Z[(int64_t)s0 * QEIJ_Q + e];
        __syncthreads();
        if (t < ns) {   // f = mu + L z, row by row; the first maximum under strict '>'
            const double* z = zl + t * QEIJ_LS;
            double best = 0.0;
            int js = 0;
            for (int r = 0; r < q; ++r) {
                double f = mul[r];
                for (int k = 0; k <= r; ++k) f = f + L[r * QEIJ_LS + k] * z[k];
                if (r == 0 || f > best) { best = f; js = r; }
            }
            const bool hit = best > a.tau;
            code[t] = (unsigned char)(hit ? 0x80 | js : js);
            gain[t] = hit ? best - a.tau : 0.0;
        }
        __syncthreads();
        if (tri) {
            const unsigned char want = (unsigned char)(0x80 | j);
            for (int s = 0; s < ns; ++s)
                if (code[s] == want) {
                    lbar = lbar + g * zl[s * QEIJ_LS + i];
                    if (i == j) mb = mb + g;
                }
        } else if (t == 255) {
            for (int s = 0; s < ns; ++s) vsum = vsum + gain[s];
        }
    }
    if (tri) Lb[j * QEIJ_LS + i] = lbar;
    if (tri && i == j) a.mubar[b * q + j] = mb;
    if (t == 255) { a.value[b] = vsum / (double)S; a.pivot[b] = 0; }
    __syncthreads();
    // P = Phi(L'Lbar) by thread (j, i); column t of L^-1 by thread t < q, forward substitution
    if (tri) {
        double p = 0.0;
        for (int k = j; k < q; ++k) p = p + L[k * QEIJ_LS + j] * Lb[k * QEIJ_LS + i];
        P[j * QEIJ_LS + i] = i == j ? 0.5 * p : p;
    } else if (t >= 192 && t - 192 < q) {
        const int c = t - 192;
        Li[c * QEIJ_LS + c] = 1.0 / L[c * QEIJ_LS + c];
        for (int r = c + 1; r < q; ++r) {
            double s = 0.0;
            for (int k = c; k < r; ++k) s = s + L[r * QEIJ_LS + k] * Li[k * QEIJ_LS + c];
            Li[r * QEIJ_LS + c] = -s / L[r * QEIJ_LS + r];
        }
    }
    __syncthreads();
    // T = P L^-1 (lower), M = L^-T T (full), Sbar = (M + M') / 2
    if (tri) {
        double s = 0.0;
        for (int k = i; k <= j; ++k) s = s + P[j * QEIJ_LS + k] * Li[k * QEIJ_LS + i];
        T[j * QEIJ_LS + i] = s;
    }
    __syncthreads();
    double m = 0.0;
    if (fj < q && fi < q)
        for (int k = max(fj, fi); k < q; ++k) m = m + Li[k * QEIJ_LS + fj] * T[k * QEIJ_LS + fi];
    A[fj * QEIJ_LS + fi] = m;   // (Sigma's tile is dead)
    __syncthreads();
    a.Sbar[b * (QEIJ_Q * QEIJ_Q) + t] = 0.5 * (A[fj * QEIJ_LS + fi] + A[fi * QEIJ_LS + fj]);
}

// E[b q + j][n] = mubar_j alpha[n] - 2 sum_i Sbar_ji U'[b q + i][n] over U' in place; grid (B, column blocks of 64), a wave = 16 columns
__global__ __launch_bounds__(256) void k_qeij_mix(const double* __restrict__ Sbar, const double* __restrict__ mubar,
                                                  const double* __restrict__ alpha, int q, int64_t N, int64_t Npad, double* __restrict__ E,
                                                  int64_t lde) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane >> 4, lc = lane & 15;
    const int64_t b = blockIdx.x, n = ((int64_t)blockIdx.y * 4 + wave) * 16 + lc;
    if (n - lc >= Npad) return;   // (the whole wave)
    double* e = E + b * q * lde + n;
    double u[4], mb[4], acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // the tile: rows 4k + lr, read before anything is written
        const bool live = 4 * k + lr < q && n < N;
        u[k] = live ? e[(int64_t)(4 * k + lr) * lde] : 0.0;
        mb[k] = 4 * k + lr < q ? mubar[b * q + 4 * k + lr] : 0.0;
    }
    const double al = n < N ? alpha[n] : 0.0;
    const double* sb = Sbar + b * (QEIJ_Q * QEIJ_Q);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        acc[m] = mb[m] * al;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[m] = mfma444(-2.0 * sb[(4 * m + (lane & 3)) * QEIJ_Q + 4 * k + lr], u[k], acc[m]);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
        if (4 * m + lr < q) e[(int64_t)(4 * m + lr) * lde] = n < N ? acc[m] : 0.0;
}

// grad[r][k] += 2 sum_{i != j} Sbar_ji fx(r_ji) il2_k (x_jk - x_ik), i ascending; r = b q + j
template <int DT, bool LOW>
__global__ __launch_bounds__(64) void k_qeij_direct(const double* __restrict__ Xs, int64_t R, int q, KernelHyper hp,
                                                    const double* __restrict__ Sbar, double* __restrict__ grad) {
#pragma clang fp contract(off)
    const int d = hp.d;
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int64_t b = r / q;
    const int j = (int)(r % q);
    double x[DT], ge[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) {
        x[k] = k < d ? Xs[r * d + k] : 0.0;
        ge[k] = k < d ? grad[r * d + k] : 0.0;
    }
    const double* sb = Sbar + b * (QEIJ_Q * QEIJ_Q) + j * QEIJ_Q;
    for (int i = 0; i < q; ++i) {
        if (i == j) continue;
        const double* xi = Xs + (b * q + i) * d;
        double dx[DT], rr = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) {
                dx[k] = x[k] - xi[k];
                rr += hp.il2[k] * (dx[k] * dx[k]);
            }
        const double fac = pend_fx<LOW>(hp, rr), w = 2.0 * sb[i];
#pragma unroll
        for (int k = 0; k < DT; ++k)
            if (k < d) ge[k] += fac * dx[k] * hp.il2[k] * w;
    }
#pragma unroll
    for (int k = 0; k < DT; ++k)
        if (k < d) grad[r * d + k] = ge[k];
}

}  // namespace bohip
