// kernels_loo.hip -- leave-one-out cross-validation of the resident model (include/bohip_loo.h): role of
// GaussianProcesses.jl predict_LOO / logp_LOO / dlogpdtheta_LOO (Rasmussen & Williams 5.4.2).  Included by bohip.hip after the
// linear algebra (KernelHyper, the family expressions, d2).  With kappa_i = [cK^-1]_ii:
//     mu_-i = y_i - alpha_i / kappa_i,   var_-i = 1 / kappa_i,   logp_i = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi
//   k_loo_kappa    kappa_i = sum_{k >= i} W'[i][k]^2: one pass over the upper triangle of the resident W', no cK^-1
//   k_loo_finish   mu, var, logp per point, their sum in a fixed order, and q = alpha / kappa, sqrt(c) for the gradient
//   k_loo_scale    Z = cK^-1 diag(sqrt c) from the lower-stored cK^-1, mirrored while reading
//   k_dloo_parts   sum_ab D_ab G_ab, G = 1/2 (b alpha' + alpha b') - M, M = Z Z': k_dmll_parts' pass with another weight matrix
#pragma once

namespace bohip {

// kappa[i] = sum_{i <= k < N} WT[i][k]^2.  One wave per row, four rows per workgroup.  Lane l takes the 16-byte pieces at columns
// (i & ~1) + 2 l + 128 t, t = 0, 1, ... and adds x^2 then y^2 of each piece in that order; the 64 lanes are combined by a
// butterfly.  The order depends on (i, N) only.  What lies left of the diagonal (the odd-row piece starts one column early) and
// from column N on is masked by index: those entries belong to other code and are never used as numbers.
__global__ __launch_bounds__(256) void k_loo_kappa(const double* __restrict__ WT, int64_t ld, int64_t N, double* __restrict__ kappa) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;   // (whole waves leave: no barrier below)
    const double* row = WT + i * ld;
    double s = 0.0;
#pragma unroll 4
    for (int64_t k = (i & ~(int64_t)1) + 2 * lane; k < N; k += 128) {   // k even, k + 1 <= N < ld: the piece lies inside the row
        const d2 v = *reinterpret_cast<const d2*>(row + k);
        const double x = k >= i ? v.x : 0.0, y = k + 1 < N ? v.y : 0.0;
        s += x * x;
        s += y * y;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) kappa[i] = s;
}

// Per point: mu, var, logp (kept on the device; the host copies what the caller asked for), q = alpha / kappa and
// sc = sqrt(c), c = 1/2 (1 / kappa + alpha^2 / kappa^2) > 0.  out[0] = sum_i logp_i: single workgroup, fixed order (the shape of k_mll).
__global__ __launch_bounds__(256) void k_loo_finish(const double* __restrict__ y, const double* __restrict__ alpha,
                                                    const double* __restrict__ kappa, int64_t N, double* __restrict__ mu,
                                                    double* __restrict__ var, double* __restrict__ logp, double* __restrict__ q,
                                                    double* __restrict__ sc, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const double kp = kappa[i], a = alpha[i], v = 1.0 / kp, qi = a * v;
        const double lp = 0.5 * log(kp) - 0.5 * a * qi - 0.5 * log(2.0 * M_PI);
        mu[i] = y[i] - qi;
        var[i] = v;
        logp[i] = lp;
        q[i] = qi;
        sc[i] = sqrt(0.5 * (v + qi * qi));
        s += lp;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// Z[i][k] = cK^-1[i][k] sc[k] for i, k < N, literal zeros from N up to the padded edge Np (a multiple of 64).  S holds cK^-1 in
// its lower triangle only: entry (i, k) is read at (max, min), so nothing with column > row is touched, inside diagonal tiles too.
// Workgroup = one 64 x 64 tile of Z; its source tile goes through LDS so that the mirrored tiles are read along rows as well.
__global__ __launch_bounds__(256) void k_loo_scale(const double* __restrict__ S, int64_t ld, int64_t N, const double* __restrict__ sc,
                                                   double* __restrict__ Z) {
    __shared__ double tile[64][65];
    const int bi = blockIdx.y, bj = blockIdx.x;
    const int si = max(bi, bj), sj = min(bi, bj);   // the stored tile
    const int tc = (threadIdx.x & 31) * 2, tr = threadIdx.x >> 5;
    for (int r = tr; r < 64; r += 8) {
        const int64_t gr = (int64_t)si * 64 + r, gc = (int64_t)sj * 64 + tc;
        double x = 0.0, y = 0.0;
        if (gr < N) {
            if (gc + 1 <= gr) {   // both entries on or below the diagonal (gc + 1 <= gr < N)
                const d2 v = *reinterpret_cast<const d2*>(S + gr * ld + gc);
                x = v.x; y = v.y;
            } else if (gc <= gr) {
                x = S[gr * ld + gc];
            }
        }
        tile[r][tc] = x;
        tile[r][tc + 1] = y;
    }
    __syncthreads();
    for (int r = tr; r < 64; r += 8) {
        const int64_t gr = (int64_t)bi * 64 + r, gc = (int64_t)bj * 64 + tc;
        d2 v = {0.0, 0.0};
        if (gr < N) {
            // (a diagonal tile holds its lower half: take (r, c) from there when c <= r, from (c, r) otherwise)
            const bool lo0 = bj < bi || (bj == bi && tc <= r), lo1 = bj < bi || (bj == bi && tc + 1 <= r);
            if (gc < N) v.x = (lo0 ? tile[r][tc] : tile[tc][r]) * sc[gc];
            if (gc + 1 < N) v.y = (lo1 ? tile[r][tc + 1] : tile[tc + 1][r]) * sc[gc + 1];
        }
        *reinterpret_cast<d2*>(Z + gr * ld + gc) = v;
    }
}

// d L / d theta = sum_ab D_ab G_ab with G = 1/2 (b alpha' + alpha b') - M, D = d cK / d theta: the pass of k_dmll_parts (same grid,
// same thread = column / block = rows walk, same partial layout [block][NP] for k_dmll_final) with G formed on the fly from b,
// alpha and the lower-stored M.  The lower triangle is walked once, so an off-diagonal entry counts twice and the diagonal once.
// The mean slot is sum_i b_i.  The per-family expressions restate those of k_dmll_parts, which stays as it is.
template <int DT, bool LOW>
__global__ __launch_bounds__(256) void k_dloo_parts(const double* __restrict__ X, int64_t N, KernelHyper hp, double noise_var,
                                                    const double* __restrict__ M, int64_t ld, const double* __restrict__ alpha,
                                                    const double* __restrict__ b, int rows_per_block, double* __restrict__ parts) {
    const int d = hp.d, NP = d + 3;
    const int64_t j = blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t i1 = min(N, i0 + rows_per_block);
    double* out = parts + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NP;
    if ((int64_t)blockIdx.x * 256 > i1 - 1) {   // block entirely above the diagonal
        for (int k = threadIdx.x; k < NP; k += 256) out[k] = 0.0;
        return;
    }
    double xj[DT], acc[DT], a_sig = 0.0, a_noise = 0.0, a_mean = 0.0;
#pragma unroll
    for (int k = 0; k < DT; ++k) {
        xj[k] = (j < N && k < d) ? X[j * d + k] : 0.0;
        acc[k] = 0.0;
    }
    const double aj = j < N ? alpha[j] : 0.0, bj = j < N ? b[j] : 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        if (j > i) continue;   // (j <= i < N)
        const double ai = alpha[i], bi = b[i];
        const double G = i == j ? ai * bi - M[i * ld + j] : (bi * aj + ai * bj) - 2.0 * M[i * ld + j];
        double t[DT], r = 0.0;
#pragma unroll
        for (int k = 0; k < DT; ++k) {
            const double dx = (k < d) ? X[i * d + k] - xj[k] : 0.0;
            t[k] = (k < d) ? hp.il2[k] * (dx * dx) : 0.0;
            r += t[k];
        }
        double Kij, fac;
        if constexpr (LOW) {
            Kij = matern_lo_k(hp.fam, hp.sigma2, r);
            fac = -matern_lo_fx(hp.fam, hp.sigma2, r);   // 0 on the diagonal for M12, whose limit there is 0
        } else if (hp.fam == FAM_M52) {
            const double sq = sqrt(5.0) * sqrt(r), e = exp(-sq);
            Kij = hp.sigma2 * (1.0 + sq + 5.0 / 3.0 * r) * e;
            fac = 5.0 / 3.0 * hp.sigma2 * (1.0 + sq) * e;
        } else {
            Kij = hp.sigma2 * exp(-0.5 * r);
            fac = Kij;
        }
        const double gf = G * fac;
#pragma unroll
        for (int k = 0; k < DT; ++k) acc[k] += gf * t[k];
        a_sig += G * 2.0 * Kij;
        if (i == j) {
            a_noise += G * 2.0 * noise_var;
            a_mean += bi;
        }
    }
    // block reduction of NP accumulators: wave shuffles, then 4 wave leaders through LDS
    __shared__ double red[4][DMAX + 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto wsum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
    a_noise = wsum(a_noise); a_mean = wsum(a_mean); a_sig = wsum(a_sig);
#pragma unroll
    for (int k = 0; k < DT; ++k) acc[k] = wsum(acc[k]);
    if (lane == 0) {
        red[wave][0] = a_noise; red[wave][1] = a_mean;
#pragma unroll
        for (int k = 0; k < DT; ++k) if (k < d) red[wave][2 + k] = acc[k];
        red[wave][2 + d] = a_sig;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NP; k += 256) out[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

}  // namespace bohip
