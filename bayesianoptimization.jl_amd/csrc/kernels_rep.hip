// kernels_rep.hip -- replicated sites (include/bohip_rep.h): r_i evaluations at one position enter the model as ONE row,
// their mean with the noise term nu / r_i.  Two small kernels, launched for weighted handles only; k_build_cov, k_cov_rows and every
// factorisation kernel stay as they are and an unweighted handle launches none of this.
//   k_rep_diag        cK_w[i][i] = sigma_f^2 + noise / r_i over rows [i0, i1): behind k_build_cov (all rows) and k_cov_rows (the new ones)
//   k_rep_noise_sum   sum_i (alpha_i^2 - (cK_w^-1)_ii) / r_i, one workgroup, fixed order: the logNoise slot of the gradient
#pragma once

namespace bohip {

// Every supported kernel is stationary: k(x, x) = sigma_f^2 exactly (cov_from_r at r = 0), so the diagonal entry is rewritten whole
// rather than corrected.  invr[i] = 1 / r_i, 1.0 for a plain row -- which then keeps the bits k_build_cov gave it.
__global__ __launch_bounds__(256) void k_rep_diag(double* __restrict__ L, int64_t ld, int64_t i0, int64_t i1, double sigma2,
                                                  double noise, const double* __restrict__ invr) {
#pragma clang fp contract(off)
    const int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < i1) L[i * ld + i] = sigma2 + noise * invr[i];
}

// out[0] = sum_i (alpha_i^2 - Kinv[i][i]) invr[i]   (Kinv: the lower tiles of cK_w^-1 that kinv_into_scratch leaves in dS)
__global__ __launch_bounds__(256) void k_rep_noise_sum(const double* __restrict__ alpha, const double* __restrict__ Kinv, int64_t ld,
                                                       int64_t N, const double* __restrict__ invr, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) s += (alpha[i] * alpha[i] - Kinv[i * ld + i]) * invr[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

}  // namespace bohip
