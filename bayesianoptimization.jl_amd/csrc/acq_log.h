// acq_log.h -- LogEI: the logarithm of the TEXTBOOK expected improvement and its partials, finite and accurate for any z
// (Ament et al., "Unexpected Improvements to Expected Improvement", NeurIPS 2023).  An extension: the reference
// has no such functor.  Included ahead of kernels_score.hip, whose acq_eval / acq_partials call it for ACQ_LOGEI.
//
//   sigma = sqrt(s2), z = (mu - tau) / sigma, h(z) = phi(z) + z Phi(z), c = log(2 pi) / 2
//   LogEI(mu, s2, tau) = log sigma + log h(z)
//   d/dmu  = Phi(z) / (sigma h(z))
//   d/ds2  = phi(z) / (2 s2 h(z))            (h - z Phi = phi: strictly positive)
//   s2 == 0:  value = mu > tau ? log(mu - tau) : -inf;  d/dmu = mu > tau ? 1 / (mu - tau) : 0;  d/ds2 = 0
//
// logei_parts(z) returns log h, Phi / h and phi / h.
//   z > -4   direct: phi = exp(-z^2/2) / sqrt(2 pi), Phi = erfc(-z / sqrt 2) / 2, h = phi + z Phi (cancels at most ~20x at -4).
//   z <= -4  t = -z, Mills' ratio m(t) = Phi(z) / phi(z) = 1 / (t + 1 / (t + 2 / (t + 3 / (t + ...)))) from its continued
//            fraction, bottom-up at the fixed depth LOGEI_CF_DEPTH:  r = 2 / (t + 3 / (t + ...)),  c1 = 1 / (t + r),  m = 1 / (t + c1).
//            h / phi = 1 - t m = c1 / (t + c1) needs no subtraction, and the two ratios need no division by it:
//                Phi / h = m / (c1 m) = t + r          phi / h = (t + c1) / c1 = (t + c1) (t + r)
//            so t = +inf gives (-inf, +inf, +inf) and no NaN.  log h = -z^2/2 - c + log(c1 / (t + c1)).
// Contraction is off, as in acq_eval: tests/logei_reference.py is the NumPy twin, operation for operation.
#pragma once
#include "common.h"

namespace bohip {

constexpr double LOGEI_SWITCH = -4.0;
constexpr int LOGEI_CF_DEPTH = 40;

__device__ __forceinline__ void logei_parts(double z, double& logh, double& Phi_h, double& phi_h) {
#pragma clang fp contract(off)
    if (z > LOGEI_SWITCH) {
        const double phi = 0.3989422804014327 * exp(-0.5 * (z * z));
        const double Phi = 0.5 * erfc(-z / 1.4142135623730951);
        const double h = phi + z * Phi;
        logh = log(h);
        Phi_h = Phi / h;
        phi_h = phi / h;
        return;
    }
    const double t = -z;
    double r = 0.0;
#pragma unroll 1
    for (int k = LOGEI_CF_DEPTH; k >= 2; --k) r = (double)k / (t + r);
    const double tr = t + r, c1 = 1.0 / tr, tc = t + c1;
    logh = -0.5 * (z * z) - 0.9189385332046728 + log(c1 / tc);
    Phi_h = tr;
    phi_h = tc * tr;
}

// The two bodies are NOT inlined: acq_eval / acq_partials sit inside kernels at their register limit (k_small_v / k_small_u, the
// one-workgroup ascent, k_grad_finish), and erfc, exp, log and the division loop inlined there cost up to 56 VGPRs, an occupancy
// step in three kernels and scratch in two (profiles/logei_resources.txt).  As calls they cost ids 0-4 nothing, and only a
// LogEI call pays the jump.  Results travel by value, in registers: reference parameters would put them on the stack.
struct LogEIPartials { double dmu, ds2; };

__device__ __noinline__ double logei_value(double mu, double s2, double tau) {
#pragma clang fp contract(off)
    if (s2 == 0.0) return mu > tau ? log(mu - tau) : -INFINITY;
    const double s = sqrt(s2);
    double logh, a, b;
    logei_parts((mu - tau) / s, logh, a, b);
    return log(s) + logh;
}

__device__ __noinline__ LogEIPartials logei_partials(double mu, double s2, double tau) {
#pragma clang fp contract(off)
    if (s2 == 0.0) return {mu > tau ? 1.0 / (mu - tau) : 0.0, 0.0};
    const double s = sqrt(s2);
    double logh, a, b;
    logei_parts((mu - tau) / s, logh, a, b);
    return {a / s, b / (2.0 * s2)};
}

}  // namespace bohip
