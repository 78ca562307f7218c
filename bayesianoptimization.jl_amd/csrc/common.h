// common.h -- shared constants and small helpers for the gfx950 (CDNA4) kernels of libbohip.
// Everything here is FP64: the acceptance bar is 1e-6 relative on sigma^2 = s_f^2 - v'v, which
// cancels catastrophically near observations, so no reduced-precision MFMA is usable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bohip {

// ---- tiling of every dense FP64 contraction --------------------------------------------------
// Workgroup tile 128 rows x 64 columns, 4 waves (2 x 2), wave tile 64 x 32 = 8 x 4 MFMA groups of 8 x 8.
// K is consumed in chunks of KC = 16 doubles (128 B = one cache line per row).  See gemm_core.h.
constexpr int TILE = 128;      // row-tile height and the block size of all blocked algorithms
constexpr int CTILE = 64;      // column-tile width of the contraction engine
constexpr int KC = 16;
constexpr int GEMM_THREADS = 256;

__host__ __device__ inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// kernel ids / acquisition ids mirror include/bohip.h
enum { KERN_SEARD = 0, KERN_SEISO = 1, KERN_MAT52ARD = 2, KERN_MAT32ARD = 3, KERN_MAT12ARD = 4, KERN_MAT52ISO = 5,
       KERN_MAT32ISO = 6, KERN_MAT12ISO = 7, KERN_COUNT = 8 };
enum { ACQ_EI = 0, ACQ_PI = 1, ACQ_UCB = 2, ACQ_MI = 3, ACQ_MAXMEAN = 4, ACQ_LOGEI = 6 };   // (5: BOHIP_ACQ_THOMPSON_DRAW, host only)
// the ids a scoring entry point takes: 0-4 and 6 (include/bohip_acq.h)
__host__ __device__ inline bool acq_id_scores(int id) { return (id >= ACQ_EI && id <= ACQ_MAXMEAN) || id == ACQ_LOGEI; }
// What the device kernels see of the kernel: its family.  An iso kernel differs from its ARD form only in il2, which the
// host fills with one length-scale.  FAM_M52 keeps the value 2 that the device compared the Mat52Ard id against.
enum { FAM_SE = 0, FAM_M12 = 1, FAM_M52 = 2, FAM_M32 = 3 };

constexpr int DMAX = 64;  // largest supported input dimension (hyper-parameters live in kernel args)

struct KernelHyper {
    int fam;           // FAM_*
    int d;
    double sigma2;     // exp(2 logsig)
    double il2[DMAX];  // exp(-2 loglen_k)
};

// Matérn 1/2 and 3/2 as functions of the squared scaled distance r = sum_k il2_k dx_k^2, rho = sqrt(r) (DESIGN.md "Matérn
// kernels").  The SE and Matérn 5/2 expressions stay written out at every site; these two helpers serve the two new families.
//   k:  M12 sigma2 exp(-rho)            M32 sigma2 (1 + sqrt3 rho) exp(-sqrt3 rho)
//   fx = 2 dk/dr, so that dk(x*, x_j)/dx*_k = fx dx_k il2_k and dk/dll_k = -fx dx_k^2 il2_k:
//       M12 -sigma2 exp(-rho) / rho, and 0 at rho = 0 (the minimum-norm subgradient of rho there)
//       M32 -3 sigma2 exp(-sqrt3 rho)
// Contraction is off inside them, so every site computes the same bits from the same r.
__device__ __forceinline__ double matern_lo_k(int fam, double sigma2, double r) {
#pragma clang fp contract(off)
    const bool m32 = fam == FAM_M32;
    const double s = (m32 ? sqrt(3.0) : 1.0) * sqrt(r);
    return sigma2 * (m32 ? 1.0 + s : 1.0) * exp(-s);
}
__device__ __forceinline__ double matern_lo_fx(int fam, double sigma2, double r) {
#pragma clang fp contract(off)
    const bool m32 = fam == FAM_M32;
    const double rho = sqrt(r), e = exp(-((m32 ? sqrt(3.0) : 1.0) * rho));
    if (m32) return -3.0 * sigma2 * e;
    return rho > 0.0 ? -(sigma2 * e) / rho : 0.0;
}

// bound of every in-kernel wait of the dataflow factorisation, in ticks of wall_clock64() (100 MHz): 200 ms (kernels_chol.hip)
constexpr unsigned long long CH_SPIN_TICKS_DEFAULT = 20000000ull;

// INLINE-ASM 16-BYTE STORES carry "s_nop 1" behind them.  gfx9 has a hazard: a VMEM store of more than 64 bits of data followed by
// a VALU instruction that writes one of the store's data VGPRs needs a wait state.  hipcc inserts it for stores it emitted
// itself, but its hazard recogniser does not look inside an inline-asm string, so `global_store_dwordx4 ... sc1` written as asm
// (the atomic builtins stop at 8 bytes) followed by ordinary code that reuses the data registers stored a corrupted low dword:
// measured in the inverter (kernels_chol.hip) as the first double of every other 16-byte piece off by ~1e-7 relative.

struct Best {
    double val;
    long long idx;
};

}  // namespace bohip
