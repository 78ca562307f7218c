// kernels_kg.hip -- the knowledge gradient over a candidate set, exact (include/bohip_kg.h):
//     KG(e) = E_Z[max_j (a_j + b_j Z)] - max_j a_j,   b_j = Sigma_je / sqrt(Sigma_ee + nu),
// by a march along the upper envelope of the R lines of evaluation point e: from the line of smallest slope, the next line of the
// envelope is the one the current line meets first, z_i = (a_c - a_i) / (b_i - b_c) smallest over the steeper lines, and every
// segment adds (b_t - b_c) h(-|z_t|) >= 0.
//   k_kg       one workgroup (4 waves) per evaluation point.  a and the point's b sit in LDS (16 R bytes: R <= KG_RMAX = 8192 is
//              128 KiB of the CU's 160), read once from the covariance row -- Sigma is exactly symmetric, so column e is the
//              contiguous row e -- with 16-byte loads, b divided by sqrt(Sigma_ee + nu) on the way in.  A line that takes no part
//              (a or b not finite) gets b = NaN, which fails every comparison of the march.  A step: the lanes stride over the
//              lines -- subtract, divide, compare -- the record (z, b, a, index) is reduced across the wave with shuffles and
//              across the four waves through two alternating LDS slots, so a step costs ONE barrier; wave 0 adds the term.
//              The order of the record is total (the index ends every tie), so the winner does not depend on who compares first.
//   k_kg_best  the arg-max record over the E values (`better` of kernels_score.hip: strict '>', NaN never wins)
// No atomics, no communication between workgroups.  Contraction is off: z and the products of a term are those of the NumPy twin
// (tests/kg_reference.py) bit for bit; exp and erfc are the device's.
#include "common.h"   // (`better`, block_argmax come from kernels_score.hip, included before; the forms of h from acq_log.h)

namespace bohip {

constexpr int KG_THREADS = 256;
constexpr int KG_RMAX = 8192;                               // BOHIP_KG_RMAX
constexpr int KG_SLOT_BYTES = 2 * (KG_THREADS / 64) * 32;   // two alternating sets of one 32-byte record per wave
constexpr size_t kg_lds_bytes(int64_t R) { return (size_t)((R + 1) & ~(int64_t)1) * 16 + KG_SLOT_BYTES; }

struct KgRec {   // 32 bytes
    double z, b, a;
    int i, pad;
};

// does record (z, b, a, i) come before (oz, ob, oa, oi)?  z ascending, then b descending, a descending, index ascending; i < 0: none
__device__ __forceinline__ bool kg_before(double z, double b, double a, int i, double oz, double ob, double oa, int oi) {
    if (i < 0) return false;
    if (oi < 0) return true;
    if (z != oz) return z < oz;
    if (b != ob) return b > ob;
    if (a != oa) return a > oa;
    return i < oi;
}

// the workgroup's first record under kg_before, in every thread.  `slots`: the set of this step (the caller alternates them: a wave
// that runs ahead writes the other set, and cannot reach this one again before everybody has passed the next step's barrier)
__device__ __forceinline__ void kg_reduce(double& z, double& b, double& a, int& i, KgRec* slots) {
    for (int o = 32; o > 0; o >>= 1) {
        const double oz = __shfl_xor(z, o), ob = __shfl_xor(b, o), oa = __shfl_xor(a, o);
        const int oi = __shfl_xor(i, o);
        if (kg_before(oz, ob, oa, oi, z, b, a, i)) { z = oz; b = ob; a = oa; i = oi; }
    }
    if ((threadIdx.x & 63) == 0) {
        KgRec r;
        r.z = z; r.b = b; r.a = a; r.i = i; r.pad = 0;
        slots[threadIdx.x >> 6] = r;
    }
    __syncthreads();
    i = -1;
#pragma unroll
    for (int w = 0; w < KG_THREADS / 64; ++w) {
        const KgRec r = slots[w];
        if (kg_before(r.z, r.b, r.a, r.i, z, b, a, i)) { z = r.z; b = r.b; a = r.a; i = r.i; }
    }
}

// T(db, x) = db h(x), h(x) = phi(x) + x Phi(x), x <= 0 (include/bohip_kg.h).  Not inlined, as the bodies of acq_log.h: erfc, exp and
// the division loop stay out of the march's registers.
__device__ __noinline__ double kg_term(double db, double x) {
#pragma clang fp contract(off)
    if (x > LOGEI_SWITCH) {
        const double phi = 0.3989422804014327 * exp(-0.5 * (x * x));
        const double Phi = 0.5 * erfc(-x / 1.4142135623730951);
        return db * (phi + x * Phi);
    }
    const double t = -x;
    double r = 0.0;
#pragma unroll 1
    for (int k = LOGEI_CF_DEPTH; k >= 2; --k) r = (double)k / (t + r);
    const double c1 = 1.0 / (t + r), tc = t + c1;
    const double e = exp(-0.25 * (x * x));
    return (db * e) * ((0.3989422804014327 * e) * (c1 / tc));
}

// SCALE: B is the posterior covariance and row e becomes b_j = B[e][j] / sqrt(B[e][e] + nu); otherwise row e holds the slopes
template <bool SCALE>
__global__ __launch_bounds__(KG_THREADS) void k_kg(const double* __restrict__ a, const double* __restrict__ B, int64_t ldb, int R,
                                                   double nu, double* __restrict__ kg, int* __restrict__ nseg) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char kg_smem[];
    const int Rp = (R + 1) & ~1;
    double* sa = reinterpret_cast<double*>(kg_smem);
    double* sb = sa + Rp;
    KgRec* slots = reinterpret_cast<KgRec*>(sb + Rp);
    const int e = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ row = B + (int64_t)e * ldb;
    double s = 1.0;
    if (SCALE) {
        const double dd = row[e] + nu;
        if (!(dd > 0.0) || !(dd < INFINITY)) {   // (the same in every thread: nobody is left at a barrier)
            if (tid == 0) { kg[e] = 0.0; nseg[e] = 0; }
            return;
        }
        s = sqrt(dd);
    }
    auto line = [&](double aj, double bj) {
        if (SCALE) bj = bj / s;
        return (fabs(aj) < INFINITY && fabs(bj) < INFINITY) ? bj : NAN;
    };
    if ((((uintptr_t)row | (uintptr_t)a) & 15) == 0) {
        for (int j = 2 * tid; j + 1 < R; j += 2 * KG_THREADS) {
            const double2 av = *reinterpret_cast<const double2*>(a + j), bv = *reinterpret_cast<const double2*>(row + j);
            *reinterpret_cast<double2*>(sa + j) = av;
            *reinterpret_cast<double2*>(sb + j) = make_double2(line(av.x, bv.x), line(av.y, bv.y));
        }
        if ((R & 1) && tid == 0) { sa[R - 1] = a[R - 1]; sb[R - 1] = line(a[R - 1], row[R - 1]); }
    } else {
        for (int j = tid; j < R; j += KG_THREADS) { sa[j] = a[j]; sb[j] = line(a[j], row[j]); }
    }
    __syncthreads();
    // the start: smallest b, then largest a, then smallest index (kg_before on (b, a, 0))
    double kz = 0.0, kb = 0.0, ka = 0.0;
    int ki = -1;
    for (int j = tid; j < R; j += KG_THREADS) {
        const double bj = sb[j];
        if (bj == bj) {
            const double aj = sa[j];
            if (kg_before(bj, aj, 0.0, j, kz, kb, ka, ki)) { kz = bj; kb = aj; ki = j; }
        }
    }
    kg_reduce(kz, kb, ka, ki, slots);
    double acc = 0.0;
    int n = 0;
    if (ki >= 0) {
        double bc = kz, ac = kb;
        for (int step = 1;; ++step) {
            ki = -1;
            for (int j = tid; j < R; j += KG_THREADS) {
                const double bj = sb[j];
                if (bj > bc) {
                    const double aj = sa[j];
                    const double z = (ac - aj) / (bj - bc);
                    if (z == z && kg_before(z, bj, aj, j, kz, kb, ka, ki)) { kz = z; kb = bj; ka = aj; ki = j; }
                }
            }
            kg_reduce(kz, kb, ka, ki, slots + (step & 1) * (KG_THREADS / 64));
            if (ki < 0) break;
            if (tid < 64) acc += kg_term(kb - bc, -fabs(kz));
            ++n;
            bc = kb;
            ac = ka;
        }
    }
    if (tid == 0) { kg[e] = acc; nseg[e] = n; }
}

__global__ __launch_bounds__(256) void k_kg_best(const double* __restrict__ kg, int E, Best* __restrict__ out) {
    __shared__ Best sh[4];
    double v = -INFINITY;
    long long idx = -1;
    for (int i = threadIdx.x; i < E; i += 256)
        if (better(kg[i], i, v, idx)) { v = kg[i]; idx = i; }
    block_argmax(v, idx, sh);
    if (threadIdx.x == 0) { out->val = idx >= 0 ? v : -INFINITY; out->idx = idx; }
}

}  // namespace bohip
