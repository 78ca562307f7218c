// Stand-alone host check of csrc/devbuf.h and csrc/scratch_layout.h (tests/test_devbuf_host.py builds it with
// -fsanitize=address,undefined and runs it).  The buffer type is driven with malloc / free in place of the HIP calls; the
// layouts are walked on a made-up base address and never dereferenced.
#include "../../bayesianoptimization.jl_amd/csrc/scratch_layout.h"
#include "../../include/bohip_con.h"
#include "../../include/bohip_kg.h"
#include "../../include/bohip_mes.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

using devbuf::Grow;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

struct HostAlloc {
    using error_t = int;
    using stream_t = int*;   // counts the synchronisations
    static constexpr error_t ok = 0;
    static inline long allocs = 0, frees = 0, fail_at = -1;   // fail_at: the allocation (counted from 0) that fails
    static error_t alloc(void** p, size_t bytes, devbuf::Kind) {
        if (allocs++ == fail_at) return 2;
        *p = std::malloc(bytes ? bytes : 1);
        return *p ? ok : 2;
    }
    static error_t free(void* p, devbuf::Kind) { std::free(p); ++frees; return ok; }
    static error_t sync(stream_t s) { ++*s; return ok; }
};
template <class T>
using Dev = devbuf::Buf<T, devbuf::DEVICE, HostAlloc>;
template <class T>
using Pin = devbuf::Buf<T, devbuf::PINNED, HostAlloc>;

static int64_t live(int k) { return devbuf::g_live_bytes[k].load(); }

// the formulas the call sites used before the buffer type existed
static size_t old_exact(size_t need, size_t) { return need; }
static size_t old_half(size_t need, size_t old) { return std::max(need, old + old / 2); }
static size_t old_quarter(size_t need, size_t) { return need + need / 4; }

static void check_policy(Grow rule, size_t (*old_rule)(size_t, size_t)) {
    // rising, falling, rising again: a request within the capacity changes nothing, a larger one grows by the old formula
    const size_t seq[] = {100, 101, 400, 40, 1, 400, 401, 600, 599, 700, 2000, 8, 3001};
    Dev<double> b;
    int syncs = 0;
    size_t cap = 0;
    for (size_t n : seq) {
        double* before = b.get();
        const int syncs_before = syncs;
        const long allocs_before = HostAlloc::allocs;
        bool grew = false;
        REQUIRE(b.reserve(n, &syncs, rule, &grew) == 0);
        if (n > cap) {
            cap = old_rule(n, cap);
            REQUIRE(grew);
            REQUIRE(syncs == syncs_before + (before ? 1 : 0));   // waits for the stream only when there is an old block to free
        } else {
            REQUIRE(!grew && b.get() == before && syncs == syncs_before);
        }
        REQUIRE(grew == (HostAlloc::allocs != allocs_before));   // grew exactly when the block is a new one ...
        REQUIRE(grew || b.get() == before);                       // ... and the pointer changes at no other time
        REQUIRE(b.capacity() == cap && b.get() != nullptr);
        REQUIRE(live(devbuf::DEVICE) == (int64_t)(cap * sizeof(double)));
        b.get()[cap - 1] = 1.0;   // the whole capacity is there (ASan)
    }
    REQUIRE(b.release() == 0 && b.get() == nullptr && b.capacity() == 0 && live(devbuf::DEVICE) == 0);
}

static void check_floors() {   // the max(8 bytes, ...) floors of dX / dy / dXs: the callers ask for max(1, n) elements
    Dev<double> b;
    int s = 0;
    REQUIRE(b.reserve(std::max<size_t>(1, 0), &s) == 0 && b.capacity() * sizeof(double) == 8);
    Dev<double> none;
    bool grew = false;
    REQUIRE(none.reserve(0, &s, Grow::Exact, &grew) == 0 && !grew && none.get() == nullptr);   // nothing asked, nothing made
}

static void check_failure() {
    int s = 0;
    Dev<int> b;
    REQUIRE(b.reserve(10, &s) == 0);
    Pin<int> p;
    REQUIRE(p.reserve(7, &s) == 0);
    const int64_t dev0 = live(devbuf::DEVICE), pin0 = live(devbuf::PINNED);
    REQUIRE(dev0 == 40 && pin0 == 28);
    HostAlloc::fail_at = HostAlloc::allocs;   // the next allocation fails
    bool grew = false;
    REQUIRE(b.reserve(1000, &s, Grow::Half, &grew) != 0);
    REQUIRE(b.get() == nullptr && b.capacity() == 0 && !grew);   // never a dangling pointer with a stale capacity
    REQUIRE(live(devbuf::DEVICE) == dev0 - 40 && live(devbuf::PINNED) == pin0);
    Dev<int> fresh;
    HostAlloc::fail_at = HostAlloc::allocs;
    REQUIRE(fresh.reserve(5, &s) != 0 && fresh.get() == nullptr && fresh.capacity() == 0 && live(devbuf::DEVICE) == 0);
    HostAlloc::fail_at = -1;
    REQUIRE(b.reserve(1000, &s, Grow::Half, &grew) == 0 && grew && b.capacity() == 1000);   // a later reserve succeeds
    b.get()[999] = 1;
    REQUIRE(live(devbuf::DEVICE) == 4000);
}

static void check_moves() {
    int s = 0;
    const long a0 = HostAlloc::allocs - HostAlloc::frees;
    {
        Dev<double> a;
        REQUIRE(a.reserve(16, &s) == 0);
        double* p = a.get();
        Dev<double> b(std::move(a));
        REQUIRE(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 16);
        Dev<double> c;
        REQUIRE(c.reserve(4, &s) == 0);
        c = std::move(b);   // frees c's block, takes b's
        REQUIRE(b.get() == nullptr && c.get() == p && c.capacity() == 16 && live(devbuf::DEVICE) == 128);
        c = std::move(c);
        REQUIRE(c.get() == p);
        std::vector<Dev<double>> v;
        v.push_back(std::move(c));
        v.emplace_back();
        REQUIRE(v[1].reserve(3, &s) == 0 && live(devbuf::DEVICE) == 128 + 24);
    }
    REQUIRE(live(devbuf::DEVICE) == 0 && HostAlloc::allocs - HostAlloc::frees == a0);
}

// ---- the carved blocks -----------------------------------------------------------------------------------------------------------
struct Member { const char* name; const void* p; size_t bytes, align; };
static void check_block(const char* what, uintptr_t base, size_t total, std::vector<Member> ms) {
    size_t sum = 0;
    for (const Member& m : ms) {
        const uintptr_t a = (uintptr_t)m.p;
        if (!(a >= base && a + m.bytes <= base + total && (a - base) % m.align == 0)) {
            std::fprintf(stderr, "%s: member %s at offset %zu (%zu bytes, alignment %zu) of %zu\n", what, m.name, (size_t)(a - base), m.bytes,
                         m.align, total);
            std::exit(1);
        }
        sum += m.bytes;
    }
    REQUIRE(total >= sum);
    std::sort(ms.begin(), ms.end(), [](const Member& x, const Member& y) { return (uintptr_t)x.p < (uintptr_t)y.p; });
    for (size_t i = 0; i + 1 < ms.size(); ++i)
        if ((uintptr_t)ms[i].p + ms[i].bytes > (uintptr_t)ms[i + 1].p) {
            std::fprintf(stderr, "%s: members %s and %s overlap\n", what, ms[i].name, ms[i + 1].name);
            std::exit(1);
        }
}
#define M(s, f, n, al) Member{#f, (s).f, (size_t)(n) * sizeof(*(s).f), (size_t)(al)}

struct Best { double val; long long idx; };
static void* const BASE = (void*)(uintptr_t)0x100000;   // as aligned as the allocators make a block (256 bytes and more)
static const uintptr_t B0 = (uintptr_t)BASE;

// the documented limits (include/bohip_kg.h, bohip_mes.h, bohip_con.h) and the kernels' constants as the call sites pass them
static const size_t KG_RMAX = BOHIP_KG_RMAX, MES_KMAX = BOHIP_MES_KMAX, MES_RMAX = BOHIP_MES_RMAX, CON_CMAX = BOHIP_CON_CMAX;
static const size_t CON_GRID_MAX = 1024, MES_STATE = 8, MES_BR_MAX = 256, MES_SUMS = 3 * 15, MES_SLICE = 8192, ASC_M = 8, ASC_RING = 8,
                    BATCH_WG_MAX = 512, QEI_B = 32, QEI_PICK = 256;

static void check_qei() {
    struct W { double *m, *part; Best* tile; double* gain; long long* idx; unsigned *done, *arrive; };
    const size_t cases[][3] = {{1, 1, 1}, {3, 5, 3}, {64, 64, 64}, {4097, 33, 4097}};   // (R, S, q), q = R among them
    for (auto& c : cases) {
        const size_t R = c[0], S = c[1], q = c[2], NB = (S + QEI_B - 1) / QEI_B, NT = (R + QEI_PICK - 1) / QEI_PICK;
        W w, w0;
        const size_t total = layout::qei(BASE, S, NB * R, NT, q, &w);
        REQUIRE(layout::qei(nullptr, S, NB * R, NT, q, &w0) == total);   // the sizing walk and the real one agree
        REQUIRE(w.arrive == w.done + 1);
        check_block("qei", B0, total,
                    {M(w, m, S, 8), M(w, part, NB * R, 8), M(w, tile, NT, 16), M(w, gain, q, 8), M(w, idx, q, 8), M(w, done, 2, 4)});
    }
}
static void check_kg() {
    struct W { double* kg; Best* best; int* nseg; double *a, *B; };
    for (size_t R : {(size_t)1, (size_t)3, (size_t)64, KG_RMAX})
        for (size_t E : {(size_t)1, R})
            for (int lines = 0; lines < 2; ++lines) {
                W w;
                const size_t nl = lines ? R : 0, total = layout::kg(BASE, E, nl, &w);
                check_block("kg", B0, total, {M(w, kg, E, 8), M(w, best, 1, 16), M(w, nseg, E, 4), M(w, a, nl, 16), M(w, B, E * nl, 16)});
            }
}
static void check_mes() {
    struct Ws { double *st, *br, *part; int nsl; };
    struct Bufs { double *mes, *dmu, *dvar, *maxvals, *quant, *mu, *var; Best *blocks, *best; Ws w; };
    const size_t cases[][2] = {{1, 1}, {257, 3}, {4096, 16}, {MES_RMAX, MES_KMAX}};
    for (auto& c : cases) {
        const size_t R = c[0], K = c[1], nsl = (R + MES_SLICE - 1) / MES_SLICE, nb = (R + 255) / 256;
        Bufs b;
        const size_t total = layout::mes(BASE, R, K, 2 * MES_STATE + 4, 3 * MES_BR_MAX, 2 * MES_SUMS * nsl, nb, &b);
        REQUIRE(b.dmu == b.mes + R && b.dvar == b.mes + 2 * R && b.mu == b.mes + 3 * R && b.var == b.mes + 4 * R && b.best == b.blocks + nb);
        check_block("mes", B0, total,
                    {M(b, mes, 5 * R, 8), M(b, maxvals, K, 8), M(b, quant, 4, 8), M(b.w, st, 2 * MES_STATE + 4, 8), M(b.w, br, 3 * MES_BR_MAX, 8),
                     M(b.w, part, 2 * MES_SUMS * nsl, 8), M(b, blocks, nb + 1, 16)});
    }
}
static void check_con() {
    struct Bufs { double *mu, *var, *pmu, *pvar, *value, *logfeas, *jmu, *jvar, *grad; Best *blocks, *best; };
    for (size_t C : {(size_t)0, (size_t)1, (size_t)3, CON_CMAX})
        for (size_t R : {(size_t)1, (size_t)37, (size_t)4096})
            for (size_t d : {(size_t)0, (size_t)1, (size_t)3, (size_t)64}) {
                Bufs b;
                const size_t m = (C + 1) * R, total = layout::con(BASE, m, R, CON_GRID_MAX, d, &b);
                REQUIRE(b.best == b.blocks + CON_GRID_MAX);
                std::vector<Member> ms = {M(b, mu, m, 8),    M(b, var, m, 8),     M(b, pmu, m, 8),   M(b, pvar, m, 8),
                                          M(b, value, R, 8), M(b, logfeas, R, 8), M(b, blocks, CON_GRID_MAX + 1, 16)};
                if (d) {
                    ms.push_back(M(b, jmu, m * d, 8)); ms.push_back(M(b, jvar, m * d, 8)); ms.push_back(M(b, grad, R * d, 8));
                } else {
                    REQUIRE(!b.jmu && !b.jvar && !b.grad);
                }
                check_block("con", B0, total, ms);
            }
}
static void check_batch() {
    struct Rec { double a, b, c; long long i; int k; };
    struct Scal { double v[5]; };
    struct W { double* U; Rec* rec; Scal* scal; Best* wg_best; int* picked; };
    const size_t cases[][2] = {{1, 256}, {3, 384}, {384, 384}};   // (q, rows), q = R among them
    for (auto& c : cases) {
        W w;
        const size_t total = layout::batch(BASE, c[0], c[1], BATCH_WG_MAX, &w);
        check_block("batch", B0, total,
                    {M(w, U, c[0] * c[1], 8), M(w, rec, c[0], alignof(Rec)), M(w, scal, 1, alignof(Scal)), M(w, wg_best, BATCH_WG_MAX, 16), M(w, picked, c[1], 4)});
    }
}
static void check_ascent() {
    struct A {
        double *X, *G, *Xt, *Gt, *Xn, *Gn, *D, *Gp, *best_X, *S, *Y, *f, *ft, *fn, *step, *best_f;
        int *active, *accepted, *it, *bt, *h_accepted, *h_active, *h_cnt;
        unsigned *nact, *ticket;
    };
    for (size_t cap : {(size_t)32, (size_t)33, (size_t)4096})
        for (size_t d : {(size_t)1, (size_t)3, (size_t)64}) {
            A a;
            const size_t rd = cap * d, Mm = ASC_M, ring = ASC_RING;
            size_t total = layout::ascent_doubles(BASE, cap, d, Mm, &a);
            REQUIRE(total == ((9 + 2 * Mm) * rd + 5 * cap) * 8);   // the bytes the block always had
            check_block("ascent doubles", B0, total,
                        {M(a, X, rd, 8), M(a, G, rd, 8), M(a, Xt, rd, 8), M(a, Gt, rd, 8), M(a, Xn, rd, 8), M(a, Gn, rd, 8), M(a, D, rd, 8),
                         M(a, Gp, rd, 8), M(a, best_X, rd, 8), M(a, S, Mm * rd, 8), M(a, Y, Mm * rd, 8), M(a, f, cap, 8), M(a, ft, cap, 8),
                         M(a, fn, cap, 8), M(a, step, cap, 8), M(a, best_f, cap, 8)});
            total = layout::ascent_words(BASE, cap, ring, &a);
            REQUIRE(total == (4 * cap + 2 * ring + 2) * 4);
            check_block("ascent words", B0, total,
                        {M(a, active, cap, 4), M(a, accepted, cap, 4), M(a, it, cap, 4), M(a, bt, cap, 4), M(a, nact, 2 * ring, 4), M(a, ticket, 2, 4)});
            total = layout::ascent_pinned(BASE, cap, ring, &a);
            REQUIRE(total == (2 * cap + ring) * 4);
            check_block("ascent pinned", B0, total, {M(a, h_accepted, cap, 4), M(a, h_active, cap, 4), M(a, h_cnt, ring, 4)});
        }
}
static void check_small() {
    const size_t cases[][4] = {{1, 1, 1, 2}, {1, 3, 2, 4}, {16, 79, 79, 64}};   // (npass, T, ntiles, DT): up to 256 candidates
    for (auto& c : cases) {
        const size_t np = c[0], T = c[1], nt = c[2], DT = c[3];
        const size_t n_part = np * nt * 2048, n_v16 = np * T * 128 * 16, n_rec = np * T * 16, n_g = np * nt * 16 * DT, n_gm = np * T * 16 * DT;
        layout::SmallWs w;
        const size_t total = layout::small(BASE, n_part, n_v16, n_rec, np * 32, 256, n_g, n_gm, &w);
        REQUIRE(total == (n_part + 2 * n_v16 + 2 * n_rec + np * 32 + 256 + n_g + n_gm) * 8);   // the bytes the block always had
        check_block("small", B0, total,
                    {M(w, part, n_part, 8), M(w, v16, n_v16, 8), M(w, qpart, n_rec, 8), M(w, mupart, n_rec, 8), M(w, post, np * 32, 8),
                     M(w, fstash, 256, 8), M(w, ks16, n_v16, 8), M(w, gpart, n_g, 8), M(w, gmpart, n_gm, 8)});
    }
}
static void check_pruned() {
    const size_t cases[][4] = {{256, 144, 1, 8}, {384, 272, 3, 23}, {65664, 10128, 79, 403}};   // (Rpad, ld, T, table words)
    for (auto& c : cases) {
        const size_t Rpad = c[0], ld = c[1], T = c[2], P = T * 2;
        layout::PrunedWs w;
        const size_t total = layout::pruned(BASE, Rpad * ld, 2 * T * Rpad, Rpad, 64, 2 * P * Rpad, c[3], &w);
        REQUIRE(total % 256 == 0);
        check_block("pruned", B0, total,
                    {M(w, ks, Rpad * ld, 256), M(w, q2, 2 * T * Rpad, 256), M(w, mu2, Rpad, 256), M(w, ub, Rpad, 256), M(w, l1, 64, 256),
                     M(w, l2, Rpad, 256), M(w, mark, Rpad, 256), M(w, cnt, 64, 256), Member{"rec", w.rec, 256, 256}, M(w, parts, 2 * P * Rpad, 256),
                     M(w, pcs, c[3], 256)});
    }
}
static void check_pinned_small() {
    for (size_t ns : {(size_t)1, (size_t)32})
        for (size_t dmax : {(size_t)1, (size_t)64}) {
            layout::PinnedSmall w;
            const size_t total = layout::pinned_small(BASE, ns, dmax, &w);
            REQUIRE(total == (3 * ns + 2 + 2 * ns * dmax) * 8);   // the doubles the block always had ...
            // ... at the offsets the call sites used to spell out
            const double* b = (const double*)BASE;
            REQUIRE(w.score == b && w.mu == b + ns && w.var == b + 2 * ns && w.rec == b + 3 * ns && w.grad == b + 3 * ns + 2 &&
                    w.cand == b + 3 * ns + 2 + ns * dmax && (const void*)w.words == (const void*)w.rec);
            check_block("pinned_small", B0, total,
                        {M(w, score, ns, 8), M(w, mu, ns, 8), M(w, var, ns, 8), M(w, rec, 2, 8), M(w, grad, ns * dmax, 8), M(w, cand, ns * dmax, 8)});
        }
    // the deliberate aliases fit at the shipped sizes (common.h: SMALL_R = 32 candidates, DMAX = 64 coordinates): an arg-max record and
    // the refit's two words in the record area, mll_grad's DMAX + 4 doubles and the append's SMALL_R x DMAX in the gradient area
    const size_t SMALL_R = 32, DMAX = 64;
    layout::PinnedSmall w;
    layout::pinned_small(BASE, SMALL_R, DMAX, &w);
    const size_t rec_bytes = (size_t)((const char*)w.grad - (const char*)w.rec), grad_bytes = (size_t)((const char*)w.cand - (const char*)w.grad);
    REQUIRE(sizeof(Best) <= rec_bytes && 2 * sizeof(int) <= rec_bytes && (DMAX + 4) * 8 <= grad_bytes && SMALL_R * DMAX * 8 <= grad_bytes);
}
static void check_fit_and_ens() {
    for (size_t H : {(size_t)1, (size_t)5, (size_t)65535}) {
        layout::FitIo f;
        const size_t P = 6, total = layout::fit_io(BASE, H, P, 6, &f);
        REQUIRE(total == H * (2 * P + 2) * 8 + 6 * 8);   // the bytes the block always had
        check_block("fit_io", B0, total, {M(f, theta, H * P, 8), M(f, mll, H, 8), M(f, grad, H * P, 8), M(f, pivot, H, 8), M(f, stamps, 6, 8)});
    }
    for (size_t H : {(size_t)1, (size_t)2, (size_t)6})
        for (size_t dg : {(size_t)0, (size_t)3}) {
            const size_t P = 6, Rc = 64, d = 3, R = 101, nblk = 2;
            layout::EnsIo<Best> e;
            const size_t total = layout::ens_io(BASE, H, P, Rc, d, R, nblk, dg, &e);
            REQUIRE(e.best == e.blk + nblk);
            std::vector<Member> ms = {M(e, theta, H * P, 8), M(e, w, H, 8),        M(e, wt, H, 8),       M(e, pivot, H, 8), M(e, xs, Rc * d, 8),
                                      M(e, each, H * Rc, 8), M(e, mu, H * Rc, 8), M(e, var, H * Rc, 8), M(e, scores, R, 8), M(e, blk, nblk + 1, 16)};
            if (dg) {
                ms.push_back(M(e, geach, H * Rc * dg, 8)); ms.push_back(M(e, grad, R * dg, 8));
            } else {
                REQUIRE(!e.geach && !e.grad);
            }
            check_block("ens_io", B0, total, ms);
        }
}

int main() {
    check_policy(Grow::Exact, old_exact);
    check_policy(Grow::Half, old_half);
    check_policy(Grow::Quarter, old_quarter);
    check_floors();
    check_failure();
    check_moves();
    check_qei();
    check_kg();
    check_mes();
    check_con();
    check_batch();
    check_ascent();
    check_small();
    check_pruned();
    check_pinned_small();
    check_fit_and_ens();
    REQUIRE(live(devbuf::DEVICE) == 0 && live(devbuf::PINNED) == 0);   // nothing is left behind
    std::puts("devbuf_check ok");
    return 0;
}
