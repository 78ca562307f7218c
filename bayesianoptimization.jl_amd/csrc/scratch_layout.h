// scratch_layout.h -- the layout of every scratch block that holds more than one array: ONE function per block, which takes the
// members from a devbuf::Carve, fills the caller's struct of pointers and returns the bytes the block needs.  Called on a null
// base to size the block and on the block to get the pointers.  The functions take element counts and are templates over the
// struct they fill, so they depend on no kernel header (tests/host/devbuf_check.cpp checks overlap and alignment on the host).
// Arg-max records are placed at 16 bytes; k_kg's a / B (16-byte loads) too; the pruned pass keeps every part 256-aligned.
#pragma once
#include "devbuf.h"
#include <type_traits>

namespace layout {
using devbuf::Carve;
template <class P>
using elem_t = std::remove_pointer_t<P>;
static constexpr size_t REC_ALIGN = 16;

// greedy q-EI: [m S | partials NB x R | records NT | gain q | idx q | done, arrive]
template <class W>
size_t qei(const void* base, size_t S, size_t part, size_t NT, size_t q, W* w) {
    Carve c(base);
    w->m = c.take<double>(S);
    w->part = c.take<double>(part);
    w->tile = c.take<elem_t<decltype(w->tile)>>(NT, REC_ALIGN);
    w->gain = c.take<double>(q);
    w->idx = c.take<long long>(q);
    w->done = c.take<unsigned>(4);
    w->arrive = w->done + 1;
    return c.total();
}
// knowledge gradient: [kg E | record | nseg E | a R | B E x R], the last two (nline = R or 0) for the caller's lines only
template <class W>
size_t kg(const void* base, size_t E, size_t nline, W* w) {
    Carve c(base);
    w->kg = c.take<double>(E);
    w->best = c.take<elem_t<decltype(w->best)>>(1, REC_ALIGN);
    w->nseg = c.take<int>(E);
    w->a = c.take<double>(nline, 16);
    w->B = c.take<double>(E * nline, 16);
    return c.total();
}
// max-value entropy search: [mes | dmu | dvar | mu | var (R each, one array: bohip_gp_mes strides across them) | maxvals K |
// quantiles 3 (+1) | state | bracket partials | probe sums | records nb + 1]
template <class B>
size_t mes(const void* base, size_t R, size_t K, size_t n_state, size_t n_br, size_t n_part, size_t nb, B* b) {
    Carve c(base);
    double* d = c.take<double>(5 * R);
    b->mes = d; b->dmu = d + R; b->dvar = d + 2 * R; b->mu = d + 3 * R; b->var = d + 4 * R;
    b->maxvals = c.take<double>(K);
    b->quant = c.take<double>(4);
    b->w.st = c.take<double>(n_state);
    b->w.br = c.take<double>(n_br);
    b->w.part = c.take<double>(n_part);
    b->blocks = c.take<elem_t<decltype(b->blocks)>>(nb + 1, REC_ALIGN);
    b->best = b->blocks + nb;
    return c.total();
}
// constrained scoring: [mu | var | pmu | pvar (m each) | value | logfeas (R each) | records nrec + 1 | jmu | jvar (m d) | grad (R d)],
// the Jacobians for the gradient route only (d = 0: null)
template <class B>
size_t con(const void* base, size_t m, size_t R, size_t nrec, size_t d, B* b) {
    Carve c(base);
    b->mu = c.take<double>(m); b->var = c.take<double>(m); b->pmu = c.take<double>(m); b->pvar = c.take<double>(m);
    b->value = c.take<double>(R); b->logfeas = c.take<double>(R);
    b->blocks = c.take<elem_t<decltype(b->blocks)>>(nrec + 1, REC_ALIGN);
    b->best = b->blocks + nrec;
    b->jmu = d ? c.take<double>(m * d) : nullptr;
    b->jvar = d ? c.take<double>(m * d) : nullptr;
    b->grad = d ? c.take<double>(R * d) : nullptr;
    return c.total();
}
// batch selection: [u_i q x rows | records q | scalars | workgroup records | picked rows]
template <class W>
size_t batch(const void* base, size_t q, size_t rows, size_t nwg, W* w) {
    Carve c(base);
    w->U = c.take<double>(q * rows);
    w->rec = c.take<elem_t<decltype(w->rec)>>(q);
    w->scal = c.take<elem_t<decltype(w->scal)>>(1);
    w->wg_best = c.take<elem_t<decltype(w->wg_best)>>(nwg, REC_ALIGN);
    w->picked = c.take<int>(rows);
    return c.total();
}
// the ascent's state: three blocks (doubles, device words, pinned words) for `cap` starts of d coordinates, memory pairs M, ring
template <class A>
size_t ascent_doubles(const void* base, size_t cap, size_t d, size_t M, A* a) {
    Carve c(base);
    const size_t rd = cap * d;
    a->X = c.take<double>(rd); a->G = c.take<double>(rd); a->Xt = c.take<double>(rd); a->Gt = c.take<double>(rd);
    a->Xn = c.take<double>(rd); a->Gn = c.take<double>(rd); a->D = c.take<double>(rd); a->Gp = c.take<double>(rd);
    a->best_X = c.take<double>(rd);
    a->S = c.take<double>(M * rd); a->Y = c.take<double>(M * rd);
    a->f = c.take<double>(cap); a->ft = c.take<double>(cap); a->fn = c.take<double>(cap); a->step = c.take<double>(cap);
    a->best_f = c.take<double>(cap);
    return c.total();
}
template <class A>
size_t ascent_words(const void* base, size_t cap, size_t ring, A* a) {
    Carve c(base);
    a->active = c.take<int>(cap); a->accepted = c.take<int>(cap); a->it = c.take<int>(cap); a->bt = c.take<int>(cap);
    a->nact = c.take<unsigned>(2 * ring); a->ticket = c.take<unsigned>(2);
    return c.total();
}
template <class A>
size_t ascent_pinned(const void* base, size_t cap, size_t ring, A* a) {
    Carve c(base);
    a->h_accepted = c.take<int>(cap); a->h_active = c.take<int>(cap); a->h_cnt = c.take<int>(ring);
    return c.total();
}
// the small-batch pass: [part | v16 | qpart | mupart | post npass x 32 | fstash | ks16 | gpart | gmpart]
struct SmallWs { double *part, *v16, *qpart, *mupart, *post, *fstash, *ks16, *gpart, *gmpart; };
inline size_t small(const void* base, size_t n_part, size_t n_v16, size_t n_rec, size_t n_post, size_t n_stash, size_t n_g, size_t n_gm,
                    SmallWs* w) {
    Carve c(base);
    w->part = c.take<double>(n_part); w->v16 = c.take<double>(n_v16); w->qpart = c.take<double>(n_rec); w->mupart = c.take<double>(n_rec);
    w->post = c.take<double>(n_post); w->fstash = c.take<double>(n_stash); w->ks16 = c.take<double>(n_v16);
    w->gpart = c.take<double>(n_g); w->gmpart = c.take<double>(n_gm);
    return c.total();
}
// the pruned arg-max: [packed K*' rows | q2 | mu2 | bounds | list 1 | list 2 | marks | counters | record | k_kstar's partials | pieces],
// every part 256-aligned
struct PrunedWs {
    double *ks, *q2, *mu2, *ub, *parts;
    int *l1, *l2, *mark, *pcs;
    unsigned* cnt;
    void* rec;
};
inline size_t pruned(const void* base, size_t n_ks, size_t n_q2, size_t Rpad, size_t k1, size_t n_parts, size_t n_pcs, PrunedWs* w) {
    Carve c(base);
    const size_t A = 256;
    w->ks = c.take<double>(n_ks, A); w->q2 = c.take<double>(n_q2, A); w->mu2 = c.take<double>(Rpad, A); w->ub = c.take<double>(Rpad, A);
    w->l1 = c.take<int>(k1, A); w->l2 = c.take<int>(Rpad, A); w->mark = c.take<int>(Rpad, A);
    w->cnt = c.take<unsigned>(64, A); w->rec = c.take<char>(256, A);
    w->parts = c.take<double>(n_parts, A); w->pcs = c.take<int>(n_pcs, A);
    c.take<char>(0, A);   // (the block ends on a 256-byte boundary, as its parts do)
    return c.total();
}
// batched marginal likelihood: [theta H x P | mll H | grad H x P | pivot H | stamps]
struct FitIo { double *theta, *mll, *grad; long long* pivot; unsigned long long* stamps; };
inline size_t fit_io(const void* base, size_t H, size_t P, size_t n_stamps, FitIo* w) {
    Carve c(base);
    w->theta = c.take<double>(H * P); w->mll = c.take<double>(H); w->grad = c.take<double>(H * P);
    w->pivot = c.take<long long>(H); w->stamps = c.take<unsigned long long>(n_stamps);
    return c.total();
}
// batched leave-one-out: the per-point log-probabilities of every setting, [logp H x N]
struct LooBatchIo { double* logp; };
inline size_t loo_batch_io(const void* base, size_t H, size_t N, LooBatchIo* w) {
    Carve c(base);
    w->logp = c.take<double>(H * N);
    return c.total();
}
// marginalised acquisition: [theta | w | w~ | pivot | xs chunk | each, mu, var H x Rc | d each / d x (H x Rc x d) | scores R |
// gradient R x d | workgroup records nblk + 1], the two gradient members with dg = d only (dg = 0: null)
template <class Rec>
struct EnsIo { double *theta, *w, *wt, *xs, *each, *mu, *var, *geach, *scores, *grad; long long* pivot; Rec *blk, *best; };
template <class Rec>
size_t ens_io(const void* base, size_t H, size_t P, size_t Rc, size_t d, size_t R, size_t nblk, size_t dg, EnsIo<Rec>* w) {
    Carve c(base);
    w->theta = c.take<double>(H * P); w->w = c.take<double>(H); w->wt = c.take<double>(H); w->pivot = c.take<long long>(H);
    w->xs = c.take<double>(Rc * d);
    w->each = c.take<double>(H * Rc); w->mu = c.take<double>(H * Rc); w->var = c.take<double>(H * Rc);
    w->geach = dg ? c.take<double>(H * Rc * dg) : nullptr;
    w->scores = c.take<double>(R);
    w->grad = dg ? c.take<double>(R * dg) : nullptr;
    w->blk = c.take<Rec>(nblk + 1, REC_ALIGN);
    w->best = w->blk + nblk;
    return c.total();
}
// leave-one-out: [total | gradient slots (n_out) | kappa | mu | var | logp | q | sqrt c | t = W q | b = W't], the vectors nv each
// and 16-byte aligned (nv covers the 256-wide chunks k_trimv_stream reads its right-hand sides in)
struct LooWs { double *out, *kappa, *mu, *var, *logp, *q, *sc, *t, *b; };
inline size_t loo(const void* base, size_t n_out, size_t nv, LooWs* w) {
    Carve c(base);
    w->out = c.take<double>(n_out);
    w->kappa = c.take<double>(nv, 16); w->mu = c.take<double>(nv, 16); w->var = c.take<double>(nv, 16); w->logp = c.take<double>(nv, 16);
    w->q = c.take<double>(nv, 16); w->sc = c.take<double>(nv, 16); w->t = c.take<double>(nv, 16); w->b = c.take<double>(nv, 16);
    return c.total();
}
// pending evaluations, the state derived from (model, pending set): [Xp pmax x d | mu_p | Sigma_p | L_p (pmax x pmax each) |
// G = V_p'V_p, one MFMA tile | pivot word]
struct PendState { double *Xp, *mu, *Sigma, *L, *G; int* info; };
inline size_t pend_state(const void* base, size_t pmax, size_t d, size_t n_tile, PendState* w) {
    Carve c(base);
    w->Xp = c.take<double>(pmax * d, 16);
    w->mu = c.take<double>(pmax); w->Sigma = c.take<double>(pmax * pmax); w->L = c.take<double>(pmax * pmax);
    w->G = c.take<double>(n_tile, 16);
    w->info = c.take<int>(4);
    return c.total();
}
// pending evaluations, one call: [C = V'V_p of a chunk, 64 columns a row | B R x p | Z S x p | tau S | mu, var, score (R each: the
// host-array stage only, n_io = R or 0) | workgroup records nb + 1]
template <class Rec>
struct PendCall { double *C, *B, *Z, *tau, *mu, *var, *score; Rec *blk, *best; };
template <class Rec>
size_t pend_call(const void* base, size_t n_c, size_t R, size_t p, size_t S, size_t n_io, size_t nb, PendCall<Rec>* w) {
    Carve c(base);
    w->C = c.take<double>(n_c, 16);
    w->B = c.take<double>(R * p); w->Z = c.take<double>(S * p); w->tau = c.take<double>(S);
    w->mu = c.take<double>(n_io); w->var = c.take<double>(n_io); w->score = c.take<double>(n_io);
    w->blk = c.take<Rec>(nb + 1, REC_ALIGN);
    w->best = w->blk + nb;
    return c.total();
}
// noisy expected improvement, the fantasies derived from (model, companion, S, seed): [F | alpha | four work matrices (rows x ld each,
// 128-byte rows for the LDS-DMA of the products) | tau S1]
struct NeiState { double *F, *alpha, *w0, *w1, *w2, *w3, *tau; };
inline size_t nei_state(const void* base, size_t rows, size_t ld, size_t S1, NeiState* w) {
    Carve c(base);
    w->F = c.take<double>(rows * ld, 128); w->alpha = c.take<double>(rows * ld, 128);
    w->w0 = c.take<double>(rows * ld, 128); w->w1 = c.take<double>(rows * ld, 128);
    w->w2 = c.take<double>(rows * ld, 128); w->w3 = c.take<double>(rows * ld, 128);
    w->tau = c.take<double>(S1);
    return c.total();
}
// noisy expected improvement, one call: [MT = the chunk's means, fantasy-major | score, mu R | mu_s R x S, var, tau (the host-array stage
// only, n_io = R or 0) | workgroup records nb + 1]
template <class Rec>
struct NeiCall { double *MT, *score, *mu, *var, *tau; Rec *blk, *best; };
template <class Rec>
size_t nei_call(const void* base, size_t n_mt, size_t R, size_t n_io, size_t S, size_t nb, NeiCall<Rec>* w) {
    Carve c(base);
    w->MT = c.take<double>(n_mt, 128);
    w->score = c.take<double>(R); w->mu = c.take<double>(R);
    w->var = c.take<double>(n_io); w->tau = c.take<double>(n_io ? S : 0);
    w->blk = c.take<Rec>(nb + 1, REC_ALIGN);
    w->best = w->blk + nb;
    return c.total();
}
// the pinned, device-visible result block of a small call (up to n_small candidates of up to dmax coordinates), in doubles:
// [score | mu | var (n_small each) | record: one arg-max record = four 32-bit words | gradient n_small x dmax | candidates n_small x dmax].
// Every caller synchronises before it returns, so the areas are free at the next call, and three callers borrow them on purpose: the
// append stages X in the gradient area, y in the score area and gets the pivot back in words[0]; mll gets its value back in score[0];
// mll_grad gets [mll | d lognoise | d mean | d kernel ...] (<= dmax + 4 doubles) in the gradient area.  A refit: words[0], words[1].
struct PinnedSmall { double *score, *mu, *var, *rec, *grad, *cand; int* words; };
inline size_t pinned_small(const void* base, size_t n_small, size_t dmax, PinnedSmall* w) {
    Carve c(base);
    w->score = c.take<double>(n_small); w->mu = c.take<double>(n_small); w->var = c.take<double>(n_small);
    w->words = reinterpret_cast<int*>(w->rec = c.take<double>(2));
    w->grad = c.take<double>(n_small * dmax); w->cand = c.take<double>(n_small * dmax);
    return c.total();
}

}   // namespace layout
