// bohip.hip -- libbohip.so: C ABI (include/bohip.h) + host orchestration of the gfx950 kernels.
// Single translation unit (the kernel files are included) so one hipcc invocation builds the library.
//
// HBM layout per handle (capacity C observations, ld = round_up(C + 1, 128)):
//   dX  [C][d]      observations, row = one observation (= Julia's d x N column-major)
//   dy  [C]
//   dL  [ld][ld]    row-major; lower 128-tiles hold cK then its Cholesky factor L (= Julia's upper U
//                   read column-major); strict-upper tiles stay zero; rows/cols >= N identity padding
//   dW  [ld][ld]    W = L^-1 (lower).  Row N (first padding row) carries alpha' so the scoring
//                   contraction V = W K* also produces mu - beta.
//   dWT [ld][ld]    W' (upper): lets every contraction run in the K-major x K-major form of the MFMA engine
//   dS  [ld][ld]    scratch: solved panels during the factorisation, S' blocks during the recursive inverse,
//                   cK^-1 for the marginal-likelihood gradient
//   dKsT [Rc][ld]   cross-covariance chunk, candidate-major
// A posterior pass is planned once (PassPlan, choose_route) and the plan travels by argument; every whole-K pass is chunk_pass.  The handle keeps
// records of the last call and state that outlives a call, never the plan of a call in flight (DESIGN.md "Who owns the plan of a pass").
// There is NO CPU fallback: every entry point that computes fails with BOHIP_E_NODEVICE / BOHIP_E_HIP
// when the GPU is unavailable.
#include "../../include/bohip.h"
#include "../../include/bohip_paths.h"
#include "../../include/bohip_fit.h"
#include "../../include/bohip_qei.h"
#include "../../include/bohip_acq.h"
#include "../../include/bohip_kg.h"
#include "../../include/bohip_mes.h"
#include "../../include/bohip_ens.h"
#include "../../include/bohip_ens_grad.h"
#include "../../include/bohip_con.h"
#include "../../include/bohip_mo.h"
#include "../../include/bohip_mom.h"
#include "../../include/bohip_loo.h"
#include "../../include/bohip_loo_batch.h"
#include "../../include/bohip_rep.h"
#include "../../include/bohip_pend.h"
#include "../../include/bohip_nei.h"
#include "kernels_linalg.hip"
#include "kernels_loo.hip"     // (after the linear algebra: KernelHyper and the family expressions of k_dmll_parts)
#include "kernels_rep.hip"     // (replicated sites: the weighted diagonal and the weighted logNoise sum)
#include "kernels_chol.hip"
#include "kernels_exec.hip"
#include "kernels_score.hip"
#include "kernels_batch.hip"   // (after the scoring kernels: shares their functors and arg-max order)
#include "kernels_sample.hip"  // (after the scoring kernels: their generator and arg-max order)
#include "kernels_qei.hip"     // (after the scoring kernels: their arg-max order)
#include "kernels_kg.hip"      // (after the scoring kernels: their arg-max order; acq_log.h's forms of h)
#include "kernels_mes.hip"     // (after the scoring and sampling kernels: their generator and arg-max order; acq_log.h's continued fraction)
#include "kernels_path.hip"    // (after the scoring kernels: their generator, arg-max order and kernel expressions)
#include "kernels_con.hip"     // (after the scoring kernels: their functors, arg-max order and k_grad_finish's launch bounds; acq_log.h's continued fraction)
#include "kernels_mo.hip"      // (after the constrained kernels: their record block; the scoring kernels' arg-max order)
#include "kernels_mom.hip"     // (after the two-objective kernel: mo_psi and its grid cap)
#include "kernels_ascent.hip"
#include "kernels_pend.hip"   // (after the scoring kernels: their functors, arg-max order, generator and kernel expressions)
#include "kernels_nei.hip"    // (after the scoring kernels: their functors, arg-max order and generator; gemm_core.h's tile loop)
#include "kernels_fit.hip"     // (after the linear algebra: cov_from_r)
#include "kernels_ens.hip"     // (after the fit and the scoring kernels: the fit's panels and tasks, acq_eval and the arg-max order)
#include "kernels_small.hip"   // (after the ascent: k_small_u's last workgroup runs its step, asc_step_one<true>)
#include "direct_l.h"          // host bookkeeping of :GN_DIRECT_L (ask / tell)
#include "scratch_layout.h"    // devbuf.h (who owns device memory) and the layouts of the carved scratch blocks

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <vector>

using namespace bohip;
using devbuf::Grow;
template <class T>
using DBuf = devbuf::Buf<T>;         // device memory
template <class T>
using HBuf = devbuf::PinnedBuf<T>;   // pinned host memory

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(BOHIP_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ \
                                         ":" + std::to_string(__LINE__) + ")");                        \
    } while (0)
#define CHK(expr)              \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != 0) return rc_; \
    } while (0)

static_assert(sizeof(bohip_best) == sizeof(Best), "record layout");
static constexpr int SMALL_MAX = 256;                      // most candidates the row-wise path takes in one go
static constexpr int APP_UT_ROW0 = SMALL_MAX;              // rows [0, 256): V' / L21;  rows [256, 512): U' / T = L21 W11
static constexpr int APP_ROWS = 2 * SMALL_MAX;
static_assert(APPEND_PMAX <= SMALL_MAX && SMALL_R <= SMALL_MAX, "the append shares the small-batch row area");

static constexpr int CHOL_DF_TCAP = 96;   // the dataflow factorisation's flag storage is sized for this many row tiles
// The handle's streams and events, as a base of the handle: a base is destroyed after the members, so every buffer of bohip_gp
// frees itself (hipFree waits for the device) before the streams and events go -- the order bohip_gp_destroy always kept.
struct gp_streams {
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    hipStream_t side_stream = nullptr;            // bulk trailing updates of the factorisation run here (look-ahead)
    hipEvent_t ev_panels = nullptr, ev_bulk = nullptr;
    hipStream_t col_stream = nullptr;             // dataflow factorisation: bulk followers + column updates (high priority)
    hipEvent_t ev_inv = nullptr;
    hipEvent_t ev_gate = nullptr;                 // a diagonal-block kernel is about to start: release one piece of the pending bulk update
    hipEvent_t ev_con = nullptr;                  // joins this handle's stream to the objective's (constrained scoring; made on first use)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tpool;  // pooled event pairs of the stage timing
    gp_streams() = default;
    gp_streams(const gp_streams&) = delete;
    ~gp_streams() {
        if (ev_con) hipEventDestroy(ev_con);
        for (auto& e : tpool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
        if (side_stream) { hipStreamSynchronize(side_stream); hipStreamDestroy(side_stream); }
        if (ev_panels) hipEventDestroy(ev_panels);
        if (ev_bulk) hipEventDestroy(ev_bulk);
        if (col_stream) { hipStreamSynchronize(col_stream); hipStreamDestroy(col_stream); }
        if (ev_inv) hipEventDestroy(ev_inv);
        if (ev_gate) hipEventDestroy(ev_gate);
        if (own_stream) hipStreamDestroy(own_stream);
    }
};
extern "C" int bohip_gp_comm_destroy(bohip_gp* g);
struct bohip_gp : gp_streams {
    // The whole teardown (bohip_gp_destroy, and every failure path of bohip_gp_create): wait for the handle's stream, detach the
    // communicator; then the members free themselves, then ~gp_streams.
    ~bohip_gp() {
        hipSetDevice(device);
        if (own_stream) hipStreamSynchronize(own_stream);
        if (comm) bohip_gp_comm_destroy(this);
        delete nei;
    }
    int d = 0, kern = 0;
    int64_t n = 0, cap = 0, ld = 0;
    // Every buffer below owns its memory and knows its capacity (devbuf.h); the plain integers next to some of them are NOT
    // capacities but what the last call derived from one (a row count, a leading dimension, the T a table was built for).
    DBuf<double> dX, dy, dL, dW, dWT, dS;
    DBuf<double> dalpha, dr, dt, dmll;
    DBuf<double> dApp;  // [APP_ROWS][ld] scratch of the incremental append and of the row-wise (small-batch) posterior
    DBuf<int> dinfo;
    DBuf<unsigned> dchol_flags;        // dataflow factorisation (kernels_chol.hip): panel[T*8] | solved[T] | crit[T] | abort[1]
    DBuf<double> dchol_idl;            // [T*8][16][16] published inverses of the 16 x 16 pivot blocks
    std::vector<double> hX, hy;
    // replicated sites (include/bohip_rep.h): a handle turns weighted with the first site of more than one evaluation and
    // stays so.  Only a weighted handle holds dinvr [cap] = 1 / r_i (ones for plain rows) and its mirrors; hy then holds the site means.
    bool weighted = false;
    DBuf<double> dinvr;
    std::vector<double> hinvr;
    std::vector<int64_t> hreps;
    int64_t n_evals_extra = 0;          // N_tot - n
    double ss_total = 0.0, sum_log_reps = 0.0;   // sum_i s_i, sum_i log r_i
    double loglen[DMAX], logsig = 0.0, lognoise = -2.0, beta = 0.0;
    bool stale = true;
    int64_t n_factored = 0;  // observations covered by the current factor
    DBuf<ExTask> dex_tasks;                       // task records of the executor form (kernels_exec.hip), built once per (buffers, T)
    bool ex_bulk4_ok = false;   // the bulk queue may be claimed two tiles at a time (exec_bulk_stride_ok)
    int ex_T = 0, ex_nsf = 0, ex_inv_g = -1, ex_grp_min = -1, ex_qbeg[EX_NQ + 1] = {0};
    bool w_done = false;       // the last factorisation also produced W = L^-1 (executor form with its inverse queue)
    // scoring scratch
    DBuf<double> dKsT;
    DBuf<unsigned long long> dclk;        // [2] core-clock / wall-clock ticks of sampled k_trigemm_sq workgroups (timing runs)
    DBuf<int> dpieces;           // k_trigemm_sq's row pieces, heaviest first (trigemm_pieces)
    std::vector<int> hpieces;
    int n_pieces = 0, pieces_T = -1;
    int64_t pieces_alpha = -1;
    int64_t kst_rows = 0;        // rows the K*' chunk buffer holds
    int64_t score_chunk = 0;     // a record (BOHIP_INFO_SCORE_CHUNK): the chunk the scratch was last sized for; a pass takes its chunk from its own PassPlan
    int64_t score_launches = 0;  // k_trigemm_sq launches of the last posterior pass (BOHIP_INFO_SCORE_LAUNCHES)
    DBuf<double> dVT, dUT;  // gradient path: V' and U' = V' W chunks, candidate-major
    DBuf<double> dq, dmu_raw, dXs, dmu, dvar, dscore;
    DBuf<Best> dblock_best, dbest;
    DBuf<unsigned> dfz_cnt;        // fused finish of k_trigemm_sq: [tiles] arrivals per candidate tile + [1] finished tiles (kept at zero)
    DBuf<Best> dfz_best;           // [tiles] per-tile arg-max records
    int64_t fz_tiles = 0;          // the [tiles] of the two above: where the finished-tiles word sits
    bool fz_dirty = false;         // a fused call failed between its launches: clear the counters before the next one
    // pruned arg-max (pruned_pass): ONE allocation [packed K*' rows | q2 | mu2 | bounds | lists, marks | counters, record | k_kstar's partials | pieces]
    DBuf<char> dpr;
    std::vector<int> hpr_pieces;
    int* pr_pieces_at = nullptr;
    HBuf<unsigned> hprune_stat;        // pinned: round 2's list length of the last pruned call (prune_wanted)
    unsigned prune_seen = 0;           // the last figure prune_wanted read from it
    bool prune_retry = false;          // the next pruned call is the retry after a back-off (prune_wanted cleared the word)
    size_t pr_ks_len = 0;              // the packed K*' rows at the head of dpr, as the last pruned call laid them out (tests: the poison)
    int prune_r2_form = -1;            // tests (bohip_debug_prune_round2_form): -1 the rule, 0 the steady form, 1 the long form
    int prune_skip = 0;                // value-only calls left on the full pass before pruning is tried again
    // batch selection (bohip_gp_select_batch): V' of ALL candidates, and ONE block [u_i q x ldu | records | scalars | workgroup records | picked]
    DBuf<double> dBV;
    DBuf<char> dbatch;
    DBuf<double> dgrad;        // d x R gradient staging of the host-pointer entry point
    double asc_ftol_abs = 0.0, asc_xtol_rel = 0.0, asc_stopval = INFINITY;   // bohip_gp_set_ascent_stop (NLopt's ftol_abs / xtol_rel / stopval)
    double asc_maxtime = 0.0;    // bohip_gp_set_maxtime: wall-clock budget of one acquire_max call in seconds (NLopt maxtime), 0 = none
    int64_t batch_hint = 0;      // bohip_gp_set_batch_hint: choose the scoring path as if the batch had at least this many candidates
    DBuf<double> dsplit;         // split-K partial planes (batches of a few hundred candidates)
    DBuf<double> dgparts;        // [SMALL_MAX][16][2 DMAX] split partial sums of k_grad_finish (small batches)
    DBuf<unsigned> dgcount;      // per-candidate arrival counters (left at zero by the kernel)
    // round 5: the small-batch pass as two MFMA kernels (kernels_small.hip): one scratch block [part | v16 | qpart | mupart | post | fstash | gpart]
    DBuf<char> dsm;
    DBuf<unsigned> dsm_cnt;
    int sm_cnt_T = 0;   // row tiles the counters are laid out for
    // pinned, device-visible host block the kernels of a small batch (R <= SMALL_R) write their results into: the
    // 2-3 device-to-host copies of a call cost more than its kernels (each ~8 us of API + DMA set-up)
    HBuf<double> hpin;           // layout::pinned_small, made once by bohip_gp_create (null: the small batches take the copies)
    layout::PinnedSmall pin{};   // its areas (all null without the block)
    DBuf<double> dschur;         // [APPEND_PMAX][APPEND_PMAX] Schur complement of an append of >= 3 rows (k_schur_dots)
    // lock-step L-BFGS ascent of acquire_max (kernels_ascent.hip)
    AscentState asc{};
    DBuf<char> asc_block;          // one allocation behind all double arrays of asc
    DBuf<char> asc_ints;           // active, accepted
    HBuf<double> asc_hio;          // pinned staging of the one-launch ascent: [lb | ub | starts] in, the packed result out
    DBuf<double> asc_dio;          // its device mirror
    HBuf<char> asc_hints;          // pinned: h_accepted, h_active
    DBuf<double> asc_bounds;       // lb, ub, best_x (3 d doubles) + starts staging is dXs
    DBuf<Best> asc_best;
    int64_t asc_rows = 0;          // starts the pointers of asc are laid out for
    DBuf<Best> dthompson;      // S arg-max records
    DBuf<double> ddmll_parts;       // per-block partial sums of the marginal-likelihood gradient
    // batched marginal likelihood (bohip_gp_mll_grad_batch): the slabs of the settings of one launch, and [theta | mll | grad | pivot | stamps]
    DBuf<double> fit_ws;
    DBuf<char> fit_io;
    // marginalised acquisition (bohip_gp_score_ens): the settings' slabs are fit_ws; ONE block
    // [theta | w | w~ | pivot | xs chunk | each, mu, var H x Rc | scores R | workgroup records | record]
    DBuf<char> ens_io;
    // its gradient (bohip_gp_score_ens_grad): alpha = W' z per setting, and what the slabs hold -- the factors of ens_theta for the
    // observations of version ens_version, left by that symbol (ens_factor_ok) -- so that the next call with the same theta skips the factor stage
    DBuf<double> ens_alpha;
    bool ens_factor_ok = false;
    std::vector<double> ens_theta;
    std::vector<long long> ens_pivot;
    uint64_t ens_version = 0;
    uint64_t data_version = 0;   // raised by whatever changes X or y
    DBuf<double> dVV, dcov;  // [Rp][Rp] V'V (lower tiles) and the full posterior covariance
    int64_t cov_ld = 0;      // their leading dimension: the Rp they were made for
    // joint sampler (bohip_gp_sample_joint): a factor workspace the model does not own -- matrix, panel scratch, the 128 x 128
    // diagonal inverses -- plus [max diag | pivot word], the S x R draws (only when asked for) and the per-tile arg-max records
    DBuf<double> sjL, sjS, sjW, sjWT, sjF, sj_scal;
    DBuf<int> sj_info;
    DBuf<Best> sj_part;
    int64_t sj_rows = 0;          // rows (a multiple of 128) the workspace holds; its leading dimension is sj_rows + 16
    // greedy q-EI over the resident draws (bohip_gp_qei_batch / _qei_select): ONE block [m | partials | records | gain | idx | words]
    DBuf<char> qei_ws;
    // knowledge gradient (bohip_gp_kg / bohip_kg_lines): ONE block [kg | record | nseg | a | B], the last two for the caller's lines only
    DBuf<char> kg_ws;
    // max-value entropy search (bohip_gp_mes / bohip_mes_values / bohip_mes_gumbel): ONE block, see ensure_mes
    DBuf<char> mes_ws;
    // constrained scoring (bohip_gp_score_con / bohip_con_values / bohip_gp_predict_grad): ONE block on the objective's handle, see
    // ensure_con (ev_con joins this handle's stream to the objective's)
    DBuf<char> con_ws;
    // two-objective scoring (bohip_gp_score_mo / bohip_mo_ehvi_values): the front's corners and heights, 2 BOHIP_MO_FRONT_MAX + 3
    // doubles made on first use; everything else lives in ensure_con's block with C = 1
    DBuf<double> mo_front;
    // two to four objectives (bohip_gp_score_mom / bohip_mom_ehvi_values): the level arrays, BOHIP_MOM_OBJ_MAX rows of
    // BOHIP_MOM_FRONT_MAX + 2 doubles, and the packed boxes, M words each (grows with the front's box count); everything else lives in
    // ensure_con's block with C = M - 1
    DBuf<double> mom_levels;
    DBuf<unsigned> mom_boxes;
    // ... and the host's plan of what those two buffers hold now (null: nothing valid): a call with the same front and ref -- every step
    // of an ascent -- neither decomposes nor uploads again
    std::shared_ptr<struct MomPlan> mom_plan;
    // leave-one-out (bohip_gp_loo / bohip_gp_loo_grad): ONE block of vectors (layout::loo), and for the gradient one more matrix of
    // the model's size, Z = cK^-1 diag(sqrt c); both made on first use, nothing in them outlives a call
    DBuf<char> loo_ws;
    DBuf<double> dZ;
    // batched leave-one-out (bohip_gp_loo_grad_batch): [logp H x N] (layout::loo_batch_io), made when logp is asked for; the rest
    // of the call lives in fit_ws and fit_io
    DBuf<char> loo_batch_io;
    // pending evaluations (include/bohip_pend.h): the set as the caller gave it (host), and what is derived from it and
    // the model lazily -- V_p' [rows][ld] (the pending columns' V', as k_trigemm_sq stores it) and ONE block [Xp | mu_p | Sigma_p | L_p
    // | V_p'V_p | pivot word] -- valid while pend_key equals what it was computed from; plus the block of one call (layout::pend_call)
    std::vector<double> hpend;
    int64_t pend_p = 0;
    uint64_t pend_gen = 0, hyper_gen = 0;   // raised by bohip_gp_pending_set / bohip_gp_set_hyper
    struct PendKey {
        int64_t n = -1, ld = 0, refits = 0, appends = 0;
        uint64_t hyper_gen = 0, pend_gen = 0;
        double jitter = 0.0;
        bool operator==(const PendKey& o) const {
            return n == o.n && ld == o.ld && refits == o.refits && appends == o.appends && hyper_gen == o.hyper_gen &&
                   pend_gen == o.pend_gen && jitter == o.jitter;
        }
    } pend_key;
    DBuf<double> dPV;
    DBuf<char> pend_state, pend_call;
    // noisy expected improvement (include/bohip_nei.h): the COMPANION -- a handle of its own for the same X under the same
    // kernel parameters with delta on the diagonal, owned by this one, made at the first call of that header and kept in step lazily
    // (nei_jrel, nei_steps: what its diagonal was set from) -- and the fantasies [F | alpha_s | work | tau_s] (layout::nei_state), valid
    // while nei_key equals what they were computed from; plus the block of one call (layout::nei_call)
    bohip_gp* nei = nullptr;
    double nei_jrel = -1.0, nei_delta = 0.0;
    int nei_steps = 0;
    int64_t nei_rebuilds = 0, nei_ld = 0;
    struct NeiKey {
        int64_t n = -1, ld = 0, refits = 0, appends = 0, c_refits = 0, c_appends = 0, S = -1;
        uint64_t hyper_gen = 0, data_version = 0, seed = 0;
        double jitter = 0.0, delta = 0.0;
        bool operator==(const NeiKey& o) const {
            return n == o.n && ld == o.ld && refits == o.refits && appends == o.appends && c_refits == o.c_refits && c_appends == o.c_appends &&
                   S == o.S && hyper_gen == o.hyper_gen && data_version == o.data_version && seed == o.seed && jitter == o.jitter &&
                   delta == o.delta;
        }
    } nei_key;
    DBuf<char> nei_ws, nei_call;
    // one-process-per-device exchange (multigpu.hip): communicator attached by bohip_gp_comm_init
    void* comm = nullptr;
    int comm_rank = 0, comm_n = 0;
    int64_t comm_exchanges = 0;        // BOHIP_INFO_COMM_EXCHANGES: all-gathers this handle has issued on its communicator
    DBuf<Best> csend, crecv, cfinal;
    // bookkeeping
    int64_t pivot = 0, refits = 0, appends = 0;
    int alpha_inc_run = 0;         // appends since alpha was last computed in full (compute_alpha); the incremental form re-synchronises every 256
    bool mirror_dirty = false;     // a staged append failed after the host mirrors advanced: the next refit uploads X and y again
    int64_t chol_lock_skips = 0;   // refits that took the launch-chained form because another process held the refit lock
    int chol_form_last = 0;            // BOHIP_INFO_CHOL_FORM: 0 launch chain, 4 executor (1-3: retired forms, never reported)
    int64_t chol_fallbacks = 0;        // BOHIP_INFO_CHOL_FALLBACKS: refits of this handle that timed out on a dependency and were redone launch-chained
    int chol_abort_T = 0;              // BOHIP_INFO_CHOL_ABORT_TILES: row tiles of the last factorisation that timed out (0: never)
    // jitter escalation on a failed factorisation (GaussianProcesses.jl make_posdef!, UPSTREAM-UNVERIFIED: off by default)
    double jitter_rel = 0.0;           // first jitter = jitter_rel x mean(diag cK), x10 per further try
    int jitter_tries = 0;              // 0 = report BOHIP_E_NOTPD at once (the default)
    int jitter_steps_last = 0;         // BOHIP_INFO_JITTER_STEPS: tries the last refit needed (0: none)
    double jitter_last = 0.0;          // what it added to the diagonal
    bool timing = false;
    bool t_open = false;
    bool timing_dominant_only = false;   // enable_timing(2): only the dominant kernel (k_trigemm_sq) is bracketed by events
    bool timing_accumulate = false;      // enable_timing(3): as 2, and the event pairs of successive calls pile up unread until
                                         // bohip_gp_get_timing (no hipEventSynchronize / hipEventElapsedTime inside a timed loop)
    size_t tused = 0;   // event pairs of tpool in use
    std::vector<const char*> tlabel;
    std::vector<std::string> tnames;
    std::vector<double> tms;
};

// ABI kernel id -> the family the device kernels branch on, and whether the kernel has one length-scale (iso)
static int kern_family(int id) {
    switch (id) {
        case KERN_MAT52ARD: case KERN_MAT52ISO: return FAM_M52;
        case KERN_MAT32ARD: case KERN_MAT32ISO: return FAM_M32;
        case KERN_MAT12ARD: case KERN_MAT12ISO: return FAM_M12;
        default: return FAM_SE;
    }
}
static bool kern_iso(int id) { return id == KERN_SEISO || id == KERN_MAT52ISO || id == KERN_MAT32ISO || id == KERN_MAT12ISO; }

// The kernels that evaluate k are instantiated twice (template argument LOW): the Matérn 1/2 and 3/2 families run their own
// instantiation, so the SE / Matérn 5/2 one compiles to the code it had before those families existed.
static bool fam_low(int fam) { return fam == FAM_M12 || fam == FAM_M32; }
static bool fam_low(const KernelHyper& h) { return fam_low(h.fam); }
#define LAUNCH_FAM(lo, k_low, k_std, ...) \
    do { if (lo) hipLaunchKernelGGL(k_low, __VA_ARGS__); else hipLaunchKernelGGL(k_std, __VA_ARGS__); } while (0)

// The kernels that loop over the coordinates are instantiated per dimension bucket DT = 2, 4, 8, 16, 32, 64 (CAP: the largest one the
// caller's kernel is compiled for): f(std::integral_constant<int, DT>{}) for the smallest bucket that holds d.
template <int CAP = DMAX, class F>
static auto dispatch_dt(int d, F&& f) {
    static_assert(CAP == 16 || CAP == 64, "a ladder ends at 16 or at DMAX = 64");
    if (d <= 2) return f(std::integral_constant<int, 2>{});
    if (d <= 4) return f(std::integral_constant<int, 4>{});
    if (d <= 8) return f(std::integral_constant<int, 8>{});
    if constexpr (CAP == 16) {
        return f(std::integral_constant<int, 16>{});
    } else {
        if (d <= 16) return f(std::integral_constant<int, 16>{});
        if (d <= 32) return f(std::integral_constant<int, 32>{});
        return f(std::integral_constant<int, 64>{});
    }
}

// (acq_id, acq_params) of the C ABI as the kernels take them: p0 of every acquisition but MaxMean, p1 of MI
static int make_acq(int acq_id, const double* acq_params, AcqParams* out) {
    if (acq_id != BOHIP_ACQ_MAXMEAN && !acq_params) return fail(BOHIP_E_ARG, "acq_params required for this acquisition");
    *out = AcqParams{acq_id, 0.0, 0.0};
    if (acq_id != BOHIP_ACQ_MAXMEAN) out->p0 = acq_params[0];
    if (acq_id == BOHIP_ACQ_MI) out->p1 = acq_params[1];
    return 0;
}

static KernelHyper make_hyper(const bohip_gp* g) {
    KernelHyper h;
    h.fam = kern_family(g->kern);
    h.d = g->d;
    h.sigma2 = std::exp(2.0 * g->logsig);
    for (int k = 0; k < DMAX; ++k) h.il2[k] = 0.0;
    for (int k = 0; k < g->d; ++k) h.il2[k] = std::exp(-2.0 * g->loglen[kern_iso(g->kern) ? 0 : k]);
    return h;
}

// ---- stage timing (HIP events on the handle's stream; the event pairs are pooled, not re-created per call) -------
static bool t_skip(const bohip_gp* g, const char* name) {
    return g->timing_dominant_only && std::strncmp(name, "trigemm_sq", 10) != 0;
}
static void t_begin(bohip_gp* g, const char* name) {
    if (!g->timing) return;
    g->t_open = !t_skip(g, name);
    if (!g->t_open) return;
    if (g->timing_accumulate && g->tused >= 8192) {   // nobody reads them: keep the newest (mode 3 piles pairs up until get_timing)
        std::rotate(g->tpool.begin(), g->tpool.begin() + 4096, g->tpool.begin() + g->tused);
        g->tlabel.erase(g->tlabel.begin(), g->tlabel.begin() + 4096);
        g->tused -= 4096;
    }
    if (g->tused == g->tpool.size()) {
        hipEvent_t a, b;
        hipEventCreate(&a);
        hipEventCreate(&b);
        g->tpool.push_back({a, b});
    }
    hipEventRecord(g->tpool[g->tused].first, g->stream);
    g->tlabel.push_back(name);
    ++g->tused;
}
static void t_end(bohip_gp* g) {
    if (!g->timing || g->tused == 0 || !g->t_open) return;
    g->t_open = false;
    hipEventRecord(g->tpool[g->tused - 1].second, g->stream);
}
static void t_reset(bohip_gp* g) {
    if (g->timing_accumulate) return;
    g->tused = 0;
    g->tlabel.clear();
}
static void t_collect(bohip_gp* g, bool force = false) {
    if (!g->timing) return;
    if (g->timing_accumulate && !force) return;
    g->tnames.clear();
    g->tms.clear();
    for (size_t i = 0; i < g->tused; ++i) {
        hipEventSynchronize(g->tpool[i].second);
        float ms = 0.f;
        hipEventElapsedTime(&ms, g->tpool[i].first, g->tpool[i].second);
        g->tnames.push_back(g->tlabel[i]);
        g->tms.push_back(ms);
    }
    g->tused = 0;
    g->tlabel.clear();
}

// ---- allocation -----------------------------------------------------------------------------------
static int free_model(bohip_gp* g) {
    for (DBuf<double>* b : {&g->dX, &g->dy, &g->dL, &g->dW, &g->dWT, &g->dS, &g->dalpha, &g->dr, &g->dt, &g->dApp, &g->dchol_idl}) b->release();
    g->dchol_flags.release();
    g->dinvr.release();
    g->ex_T = 0;   // the task records hold pointers into the buffers just freed
    return 0;
}
static size_t chol_flag_words(int T);
static size_t chol_abort_word(int T);
// ---- replicated sites (include/bohip_rep.h) ----------------------------------------------------------------------------------------
// The weights of a weighted handle as the device holds them: dinvr sized like dy, filled from the host mirror (capacity growth, a
// failed staged append, the plain rows that were there when the handle turned weighted).
static int upload_site_weights(bohip_gp* g) {
    HIPCHK(g->dinvr.reserve(std::max<size_t>(1, (size_t)std::max(g->cap, g->n)), g->stream));
    if (g->n > 0) HIPCHK(hipMemcpyAsync(g->dinvr, g->hinvr.data(), (size_t)g->n * 8, hipMemcpyHostToDevice, g->stream));
    return 0;
}
// The entry points that build cK from dX / dy in kernels of their own (or scale the noise themselves) know no per-row noise term:
// on a weighted handle they refuse instead of answering for a different model.
static int refuse_weighted(const bohip_gp* g, const char* who) {
    if (!g || !g->weighted) return 0;
    return fail(BOHIP_E_UNSUPPORTED, std::string(who) + " does not support a model with replicated sites (bohip_gp_append_sites with reps > 1): "
                                         "its kernels build the covariance with one noise term for every row");
}
static int alloc_model(bohip_gp* g, int64_t cap) {
    free_model(g);
    // chunk buffers are sized by ld: drop them, they are re-made on demand
    for (DBuf<double>* b : {&g->dKsT, &g->dVT, &g->dUT, &g->dq, &g->dBV}) b->release();
    g->kst_rows = 0;
    g->cap = cap;
    // +16 doubles: row stride is an ODD multiple of 128 B, so the 128 rows of a tile spread over the L2/HBM
    // channels instead of camping on one (a power-of-two stride sends every row of a tile to the same channel).
    g->ld = round_up(cap + 1, TILE) + 16;
    const size_t ld = (size_t)g->ld, mat = ld * ld * sizeof(double);
    hipStream_t st = g->stream;   // (everything was just released: no reserve below waits for it)
    HIPCHK(g->dX.reserve(std::max<size_t>(1, (size_t)cap * g->d), st));
    HIPCHK(g->dy.reserve(std::max<size_t>(1, (size_t)cap), st));
    for (DBuf<double>* b : {&g->dL, &g->dW, &g->dWT, &g->dS}) HIPCHK(b->reserve(ld * ld, st));
    // (+256: k_trimv_stream reads its right-hand sides in whole chunks of 256, masked by index)
    for (DBuf<double>* b : {&g->dalpha, &g->dr, &g->dt}) HIPCHK(b->reserve(ld + 256, st));
    HIPCHK(g->dApp.reserve((size_t)APP_ROWS * ld, st));
    {
        const size_t Tm = (size_t)(g->ld / TILE) + 1;
        HIPCHK(g->dchol_flags.reserve(chol_flag_words((int)std::min<size_t>(Tm, CHOL_DF_TCAP)), st));
        HIPCHK(g->dchol_idl.reserve(Tm * CH_PANELS * 256, st));   // W16 of every pivot block
    }
    HIPCHK(hipMemsetAsync(g->dL, 0, mat, g->stream));
    HIPCHK(hipMemsetAsync(g->dW, 0, mat, g->stream));
    HIPCHK(hipMemsetAsync(g->dWT, 0, mat, g->stream));
    HIPCHK(hipMemsetAsync(g->dS, 0, mat, g->stream));
    if (g->n > 0) {
        HIPCHK(hipMemcpyAsync(g->dX, g->hX.data(), (size_t)g->n * g->d * 8, hipMemcpyHostToDevice, g->stream));
        HIPCHK(hipMemcpyAsync(g->dy, g->hy.data(), (size_t)g->n * 8, hipMemcpyHostToDevice, g->stream));
    }
    if (g->weighted) CHK(upload_site_weights(g));
    g->stale = true;
    return 0;
}

// ---- GEMM launcher --------------------------------------------------------------------------------
static int g_bulk_pieces = 4;   // gated pieces of the side-stream bulk update per outer block (BOHIP_BULK_PIECES; 0/1: one launch)
static int g_sample_mfma_min = 200;  // BOHIP_SAMPLE_MFMA_MIN: draws from which bohip_gp_sample_joint takes k_sample_mfma instead of k_sample_rows
                                     // (measured at R = 4096: the two cross between 192 and 256 draws, kernels_sample.hip)
static int g_path_mfma_min = 24;     // BOHIP_PATH_MFMA_MIN: paths from which bohip_paths_eval takes k_path_mfma instead of k_path_rows (read at every
                                     // bohip_gp_paths_draw and kept by the object).  The forms cross at ~130 paths at R = 4096 and at ~15 at R = 65536
                                     // (the MFMA form is flat at 1.13 ms until its grid fills the chip, the row form is linear in S); the switch is on S
                                     // alone so that a path's bits do not depend on R, and 24 favours large candidate sets
static int g_split = 1;   // split-K path for batches of a few hundred candidates (BOHIP_SPLIT=0 disables)
static int g_asc_wg_nmax = 256;  // BOHIP_ASC_WG_NMAX: models up to this many observations run acquire_max as ONE launch, one workgroup per start point
                                 // (kernels_ascent.hip k_ascent_wg); 0: never
static const double g_asc_first_step = 0.1;   // the first step is never shorter than this fraction of the smallest box side (kernels_ascent.hip asc_direction_one)
static int g_asc_fold = 1;       // the free-running form's step inside k_small_u's last workgroup (BOHIP_ASC_LOCKSTEP=2: as a launch of its own, until round 6)
static int g_asc_lockstep = 0;   // BOHIP_ASC_LOCKSTEP=1: the lock-step driver of the device ascent (five launches + a stream synchronisation per
                                 // evaluation pass) instead of the free-running one (k_asc_step)
static int g_small_m = 0;      // BOHIP_SMALL_M: 128-chunks of the contraction index per tile of those kernels; 0 = by size
static int g_small_r = -1;  // batches up to this size (<= 256) take the row-wise path; -1: min(256, 90 + 300000 / N), the measured
                            // break-even with the MFMA path (N=500: > 256, N=3000: ~190, N=10000: ~110); BOHIP_SMALL_R overrides: below that
                            // candidates one 64-wide MFMA tile column leaves single workgroups walking the whole K extent
static int g_inv_hi_h = 16;            // levels of the triangular inverse with half-size >= this many tiles run as throughput launches (BOHIP_INV_HI_H)
static int g_chol_df = 1;  // dataflow factorisation (the executor form: kernels_chol.hip + kernels_exec.hip) for up to g_chol_df_tmax row tiles, see refit_once:
                            // N=3000 1.66 vs 2.71 ms, N=1000 0.57 vs 0.82 ms against the launch chain.  BOHIP_CHOL_DATAFLOW=0 disables, any other value is on.
static bool g_chol_df_strict = false;   // BOHIP_CHOL_DF_STRICT: a timed-out dependency is an error instead of a fall-back (tests, tools)
static bool g_chol_df_dump = false;     // measurement builds: the flags of a timed-out factorisation on stderr
static int g_chol_df_tmax = 96;   // = CHOL_DF_TCAP, N <= ~12200 (N=12000: 16.5 vs 18.5 ms for the launch chain)
// A dataflow factorisation that timed out on a dependency (another process holds the CUs, two streams share a hardware queue, ...)
// switches the PROCESS to the launch chain -- for the next `skip` refits, not for good: the cause is usually transient, a
// time-out costs one bounded wait (200 ms), and every further time-out doubles the pause (8, 24, 56, ... up to 1024 refits).
static std::atomic<int> g_chol_df_skip{0}, g_chol_df_backoff{0};
static unsigned long long g_chol_spin_ticks = CH_SPIN_TICKS_DEFAULT;   // BOHIP_CHOL_SPIN_US: bound of every in-kernel wait of the dataflow form
static int g_chol_exec_patience_us = 1000;   // BOHIP_CHOL_EXEC_PATIENCE_US: how long a workgroup only polls a held record before it takes other work meanwhile
static int g_chol_exec_fill_inv = 1;    // a workgroup waiting for the counters of a claimed task runs inverse-wave tasks meanwhile (BOHIP_CHOL_EXEC_FILL_INV)
static int g_chol_exec_inv_pairs = 0;   // inverse queue claimed one record (0) or one tile = two records (1) at a time (BOHIP_CHOL_EXEC_INV_PAIRS)
static std::atomic<int> g_chol_inv_grp_min{28};   // row tiles from which the inverse queues take the GROUP form (exec_task_list); BOHIP_CHOL_INV_GRP_MIN.  40 until the end of
                                                  // round 6: with that round's faster chain the group form wins from 28 row tiles on (28 ... 39 row tiles: -3 ... -7 %, 26: +3 %, 24: +4 %)
static std::atomic<int> g_chol_inv_g{8};      // executor form: W = L^-1 is grown behind the chain by a fifth task queue, in pieces of this many 128-blocks
                                   // of contraction (BOHIP_CHOL_INV_G; 0 = off: the level-by-level inverse runs after the factorisation)
static int g_chol_nsf = 3;         // solve-follower workgroups of the chain kernel in the executor form (BOHIP_CHOL_NSF, 1..6)
static int g_chol_exec_urgent = -1; // executor workgroups that serve the urgent queue only (BOHIP_CHOL_EXEC_URGENT); -1: 32, and 16 from 56 row tiles on
                                    // (N = 10^4: 14.0-14.2 against 14.3 ms; 8 starve the chain at N = 6000: 4.75 against 3.95; profiles/r04_inverse_group_form.txt)
static int g_chol_exec_second = 1;   // BOHIP_CHOL_EXEC_SECOND=0: every executor workgroup serves every queue (until round 4).  1: the workgroups beyond one per CU take
                                     // throughput work only (early sums, bulk, waves) and leave when it is exhausted: N = 6000 4.60 -> 4.38 ms, N = 5000 3.27 -> 3.18
static int g_small_zero_copy = 1;          // small host calls: candidates read from the pinned block (0 in the measurement build: copied to HBM first)
static int g_chol_exec_nbu = 2;      // BOHIP_CHOL_EXEC_NBU: rows behind the solve followers whose row step (Solve, Late) sits in the urgent queue
static int g_chol_exec_fast = -1;    // BOHIP_CHOL_EXEC_FAST: executor workgroups that never take bulk / wave tasks (-1: where CUs hold two executor workgroups and the chain paces, 33 ... 48 row tiles: up to 112)
static int g_chol_exec_pairs = -1; // early sums and bulk updates are claimed two records (= both halves of a tile) at a time (BOHIP_CHOL_EXEC_PAIRS=1; 0: one); p >= 2: the bulk 2 p
                                    // records (p tiles) per claim.  -1: 1, and 2 from 72 row tiles on (N = 10^4 14.05 -> 13.8 ms, N = 12000 23.1 -> 22.6; N = 8000 the same, N = 6000 4.0 -> 4.25)
static int g_chol_exec_wgs = -1;  // executor workgroups (BOHIP_CHOL_EXEC_WGS); -1: by size -- ONE per free CU up to 32 row tiles, two from 45 on (see cholesky_exec)
static int g_append_alpha_inc = 1;   // incremental alpha on append (BOHIP_APPEND_ALPHA_INC=0: recomputed as W'(W r))
static int64_t g_chunk_rows_forced = 0;   // BOHIP_CHUNK_ROWS: candidates per K*' chunk (tools: chunk-size sweeps), 0 = the rule in chunk_rows
static int g_prune_m = -1;  // pruned arg-max: row tiles of the bounding prefix (BOHIP_PRUNE_M; 0: off, -1: the rule in prune_tiles)
static int g_pa_order = 1;  // phase A's job order (BOHIP_PA_ORDER): 0 heaviest first, 1 the middle third first (phase_a_jobs): bench shape 22.1 -> 20.2 us
static int launch_gemm_nt(bohip_gp* g, const GemmNTParams& p, int batch = 1, hipStream_t st = nullptr, bool hi = false) {
    if (p.mt <= 0 || p.nt64 <= 0 || p.kc <= 0 || batch <= 0) return 0;
    if (hi) hipLaunchKernelGGL(k_gemm_nt_hi, dim3(p.mt * p.nt64, batch), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), st ? st : g->stream, p);
    else hipLaunchKernelGGL(k_gemm_nt, dim3(p.mt * p.nt64, batch), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), st ? st : g->stream, p);
    HIPCHK(hipGetLastError());
    return 0;
}

static int device_cus();
// Measurement builds only (make abl/libbohip_dev.so, -DBOHIP_DEV_KNOBS=1): the constants the sweeps under tools/ vary, by
// name.  The shipped library does not read them -- each has a measured default recorded beside its declaration above.
static void read_dev_knobs() {
#if BOHIP_DEV_KNOBS
    struct Knob { const char* name; int* v; int lo, hi; };
    static int chunk_rows = 0, dump = 0;
    const Knob knobs[] = {
        {"BOHIP_CHOL_DF_TMAX", &g_chol_df_tmax, 0, CHOL_DF_TCAP}, {"BOHIP_INV_HI_H", &g_inv_hi_h, 0, 1 << 20},
        {"BOHIP_CHOL_EXEC_PAIRS", &g_chol_exec_pairs, -1, 64},
        {"BOHIP_CHOL_EXEC_URGENT", &g_chol_exec_urgent, 1, 1 << 20}, {"BOHIP_CHOL_NSF", &g_chol_nsf, 1, CH_NSF_MAX},
        {"BOHIP_CHOL_EXEC_PATIENCE_US", &g_chol_exec_patience_us, 0, 1 << 30}, {"BOHIP_CHOL_EXEC_FILL_INV", &g_chol_exec_fill_inv, 0, 1},
        {"BOHIP_CHOL_EXEC_INV_PAIRS", &g_chol_exec_inv_pairs, 0, 1}, {"BOHIP_CHOL_EXEC_WGS", &g_chol_exec_wgs, 1, 1 << 20},
        {"BOHIP_CHOL_EXEC_FAST", &g_chol_exec_fast, -1, 1 << 20},
        {"BOHIP_CHOL_EXEC_SECOND", &g_chol_exec_second, 0, 1}, {"BOHIP_SMALL_ZERO_COPY", &g_small_zero_copy, 0, 1}, {"BOHIP_CHOL_EXEC_NBU", &g_chol_exec_nbu, 0, 16}, {"BOHIP_CHUNK_ROWS", &chunk_rows, 0, 1 << 30},
        {"BOHIP_PRUNE_M", &g_prune_m, -1, 1 << 16}, {"BOHIP_PA_ORDER", &g_pa_order, 0, 1},
        {"BOHIP_APPEND_ALPHA_INC", &g_append_alpha_inc, 0, 1}, {"BOHIP_BULK_PIECES", &g_bulk_pieces, 0, 8}, {"BOHIP_SPLIT", &g_split, 0, 1},
        {"BOHIP_SMALL_R", &g_small_r, 0, SMALL_MAX}, {"BOHIP_SMALL_M", &g_small_m, 0, 1 << 20}, {"BOHIP_CHOL_DF_DUMP", &dump, 0, 1},
    };
    for (const Knob& k : knobs)
        if (const char* e = getenv(k.name)) *k.v = std::min(k.hi, std::max(k.lo, atoi(e)));
    g_chunk_rows_forced = chunk_rows;
    g_chol_df_dump = dump != 0;
#endif
}

// The per-device once-guard: the > 64 KB dynamic-LDS opt-in is a per-device function attribute, so every place that launches such a
// kernel keeps one table of its own (a function-local static; one per instantiation of a template) and runs its set-up through this at
// the point of first use.  A set-up that fails is tried again by the next call.
template <class Setup>
static int once_per_device(bool (&done)[64], int device, Setup&& setup) {
    if (done[device & 63]) return 0;
    CHK(setup());
    done[device & 63] = true;
    return 0;
}

static int kernel_setup_of_this_device() {
    HIPCHK(hipFuncSetAttribute((const void*)k_potf2_inv, hipFuncAttributeMaxDynamicSharedMemorySize, POTF2_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute((const void*)k_gemm_nt, hipFuncAttributeMaxDynamicSharedMemorySize, glds3_lds_bytes<4>()));
    HIPCHK(hipFuncSetAttribute((const void*)k_trigemm_sq, hipFuncAttributeMaxDynamicSharedMemorySize, glds3_lds_bytes<4>()));
    HIPCHK(hipFuncSetAttribute((const void*)k_trigemm_sq_pa, hipFuncAttributeMaxDynamicSharedMemorySize, glds3_lds_bytes<4>()));
    HIPCHK(hipFuncSetAttribute((const void*)k_trigemm_rows, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute((const void*)k_batch_cond<true>, hipFuncAttributeMaxDynamicSharedMemorySize, BATCH_LDS_MAX));
    HIPCHK(hipFuncSetAttribute((const void*)k_batch_cond<false>, hipFuncAttributeMaxDynamicSharedMemorySize, BATCH_LDS_MAX));
    HIPCHK(hipFuncSetAttribute((const void*)k_chol_chain, hipFuncAttributeMaxDynamicSharedMemorySize, CH_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute((const void*)k_gemm_nt_hi, hipFuncAttributeMaxDynamicSharedMemorySize, glds3_lds_bytes<4>()));
    HIPCHK(hipFuncSetAttribute((const void*)k_chol_exec, hipFuncAttributeMaxDynamicSharedMemorySize, glds3_lds_bytes<4>()));
    HIPCHK(hipFuncSetAttribute((const void*)k_trimv_stream<TRIMV_D>, hipFuncAttributeMaxDynamicSharedMemorySize, trimv_lds_bytes(TRIMV_D)));
    HIPCHK(hipFuncSetAttribute((const void*)k_path_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)path_mfma_lds_bytes(DMAX)));
    HIPCHK(hipFuncSetAttribute((const void*)k_path_mfma<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)path_mfma_lds_bytes(DMAX)));
    HIPCHK(hipFuncSetAttribute((const void*)k_kg<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kg_lds_bytes(KG_RMAX)));
    HIPCHK(hipFuncSetAttribute((const void*)k_kg<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kg_lds_bytes(KG_RMAX)));
    // The library's switches (README "Environment"): the forms of the factorisation the tests select, the bound of its
    // waits, the ascent drivers, the small-batch pass.  Everything else that used to be read here is a constant now; the
    // sweeps under tools/ that vary those constants run against csrc/abl/libbohip_dev.so (read_dev_knobs below).
    if (const char* e = getenv("BOHIP_CHOL_DATAFLOW")) g_chol_df = atoi(e);
    if (const char* e = getenv("BOHIP_CHOL_SPIN_US")) g_chol_spin_ticks = 100ull * (unsigned long long)std::max(1, atoi(e));
    if (const char* e = getenv("BOHIP_CHOL_INV_G")) g_chol_inv_g = std::min(64, std::max(0, atoi(e)));
    if (const char* e = getenv("BOHIP_CHOL_INV_GRP_MIN")) g_chol_inv_grp_min = std::max(0, atoi(e));
    if (const char* e = getenv("BOHIP_ASC_WG_NMAX")) g_asc_wg_nmax = std::max(0, atoi(e));
    if (const char* e = getenv("BOHIP_ASC_LOCKSTEP")) { g_asc_lockstep = atoi(e) == 1; g_asc_fold = atoi(e) != 2; }
    if (const char* e = getenv("BOHIP_SAMPLE_MFMA_MIN")) g_sample_mfma_min = std::max(1, atoi(e));
    g_chol_df_strict = getenv("BOHIP_CHOL_DF_STRICT") != nullptr;
    read_dev_knobs();
    return 0;
}
static int one_time_kernel_setup() {
    static bool done[64] = {false};
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    return once_per_device(done, dev, kernel_setup_of_this_device);
}

// ---- A1-A3: full rebuild --------------------------------------------------------------------------
static int launch_rows_trimv(bohip_gp* g, const double* W, int64_t N0, const double* rows, int P, double* out, int upper);
static int compute_alpha(bohip_gp* g) {
    // alpha = W'(W (y - beta)): two passes of the row-wise kernel (W, then the resident W' as an upper-triangular
    // K-major matrix) with one right-hand side
    const int64_t N = g->n;
    g->alpha_inc_run = 0;
    // (dr = y - beta and dt = W (y - beta) stay behind for the incremental update of the appends: nothing else may write them between refits)
    hipLaunchKernelGGL(k_sub_mean, dim3((N + 255) / 256), dim3(256), 0, g->stream, g->dy, g->beta, N, g->dr);
    HIPCHK(hipGetLastError());
    CHK(launch_rows_trimv(g, g->dW, N, g->dr, 1, g->dt, 0));
    CHK(launch_rows_trimv(g, g->dWT, N, g->dt, 1, g->dalpha, 1));
    // alpha' into the first padding row of W (cols < N); W[N][N] = 1 meets K*[N] = 0.
    HIPCHK(hipMemcpyAsync(g->dW + N * g->ld, g->dalpha, (size_t)N * 8, hipMemcpyDeviceToDevice, g->stream));
    return 0;
}

static int check_info(bohip_gp* g) {
    int local = 0;
    int* const pw = g->hpin ? g->pin.words + 1 : &local;   // through the pinned block: a plain DMA command (a pageable destination is staged by the runtime)
    HIPCHK(hipMemcpyAsync(pw, g->dinfo, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    const int info = *pw;
    if (info != 0) {
        g->pivot = info;
        g->stale = true;
        return fail(BOHIP_E_NOTPD, "kernel matrix not positive definite at pivot " + std::to_string(info));
    }
    g->pivot = 0;
    return 0;
}

// ---- W = L^-1 by blocks:  [L11 0; L21 L22]^-1 = [W11 0; -W22 L21 W11, W22].  With W' kept beside W both products are
// K-major x K-major:   S'[c][i]  =  sum_k W11'[c][k] L21[i][k]     (A = W' block, upper-triangular: k >= c)
//                      W21[i][c] = -sum_k W22[i][k]  S'[c][k]      (A = W22, lower-triangular: k <= i); W21' goes to W' too
// S' lives in the (otherwise unused) upper-right part of the scratch matrix dS, whose lower part holds the solved panels
// (= L21; dL receives them only with the final copy).
// inverse_level: all pairs of half-size h (tiles) inside the diagonal region [t0, t0 + nt), one batched launch each.
static int inverse_level(bohip_gp* g, hipStream_t st, int t0, int nt, int h) {
    const int64_t ld = g->ld, base = (int64_t)t0 * TILE * (ld + 1);
    const int pairs = (nt + 2 * h - 1) / (2 * h);
    const int64_t zs = (int64_t)2 * h * TILE * (ld + 1);
    const int64_t off21 = (int64_t)h * TILE * ld, off12 = (int64_t)h * TILE, off22 = (int64_t)h * TILE * (ld + 1);
    GemmNTParams a{};
    a.A = g->dWT + base; a.lda = ld; a.B = g->dS + base + off21; a.ldb = ld; a.C = g->dS + base + off12; a.ldc = ld;
    a.zA = a.zB = a.zC = zs;
    a.mt = h; a.nt64 = 2 * h; a.kc = h * (TILE / KC); a.alpha = 1.0; a.beta = 0.0; a.klo_from_m = 1;
    a.row_t0 = 0; a.row_ts = 2 * h; a.col_t0 = h; a.col_ts = 2 * h; a.total_t = nt;
    const bool big = h >= g_inv_hi_h;   // large levels are throughput launches: two workgroups per CU, stores through LDS
    a.coalesced = big ? 1 : 0;
    CHK(launch_gemm_nt(g, a, pairs, st, big));
    GemmNTParams b{};
    b.A = g->dW + base + off22; b.lda = ld; b.B = g->dS + base + off12; b.ldb = ld; b.C = g->dW + base + off21; b.ldc = ld;
    b.CT = g->dWT + base + off12; b.ldct = ld;
    b.zA = b.zB = b.zC = b.zCT = zs;
    b.mt = h; b.nt64 = 2 * h; b.kc = h * (TILE / KC); b.alpha = -1.0; b.beta = 0.0; b.khi_from_m = 1;
    b.row_t0 = h; b.row_ts = 2 * h; b.col_t0 = 0; b.col_ts = 2 * h; b.total_t = nt;
    b.coalesced = big ? 1 : 0;
    CHK(launch_gemm_nt(g, b, pairs, st, big));
    return 0;
}

// ---- A2, the flag area of the dataflow factorisation (kernels_chol.hip, kernels_exec.hip), in words:
//   panel[8 T] | solved[T] | crit[T] | rest[T] | col[T] | farall[T] | fol[T] | colall[T] | colr[T T] | xp[8 T T] | abort word |
//   the executor's six queue cursors | one spare word | the inverse queues' counters [4 T T] | xp3[8 T] | pre3[4 T]
// The executor's task records address words by this layout (exec_task_list); words nobody waits on any more stay allocated.
static size_t chol_abort_word(int T) { return (size_t)T * (CH_PANELS + 7) + (size_t)T * T * (CH_PANELS + 1); }
static size_t chol_inv_word(int T) { return chol_abort_word(T) + 8; }      // the inverse queue's counters: 4 words per tile (i, j)
static size_t chol_xp3_word(int T) { return chol_inv_word(T) + (size_t)4 * T * T; }    // per-panel flags of S(k+3, k) (8 per block), then pre3 (4 per block)
static size_t chol_flag_words(int T) { return chol_xp3_word(T) + (size_t)12 * T; }       // abort word + the executor's queue cursors + those
static CholFlags chol_flags_layout_at(unsigned* base, double* idl, int T);
static CholFlags chol_flags_layout(bohip_gp* g, int T) { return chol_flags_layout_at(g->dchol_flags, g->dchol_idl, T); }
static CholFlags chol_flags_layout_at(unsigned* base, double* idl, int T) {
    CholFlags fl{};
    fl.T = T;
    fl.panel = base;
    fl.solved = fl.panel + (size_t)T * CH_PANELS;
    fl.crit = fl.solved + T;
    fl.rest = fl.crit + T;
    fl.col = fl.rest + T;
    fl.farall = fl.col + T;
    fl.fol = fl.farall + T;
    fl.colall = fl.fol + T;
    fl.colr = fl.colall + T;
    fl.xp = fl.colr + (size_t)T * T;
    fl.abort = fl.xp + (size_t)T * T * CH_PANELS;
    fl.xp3 = base + chol_xp3_word(T);
    fl.pre3 = fl.xp3 + (size_t)T * CH_PANELS;
    fl.w16_g = idl;
    fl.spin_ticks = g_chol_spin_ticks;
    fl.crit_want = 16u;   // the row-(k+2) update: 4 workgroups x 4 storing waves
    fl.panel_want = 3u;   // three publishing waves per panel
    return fl;
}

// ---- A2, executor form (kernels_exec.hip): the chain + ONE persistent kernel that pulls tile tasks from six in-order queues
// (four feed the factorisation's pivot chain, two grow W = L^-1 behind it).
// The records are a pure function of (buffer addresses, ld, T): built on the host at the first factorisation with this T,
// then resident.  Layout of the counters inside the flag area (all zeroed per factorisation):
//   tile (i, c), i >= c+2:  ver = xp[((c-1) T + i) 8 + 0], pver = xp[.. + 1]   (the chain uses xp[(k T + i) 8 + p] for i = k+1, k+2 only)
//   tile (c+1, c):          ver = farall[c], pver = fol[c];      tile (c, c):  ver = colall[c], pver = col[c]
//   sver(i, k) = colr[k T + i];   queue cursors = the EX_NQ = 6 words behind the abort word
static void exec_task_list(double* dL, double* dS, double* dW, double* dWT, unsigned* flag_base, int64_t ld, int T, int CH_NSF, int inv_g,
                           std::vector<ExTask>& all, int* qbeg, int inv_grp_min = -1) {
    if (inv_grp_min < 0) inv_grp_min = g_chol_inv_grp_min;   // (the test hook passes its own: no process-wide state is swapped)
    const CholFlags fl = chol_flags_layout_at(flag_base, nullptr, T);
    auto widx = [&](const unsigned* p) { return (uint32_t)(p - flag_base); };
    auto nb = [](int c) { return std::max(c / 4 - 1, 0); };         // bulk groups that touch column c
    auto ks = [](int c) { return 4 * std::max(c / 4 - 1, 0); };     // first block of column c's window (= 4 nb)
    auto ver = [&](int i, int c) {
        return i >= c + 2 ? widx(fl.xp + ((size_t)(c - 1) * T + i) * CH_PANELS) : (i == c + 1 ? widx(fl.farall + c) : widx(fl.colall + c));
    };
    auto pver = [&](int i, int c) {
        return i >= c + 2 ? widx(fl.xp + ((size_t)(c - 1) * T + i) * CH_PANELS + 1) : (i == c + 1 ? widx(fl.fol + c) : widx(fl.col + c));
    };
    auto sver = [&](int i, int k) { return widx(fl.colr + (size_t)k * T + i); };
    auto Sp = [&](int i, int kb) { return dS + (int64_t)i * TILE * ld + (int64_t)kb * TILE; };
    auto Ap = [&](int i, int c) { return dL + (int64_t)i * TILE * ld + (int64_t)c * TILE; };
    // P(i, c): the mirror tile of the scratch matrix (its upper triangle and diagonal tiles are free during the factorisation)
    auto Pp = [&](int i, int c) { return dS + (int64_t)c * TILE * ld + (int64_t)i * TILE; };
    // last block the Early sum of tile (i, c) contains; Late adds the two blocks behind it
    // (the three tiles of a row that the chain kernel finishes itself -- i <= c + 2 -- get their last block from its gated updates:
    // the executor's share ends one block earlier)
    auto e_of = [](int i, int c) { return i <= c + 2 ? i - 6 : c - 3; };
    std::vector<ExTask> q[EX_NQ];
    {   // (rough upper bounds: growing the vectors record by record was a third of the 32 ms this takes at T = 79)
        const size_t t1 = (size_t)T, t2 = t1 * t1, t3 = t2 * t1;
        const size_t cap[EX_NQ] = {32 * t1, 4 * t2, 2 * t2, 6 * t2 + 64, t3 / 10 + t2 + 64, inv_g > 0 ? t3 / (2 * (size_t)inv_g) + t2 + 64 : 0};
        for (int qi = 0; qi < EX_NQ; ++qi) q[qi].reserve(cap[qi]);
    }
    struct Dep { uint32_t idx, want; };
    auto add = [&](int qi, const double* A, const double* B, double* C, const double* P, int kc_h0, int kc_h1, bool diag, int rmw,
                   std::initializer_list<Dep> deps, uint32_t s0, uint32_t s1, int kc_split = 0, Dep d2a = Dep{EX_NONE, 0},
                   Dep d2b = Dep{EX_NONE, 0}) {
        for (int h = 0; h < 2; ++h) {
            ExTask t{};
            t.A = A; t.B = B + (int64_t)h * CTILE * ld; t.C = C + h * CTILE; t.P = P ? P + h * CTILE : nullptr;
            int nd = 0;
            for (int d = 0; d < EX_NDEP; ++d) { t.dep_idx[d] = EX_NONE; t.dep_want[d] = 0; }
            for (const Dep& d : deps) {
                if (d.idx == EX_NONE || d.want == 0) continue;
                t.dep_idx[nd] = d.idx; t.dep_want[nd] = d.want; ++nd;
            }
            t.sig_idx[0] = s0; t.sig_idx[1] = s1;
            t.kc = h == 0 ? kc_h0 : kc_h1; t.diag_h = diag ? h : -1; t.rmw = rmw; t.prio = qi <= 1 ? 2 : (qi == 2 ? 1 : 0);
            t.kc_split = kc_split;
            t.dep2_idx[0] = d2a.idx; t.dep2_want[0] = d2a.want; t.dep2_idx[1] = d2b.idx; t.dep2_want[1] = d2b.want;
            q[qi].push_back(t);
        }
    };
    const int CPB = TILE / KC;   // contraction chunks per 128-block
    for (int k = 0; k + 3 < T; ++k) {
        // Solve(i, k) = A(i, k) W_kk'  (W_kk lower-triangular: the left half of the columns needs the first 64 contraction indices only)
        const double* Wkk = dW + (int64_t)k * TILE * (ld + 1);
        // The rows k+3 .. k+2+CH_NSF are solved panel by panel inside the chain kernel (solve_follower).  The next NBU rows -- the
        // ones that become follower rows within NBU blocks -- have their row step (Solve, then Late of column k+1) in the URGENT
        // queue: what paces the whole factorisation is the latency pivot k -> inverse -> Solve -> Late of the row that enters the
        // follower window next (chain period ~ 69 us + that latency - ~29 us), and in the ordinary queue that row's two steps wait
        // for a free workgroup twice and run beside bulk work.  Everything further out is queue 1.
        const int NBU = g_chol_exec_nbu, rb = k + 3 + CH_NSF;   // first row solved by the executor
        auto solve_row = [&](int qi, int i) {
            add(qi, Ap(i, k), Wkk, Sp(i, k), nullptr, CPB / 2, CPB, false, 0,
                {{widx(fl.solved + k), 1u}, {k >= 1 ? ver(i, k) : EX_NONE, 16u * (unsigned)(nb(k) + 1)}}, sver(i, k), EX_NONE);
        };
        // Late(k): blocks max(k-1, 0) .. k into the tiles read next
        const int kb0 = std::max(k - 1, 0);
        auto late = [&](int qi, int i, int c, uint32_t sig2) {
            const bool has_p = e_of(i, c) >= ks(c);
            auto chain_row = [&](int kk, int r) { return Dep{widx(fl.xp + ((size_t)kk * T + r) * CH_PANELS + (CH_PANELS - 1)), 1u}; };
            const Dep p_dep{has_p ? pver(i, c) : EX_NONE, 16u}, v_dep{ver(i, c), 16u * (unsigned)nb(c)};
            // (a diagonal tile whose bulk groups already reach block k-1 -- c = k+4 a multiple of 4 -- gets block k only)
            const int kb = (i == c && ks(c) >= k) ? k : kb0, kcl = (k - kb + 1) * CPB;
            if (kb < k) {
                // TWO PIECES: the block k-1 half of the contraction needs nothing of block k, so the task is claimed and starts before
                // S(i, k) exists -- for the follower rows while block k is still being factored, for the others while their row
                // solve is running -- and waits for S(i, k) (and the chain's row c) inside, half a contraction from its end
                const Dep b_prev = c == k + 1 ? chain_row(k - 1, c) : Dep{sver(c, k - 1), 16u};
                add(qi, Sp(i, kb), Sp(c, kb), Ap(i, c), has_p ? Pp(i, c) : nullptr, kcl, kcl, i == c, 1,
                    {{sver(i, k - 1), 16u}, b_prev, p_dep, v_dep}, ver(i, c), sig2, CPB,
                    Dep{sver(i, k), 16u}, c <= k + 2 ? chain_row(k, c) : (c != i ? Dep{sver(c, k), 16u} : Dep{EX_NONE, 0}));
                return;
            }
            // one block, one piece.  rows of S on the B side: row c of block k
            const Dep b0 = c <= k + 2 ? chain_row(k, c) : Dep{sver(c, k), 16u};
            add(qi, Sp(i, kb), Sp(c, kb), Ap(i, c), has_p ? Pp(i, c) : nullptr, kcl, kcl, i == c, 1,
                {{sver(i, k), 16u}, b0, p_dep, v_dep}, ver(i, c), sig2);
        };
        // urgent, in the order they are needed: the tiles the chain's solve followers read in block k+1, then the three tiles of row
        // k+4 that its gated updates finish during block k+1 (pre3; the blocks up to k: one block of slack), then the row steps of
        // the rows about to enter the follower window
        for (int i = k + 4; i < std::min(T, rb); ++i) late(0, i, k + 1, EX_NONE);
        if (k + 4 < T)
            for (int j = 0; j < 3; ++j) late(0, k + 4, k + 2 + j, widx(fl.pre3 + 4 * (k + 1) + j));
        for (int i = rb; i < std::min(T, rb + NBU); ++i) solve_row(0, i);
        for (int i = rb; i < std::min(T, rb + NBU); ++i) late(0, i, k + 1, EX_NONE);
        for (int i = rb + NBU; i < T; ++i) solve_row(1, i);
        for (int i = rb + NBU; i < T; ++i) late(1, i, k + 1, EX_NONE);
    }
    for (int kp = 0; kp + 5 < T; ++kp) {
        // Early(kp): P(i, c) = sum_{b = ks(c)}^{kp} S(i, b) S(c, b)'  for the tiles Late(kp + 2) finishes
        auto early = [&](int i, int c) {
            if (i >= T || c >= T || ks(c) > kp) return;
            const int nbk = kp - ks(c) + 1;   // blocks in the sum: 1 ... 5, growing with c inside a group of four columns
            if (T <= (inv_g == 0 ? 56 : 23) && nbk >= 2) {
                // (round 6) TWO PIECES like Late: the blocks before kp need nothing of block kp, so the task starts a block earlier and waits for
                // S(i, kp) / S(c, kp) inside, one K = 128 piece from its end.  In one piece it started only when the LAST block's rows were solved and
                // then ran its whole window -- up to 50 us on the path S(i, kp) -> Early -> Late -> follower, growing over every group of four columns:
                // the drift behind the owner's 30-50 us waits for crit[k-2] at every fourth block (profiles/r06_exec_trace_N3000.txt).
                // The factorisation ALONE up to 56 row tiles: N=3000 1.14 -> 1.09-1.11 ms, N=3500 1.37 -> 1.31, N=6000 3.03 -> 2.90; N=8000 the same,
                // N=10^4 9.0 -> 9.2 (a waiting task holds a workgroup the bulk work could use); with the inverse queues the same at N <= 3000 and
                // worse beyond (N=4000 2.00 -> 2.05, N=10^4 13.65 -> 14.15): one piece there; up to 23 row tiles two pieces with them too
                // (N=1600 0.64 -> 0.615 ms, N=2000 0.78 -> 0.76, N=2300 0.93 -> 0.90, N=2800 1.147 -> 1.114).
                add(2, Sp(i, ks(c)), Sp(c, ks(c)), const_cast<double*>(Pp(i, c)), nullptr, nbk * CPB, nbk * CPB, i == c, 0,
                    {{sver(i, kp - 1), 16u}, {sver(c, kp - 1), 16u}}, pver(i, c), EX_NONE, (nbk - 1) * CPB, Dep{sver(i, kp), 16u},
                    c != i ? Dep{sver(c, kp), 16u} : Dep{EX_NONE, 0});
                return;
            }
            add(2, Sp(i, ks(c)), Sp(c, ks(c)), const_cast<double*>(Pp(i, c)), nullptr, nbk * CPB,
                nbk * CPB, i == c, 0, {{sver(i, kp), 16u}, {sver(c, kp), 16u}}, pver(i, c), EX_NONE);
        };
        early(kp + 6, kp + 4);   // the three tiles of row kp+6: blocks up to kp (e_of), then Late(kp+2) adds two, the chain the last
        early(kp + 6, kp + 5);
        early(kp + 6, kp + 6);
        for (int i = kp + 6; i < T; ++i) early(i, kp + 3);
    }
    auto add_bulk = [&](int m, int c, int i) {
        add(EX_QBULK, Sp(i, 4 * m), Sp(c, 4 * m), Ap(i, c), nullptr, 4 * CPB, 4 * CPB, i == c, 1,
            {{sver(i, 4 * m + 3), 16u}, {sver(c, 4 * m + 3), 16u}, {ver(i, c), 16u * (unsigned)m}}, ver(i, c), EX_NONE);
    };
    // group after group, column-major inside a group
    for (int m = 0; 4 * m + 8 <= T - 1; ++m)
        for (int c = 4 * m + 8; c < T; ++c)
            for (int i = c; i < T; ++i) add_bulk(m, c, i);
    // Queues 3 (EX_QROWS) and 5 (EX_QWAVE): W = L^-1 behind the chain (inv_g > 0: blocks per piece of the long contraction = chunk size G).
    //   Z(i, j) = -sum_{k=j}^{i-1} L(i, k) W(k, j)   accumulated in place at W(i, j), in k order, from three kinds of pieces:
    //       wave m     chunk m = blocks [G m, G (m+1)), pushed to EVERY row i >= G (m+1) + 1 as soon as the chunk's rows of W are
    //                  final (right-looking: queue 5, lowest priority -- thousands of independent K = 128 G tasks per wave)
    //       partial    what is left of row i's own chunk, [G m_i, i-1), m_i = (i-1) / G
    //       last       {i-1}: the only piece that needs row i-1 of W; it also stores Z' to the mirror tile (j, i) of W
    //   W(i, j) = W_ii Z(i, j)                        A = W_ii, B = Z' (K-major), result to W(i, j) and transposed to W'(j, i)
    // partial, last and the product form the row-to-row chain (queue 3, ABOVE the bulk updates: per row one K = 128 task + the product,
    // little work but serial -- starved behind the bulk it started when the bulk ended and the waves with it;
    // in ONE queue with the waves every row waited behind a whole wave).  Counters, 4 words per tile behind the queue cursors:
    // [0] zver = rounds on Z (16 each), [1] zt = Z' complete, [2] wfin.  Everything a record waits for is earlier in its queue, in
    // another queue or the chain's; nothing outside these two queues ever waits for them.
    // GROUP FORM of the two inverse queues (T >= g_chol_inv_grp_min).  Above, every row of W waits for the row before it: last(i) needs
    // W(i-1, j), product(i) needs last(i) -- two dependent K = 128 records per row, ~117 us under load, T - 1 rows one after the other.  At
    // N = 10^4 that chain IS the second half of the refit: starved behind the bulk until ~7 ms, then 67 rows x 117 us = 7.8 ms during which
    // the waves fill in but the end is the chain's (profiles/r04_exec_trace_N10000.txt).  Here the rows of a GROUP of G blocks do not wait
    // for each other.  With g0 = G g the first block of group g and D_g = L_gg^-1 the group's own triangular block of W:
    //   D_g                      by the row chain above, restricted to the columns j >= g0 (queue 3: at most G - 1 short row steps, right
    //                            behind the pivots, nothing else waits inside them)
    //   P(i, j) = -sum_{k=j}^{g0-1} L(i, k) W(k, j),  j < g0      the waves as above, one round per earlier group m (blocks of group m, pushed
    //                            to every later row as soon as group m's rows of W are final); the round of group g-1 completes P and
    //                            also stores P' to the mirror tile (j, i)
    //   W(i, j) = sum_{k=g0}^{i} W(i, k) P(k, j)                  ONE record per tile half, K = 128 (i - g0 + 1): A = row i of D_g (K-major in W),
    //                            B = the mirror tiles (j, g0 .. i)
    // so the serial part is one K = 128 G round + one product per GROUP (~250 us per G rows instead of ~117 us per row), and what runs last
    // is a full-width product, not a row chain.  Queue 5 order: rounds of group m for the rows of group m+1 first, then the first half of the
    // far rows, then the products of group m+1 (their inputs were claimed a thousand records earlier), then the other half (which separates
    // the products from the rounds of group m+1 that need them).  Counters: word 3 of tile (g0, j) counts the completed P' tiles of group g
    // and column j, word 2 of the same tile its finished products, word 3 of the diagonal tile (g0, g0) the finished tiles of D_g.
    const bool inv_groups = inv_g >= 2 && T >= inv_grp_min;   // (a group of one row has no D_g: nothing would mark W as grown)
    if (inv_groups) {
        const int G = inv_g, NG = (T + G - 1) / G;
        const uint32_t ivb = (uint32_t)chol_inv_word(T);
        auto iw = [&](int i, int j, int w) { return ivb + (uint32_t)(((size_t)i * T + j) * 4 + w); };
        auto chain_row = [&](int kk, int r) { return Dep{widx(fl.xp + ((size_t)kk * T + r) * CH_PANELS + (CH_PANELS - 1)), 1u}; };
        auto l_final = [&](int i, int k) { return i <= k + 2 ? chain_row(k, i) : Dep{sver(i, k), 16u}; };
        auto w_final = [&](int k, int j) { return k > j ? Dep{iw(k, j, 2), 16u} : Dep{widx(fl.solved + j), 1u}; };   // inside a group
        auto add_inv = [&](int qi, const double* A, const double* B, double* C, double* CTb, int kc, int mode, std::initializer_list<Dep> deps,
                           uint32_t s0, uint32_t s1) {
            for (int h = 0; h < 2; ++h) {
                ExTask t{};
                t.A = A; t.B = B + (int64_t)h * CTILE * ld; t.C = C + h * CTILE; t.P = CTb ? CTb + (int64_t)h * CTILE * ld : nullptr;
                int nd = 0;
                for (int d = 0; d < EX_NDEP; ++d) { t.dep_idx[d] = EX_NONE; t.dep_want[d] = 0; }
                for (const Dep& d : deps) {
                    if (d.idx == EX_NONE || d.want == 0) continue;
                    t.dep_idx[nd] = d.idx; t.dep_want[nd] = d.want; ++nd;
                }
                t.sig_idx[0] = s0; t.sig_idx[1] = s1;
                t.kc = kc; t.diag_h = -1; t.rmw = mode | (CTb ? 4 : 0); t.prio = 0; t.kc_split = 0;
                t.dep2_idx[0] = t.dep2_idx[1] = EX_NONE;
                q[qi].push_back(t);
            }
        };
        auto Wp = [&](int i, int j) { return dW + (int64_t)i * TILE * ld + (int64_t)j * TILE; };
        auto WTp = [&](int j, int i) { return dWT + (int64_t)j * TILE * ld + (int64_t)i * TILE; };
        auto rows_of = [&](int g) { return std::min(G, T - G * g); };
        auto tiles_of = [&](int g) { const int r = rows_of(g); return r * (r - 1) / 2; };
        auto GP = [&](int g, int j) { return iw(G * g, j, 3); };
        auto GW = [&](int g, int j) { return iw(G * g, j, 2); };
        auto GD = [&](int g) { return iw(G * g, G * g, 3); };
        // D_g: row i's tiles j = g0 .. i-1 -- what is below row i-1 in one piece (needs row i-2), then {i-1}, then the product.
        // Z(i, j) is summed in the scratch matrix's mirror tile (free since Late consumed its Early sum, long before row i was solved), NOT
        // in place: the products below read the tiles of D_g through LDS-DMA, and a tile that was written THREE times by workgroups on
        // different XCDs (Z, Z, then W) is served stale from the reader's L2 every now and then -- nothing else in these queues reads a
        // location that is written more than once (first version: 1 % errors in W at N = 3000 whenever eight refits shared the device).
        auto Zp = [&](int i, int j) { return const_cast<double*>(Pp(i, j)); };
        auto d_partial = [&](int i) {
            if (i >= T) return;
            const int g0 = G * (i / G);
            for (int j = g0; j < i - 1; ++j)
                add_inv(EX_QROWS, Sp(i, j), WTp(j, j), Zp(i, j), nullptr, (i - 1 - j) * CPB, 2, {l_final(i, i - 2), w_final(i - 2, j)}, iw(i, j, 0), EX_NONE);
        };
        auto d_last = [&](int i) {
            const int g0 = G * (i / G);
            for (int j = g0; j < i; ++j) {
                const bool hp = j < i - 1;
                add_inv(EX_QROWS, Sp(i, i - 1), WTp(j, i - 1), Zp(i, j), Wp(j, i), CPB, hp ? 1 : 2,
                        {l_final(i, i - 1), w_final(i - 1, j), Dep{hp ? iw(i, j, 0) : EX_NONE, 16u}}, iw(i, j, 0), iw(i, j, 1));
            }
        };
        auto d_product = [&](int i) {
            const int g = i / G, g0 = G * g;
            for (int j = g0; j < i; ++j)
                add_inv(EX_QROWS, Wp(i, i), Wp(j, i), Wp(i, j), WTp(j, i), CPB, 0, {Dep{iw(i, j, 1), 16u}, Dep{widx(fl.solved + i), 1u}}, iw(i, j, 2), GD(g));
        };
        for (int i = 1; i < T; ++i) {
            if ((i + 1) / G == i / G) d_partial(i + 1);
            if (i % G != 0) { d_last(i); d_product(i); }
        }
        // one round: the blocks of group m into P(i, j)
        auto round = [&](int m, int i, int j) {
            const int g = i / G, m0 = G * m, m1 = G * (m + 1), a = std::max(j, m0), nbf = j >= m0 ? 0 : m - j / G;
            const bool fin = m == g - 1;
            const Dep src = j < m0 ? Dep{GW(m, j), 16u * (unsigned)rows_of(m)} : Dep{GD(m), 16u * (unsigned)tiles_of(m)};
            add_inv(EX_QWAVE, Sp(i, a), WTp(j, a), Wp(i, j), fin ? Wp(j, i) : nullptr, (m1 - a) * CPB, nbf == 0 ? 2 : 1,
                    {l_final(i, m1 - 1), src, Dep{widx(fl.solved + m1 - 1), 1u}, Dep{nbf ? iw(i, j, 0) : EX_NONE, 16u * (unsigned)nbf}},
                    iw(i, j, 0), fin ? GP(g, j) : EX_NONE);
        };
        auto products = [&](int g) {
            const int g0 = G * g, r = rows_of(g);
            for (int i = g0; i < g0 + r; ++i)
                for (int j = 0; j < g0; ++j)
                    add_inv(EX_QWAVE, Wp(i, g0), Wp(j, g0), Wp(i, j), WTp(j, i), (i - g0 + 1) * CPB, 0,
                            {Dep{GP(g, j), 16u * (unsigned)r}, Dep{GD(g), 16u * (unsigned)tiles_of(g)}, Dep{widx(fl.solved + g0 + r - 1), 1u}}, GW(g, j), EX_NONE);
        };
        for (int m = 0; m + 1 < NG; ++m) {
            const int m1 = G * (m + 1), near_end = std::min(T, m1 + G), far_mid = near_end + (T - near_end + 1) / 2;
            for (int i = m1; i < near_end; ++i)
                for (int j = 0; j < m1; ++j) round(m, i, j);
            for (int i = near_end; i < far_mid; ++i)
                for (int j = 0; j < m1; ++j) round(m, i, j);
            products(m + 1);
            for (int i = far_mid; i < T; ++i)
                for (int j = 0; j < m1; ++j) round(m, i, j);
        }
    } else if (inv_g > 0) {
        const int G = inv_g;
        const uint32_t ivb = (uint32_t)chol_inv_word(T);
        auto iw = [&](int i, int j, int w) { return ivb + (uint32_t)(((size_t)i * T + j) * 4 + w); };
        auto chain_row = [&](int kk, int r) { return Dep{widx(fl.xp + ((size_t)kk * T + r) * CH_PANELS + (CH_PANELS - 1)), 1u}; };
        auto l_final = [&](int i, int k) {   // row i of L complete up to block k (rows are solved in block order)
            return i <= k + 2 ? chain_row(k, i) : Dep{sver(i, k), 16u};
        };
        auto w_final = [&](int k, int j) { return k > j ? Dep{iw(k, j, 2), 16u} : Dep{widx(fl.solved + j), 1u}; };   // W(k, j); the diagonal tile is the inverter's
        auto add_inv = [&](int qi, const double* A, const double* B, double* C, double* CTb, int kc, int mode, std::initializer_list<Dep> deps,
                           uint32_t s0, uint32_t s1) {
            for (int h = 0; h < 2; ++h) {
                ExTask t{};
                t.A = A; t.B = B + (int64_t)h * CTILE * ld; t.C = C + h * CTILE; t.P = CTb ? CTb + (int64_t)h * CTILE * ld : nullptr;
                int nd = 0;
                for (int d = 0; d < EX_NDEP; ++d) { t.dep_idx[d] = EX_NONE; t.dep_want[d] = 0; }
                for (const Dep& d : deps) {
                    if (d.idx == EX_NONE || d.want == 0) continue;
                    t.dep_idx[nd] = d.idx; t.dep_want[nd] = d.want; ++nd;
                }
                t.sig_idx[0] = s0; t.sig_idx[1] = s1;
                t.kc = kc; t.diag_h = -1; t.rmw = mode | (CTb ? 4 : 0); t.prio = 0; t.kc_split = 0;
                t.dep2_idx[0] = t.dep2_idx[1] = EX_NONE;
                q[qi].push_back(t);
            }
        };
        auto Wp = [&](int i, int j) { return dW + (int64_t)i * TILE * ld + (int64_t)j * TILE; };
        auto WTp = [&](int j, int i) { return dWT + (int64_t)j * TILE * ld + (int64_t)i * TILE; };
        auto m_of = [&](int i) { return (i - 1) / G; };                                       // row i's own (incomplete) chunk
        auto n_waves = [&](int i, int j) { return std::max(0, m_of(i) - j / G); };           // wave pieces tile (i, j) receives
        // what is left of row i's own chunk before its last block goes in two pieces, so that none of them has less than two rows
        // of slack behind the product it waits for: A = [G m_i, i-2) (needs row i-3 of W), B = {i-2} (row i-2).  (One piece
        // [G m_i, i-1): up to G-1 blocks of contraction, ~100 us at G = 8, between the products of two consecutive rows -- the
        // rows fell behind the pivots by that much every G rows.)
        auto has_a = [&](int i, int j) { return std::max(j, G * m_of(i)) < i - 2; };
        auto has_b = [&](int i, int j) { return i - 2 >= G * m_of(i) && j <= i - 2; };
        auto zdep = [&](int i, int j, int n) { return Dep{n ? iw(i, j, 0) : EX_NONE, 16u * (unsigned)n}; };
        auto wave = [&](int m) {   // after the product of row G (m+1) - 1
            const int k1 = G * (m + 1);
            for (int i = k1 + 1; i < T; ++i)
                for (int j = 0; j < k1; ++j) {
                    const int a = std::max(j, G * m), nbf = j >= G * m ? 0 : m - j / G;
                    add_inv(EX_QWAVE, Sp(i, a), WTp(j, a), Wp(i, j), nullptr, (k1 - a) * CPB, nbf == 0 ? 2 : 1,
                            {l_final(i, k1 - 1), w_final(k1 - 1, j), zdep(i, j, nbf)}, iw(i, j, 0), EX_NONE);
                }
        };
        auto partial_a = [&](int i) {
            if (i >= T || i < 3) return;
            for (int j = 0; j < i - 2; ++j) {
                if (!has_a(i, j)) continue;
                const int a = std::max(j, G * m_of(i)), nbf = n_waves(i, j);
                add_inv(EX_QROWS, Sp(i, a), WTp(j, a), Wp(i, j), nullptr, (i - 2 - a) * CPB, nbf == 0 ? 2 : 1,
                        {l_final(i, i - 3), w_final(i - 3, j), zdep(i, j, nbf)}, iw(i, j, 0), EX_NONE);
            }
        };
        auto partial_b = [&](int i) {
            if (i >= T || i < 2) return;
            for (int j = 0; j <= i - 2; ++j) {
                if (!has_b(i, j)) continue;
                const int nbf = n_waves(i, j) + (has_a(i, j) ? 1 : 0);
                add_inv(EX_QROWS, Sp(i, i - 2), WTp(j, i - 2), Wp(i, j), nullptr, CPB, nbf == 0 ? 2 : 1,
                        {l_final(i, i - 2), w_final(i - 2, j), zdep(i, j, nbf)}, iw(i, j, 0), EX_NONE);
            }
        };
        auto last = [&](int i) {
            for (int j = 0; j < i; ++j) {
                const int nbf = n_waves(i, j) + (has_a(i, j) ? 1 : 0) + (has_b(i, j) ? 1 : 0);
                add_inv(EX_QROWS, Sp(i, i - 1), WTp(j, i - 1), Wp(i, j), Wp(j, i), CPB, nbf == 0 ? 2 : 1,
                        {l_final(i, i - 1), w_final(i - 1, j), zdep(i, j, nbf)}, iw(i, j, 0), iw(i, j, 1));
            }
        };
        auto product = [&](int i) {
            for (int j = 0; j < i; ++j)
                add_inv(EX_QROWS, Wp(i, i), Wp(j, i), Wp(i, j), WTp(j, i), CPB, 0, {Dep{iw(i, j, 1), 16u}, Dep{widx(fl.solved + i), 1u}}, iw(i, j, 2), EX_NONE);
        };
        for (int i = 1; i < T; ++i) {   // what follows needs the product of row i-1 at most, except product(i): pivot i
            partial_a(i + 2);
            partial_b(i + 1);
            last(i);
            product(i);
            if ((i + 1) % G == 0) wave((i + 1) / G - 1);
        }
    }
    all.clear();
    {
        size_t total = 0;
        for (int qi = 0; qi < EX_NQ; ++qi) total += q[qi].size();
        all.reserve(total);
    }
    qbeg[0] = 0;
    for (int qi = 0; qi < EX_NQ; ++qi) {
        all.insert(all.end(), q[qi].begin(), q[qi].end());
        qbeg[qi + 1] = (int)all.size();
    }
}
// May the bulk queue be claimed `stride` records at a time?  A claim starts when ALL its records' counters are in and runs them back to back,
// and claims are the consecutive blocks of `stride` records from the queue's start (one fetch-and-add each) -- so no record of a block may wait
// for another record of the SAME block: that claim would wait for itself.  In the bulk queue that is two rounds on one tile next to each other,
// which happens where a group has a single tile left (T = 4 m + 9: the last round of the last diagonal tile directly behind the round before).
static bool exec_bulk_stride_ok(const std::vector<ExTask>& all, const int* qbeg, int stride) {
    for (int b = qbeg[EX_QBULK]; b < qbeg[EX_QBULK + 1]; b += stride) {
        const int e = std::min(b + stride, qbeg[EX_QBULK + 1]);
        for (int x = b; x < e; ++x)
            for (int y = x + 1; y < e; ++y)
                if (all[x].C == all[y].C) return false;
    }
    return true;
}
static int build_exec_tasks(bohip_gp* g, int T) {
    if (g->ex_T == T && g->dex_tasks && g->ex_nsf == g_chol_nsf && g->ex_inv_g == g_chol_inv_g && g->ex_grp_min == g_chol_inv_grp_min) return 0;
    std::vector<ExTask> all;
    exec_task_list(g->dL, g->dS, g->dW, g->dWT, g->dchol_flags, g->ld, T, g_chol_nsf, g_chol_inv_g, all, g->ex_qbeg);
    HIPCHK(g->dex_tasks.reserve(all.size(), g->stream));
    HIPCHK(hipMemcpyAsync(g->dex_tasks, all.data(), all.size() * sizeof(ExTask), hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));   // `all` is pageable host memory that dies with this frame
    g->ex_bulk4_ok = exec_bulk_stride_ok(all, g->ex_qbeg, 4);
    g->ex_T = T;
    g->ex_nsf = g_chol_nsf;
    g->ex_inv_g = g_chol_inv_g;
    g->ex_grp_min = g_chol_inv_grp_min;
    return 0;
}

static std::mutex g_df_mutex[64];   // per device: see refit_once
// ... and the same between PROCESSES that share a device (two ranks on one GPU in the sharded bench's test mode, several BO loops per GPU): an
// advisory file lock named after the device's PCI address, taken inside the host lock and released with it (the kernel drops it if the process
// dies).  Round 5 (advisor): the lock file lives in a PER-USER directory ($XDG_RUNTIME_DIR, else /tmp/bohip-<uid> created 0700 and checked to be
// ours), is opened O_NOFOLLOW | O_CLOEXEC with mode 0600 and never chmod'ed (a planted symlink or file cannot redirect it); the lock is taken
// NON-blocking with a bounded retry (BOHIP_DF_FILE_LOCK=n: n ms, 300 by default) -- a stopped or hung holder no longer blocks every refit on the GPU: the
// refit then goes ahead unlocked and the flags' 200 ms time-out + launch-chain fall-back stay the safety net; the descriptor is re-opened in a
// forked child (parent and child would share ONE open file description and not exclude each other).  No lock file (read-only directory,
// BOHIP_DF_FILE_LOCK=0): the refit goes ahead as before.  Processes of DIFFERENT users on one device do not see each other's lock.
struct DfFileLock {
    int fd = -1;
    static int open_lock_file(int device) {
        char bus[64] = "dev";
        if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) snprintf(bus, sizeof bus, "dev%d", device);
        for (char* c = bus; *c; ++c) if (*c == ':' || *c == '.' || *c == '/') *c = '_';
        char dir[128];
        const char* xdg = getenv("XDG_RUNTIME_DIR");
        struct stat st;
        if (xdg && xdg[0] == '/' && strlen(xdg) < 100 && stat(xdg, &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == geteuid()) {
            snprintf(dir, sizeof dir, "%s", xdg);
        } else {
            snprintf(dir, sizeof dir, "/tmp/bohip-%u", (unsigned)geteuid());
            if (mkdir(dir, 0700) != 0 && errno != EEXIST) return -1;
            if (lstat(dir, &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != geteuid() || (st.st_mode & 077)) return -1;   // not ours / a link / open to others
        }
        char path[256];
        snprintf(path, sizeof path, "%s/bohip_refit_%s.lock", dir, bus);
        return open(path, O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0600);
    }
    bool contended = false;   // another process held the lock for the whole wait: this refit takes the launch-chained form (nothing in it spins)
    DfFileLock() = default;
    // T: row tiles of the refit -- the wait covers a dozen refits of this size by the other process (300 ms up to ~50 row tiles, T^2 / 8 ms beyond)
    void acquire(int device, int T) {
        // BOHIP_DF_FILE_LOCK: 0 = off, 1 = on with the default wait, n > 1 = on, waiting up to n ms for the other process
        static int setting = [] { const char* e = getenv("BOHIP_DF_FILE_LOCK"); return e ? std::max(0, atoi(e)) : 1; }();
        const int enabled = setting != 0, wait_ms = setting > 1 ? setting : std::max(300, T * T / 8);
        if (!enabled) return;
        static int fds[64];
        static pid_t owner[64];
        static std::mutex open_mutex;
        const int dv = device & 63;
        {
            std::lock_guard<std::mutex> lk(open_mutex);
            const pid_t me = getpid();
            if (owner[dv] != me) {                        // first use in this process, or we are a forked child: an own open file description
                if (owner[dv] != 0 && fds[dv] >= 0) close(fds[dv]);
                fds[dv] = open_lock_file(device);
                owner[dv] = me;
            }
            fd = fds[dv];
        }
        if (fd < 0) return;                               // no lock file (directory not ours, ...): unlocked, the time-out fall-back is the safety net
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            if (flock(fd, LOCK_EX | LOCK_NB) == 0) return;
            if (errno != EWOULDBLOCK && errno != EINTR) break;
            if (std::chrono::steady_clock::now() - t0 >= std::chrono::milliseconds(wait_ms)) { contended = true; break; }
            usleep(200);
        }
        fd = -1;
    }
    void release() { if (fd >= 0) { flock(fd, LOCK_UN); fd = -1; } }
    ~DfFileLock() { release(); }
};
static int device_cus();
static int cholesky_exec(bohip_gp* g, int T) {
    const int64_t ld = g->ld;
    CHK(build_exec_tasks(g, T));
    CholFlags fl = chol_flags_layout(g, T);
    HIPCHK(hipMemsetAsync(g->dchol_flags, 0, chol_flag_words(T) * sizeof(unsigned), g->stream));
    HIPCHK(hipEventRecord(g->ev_panels, g->stream));           // K and the cleared flags are in place
    fl.nsf = g_chol_nsf;
    hipLaunchKernelGGL(k_chol_chain, dim3(9 + g_chol_nsf + 6), dim3(CH_THREADS), CH_LDS_BYTES, g->stream, g->dL, ld, g->dS, T, fl, g->dinfo, g->dW, g->dWT);
    HIPCHK(hipGetLastError());
    // The solved panels go home (S -> L) right behind the CHAIN kernel, not behind the executor: every S(i, k) feeds the diagonal tile of its
    // row, so all of them are final -- and the tiles of L they replace have been read for the last time -- when the last pivot is done, while the
    // executor still has the second half of W = L^-1 to grow (N = 10^4: 4.4 ms).  The copy runs beside that on the CUs the chain has left.
    hipLaunchKernelGGL(k_copy_offdiag_tiles, dim3(T * (T - 1) / 2), dim3(256), 0, g->stream, g->dS, g->dL, ld, T);
    HIPCHK(hipGetLastError());
    if (T > 3 || g->ex_qbeg[EX_NQ] > 0) {   // (T = 2, 3: no factorisation task, but the inverse's rows)
        ExQueues q{};
        q.tasks = g->dex_tasks;
        for (int i = 0; i <= EX_NQ; ++i) q.qbeg[i] = g->ex_qbeg[i];
        q.flags = g->dchol_flags;
        q.abort = g->dchol_flags + chol_abort_word(T);
        q.heads = q.abort + 1;
        q.ld = ld;
        q.spin_ticks = g_chol_spin_ticks;
        // executor workgroups: two per CU that the chain kernel leaves free (a small partition must not fill its slots with the
        // urgent queue's own workgroups: nobody would serve the other queues until the time-out)
        const int cus_free = std::max(1, device_cus() - (9 + g_chol_nsf + 6));
        // How many: two per CU share the CU's matrix pipe -- more throughput (N = 10^4: 14.5 against 15.6 ms for the bare task list), but every
        // task takes ~1.6x as long beside a busy neighbour, and at chain-paced sizes that is what the pivot chain waits for (the row steps
        // Solve -> Late of the rows about to enter its window): with ONE workgroup per CU the refit at N = 3000 takes 1.43 instead of 1.61 ms,
        // N = 4000 2.13 instead of 2.38; from N = 6000 on two per CU win (4.55 against 5.2).  Swept at T = 8 ... 47
        // (profiles/r04_exec_workgroups_by_size.txt): 1 per CU up to 32 row tiles, 2 from 45 on, linear in between.
        const double per_cu = T <= 32 ? 1.0 : (T >= 45 ? 2.0 : 1.0 + (T - 32) / 13.0);
        const int exec_wgs = std::max(2, g_chol_exec_wgs > 0 ? std::min(g_chol_exec_wgs, 2 * cus_free) : (int)(per_cu * cus_free + 0.5));
        q.nurgent = std::max(1, std::min(exec_wgs / 8, g_chol_exec_urgent > 0 ? g_chol_exec_urgent : (T >= 56 ? 16 : 32)));   // queue 0 is served by these only: never zero
        q.second_from = g_chol_exec_second && exec_wgs > cus_free ? cus_free : 0;
        // (idling the 32 second workgroups that are dispatched as the urgent workgroups' CU mates was measured: the lost throughput costs more,
        // N = 8000 8.85 against 8.60 ms, N = 10^4 alone 9.4 against 9.1)
        // (with one workgroup per CU nobody slows a neighbour down and the reserve buys nothing: 1.43 ms at N = 3000 with 0, 30 or 59 of them)
        // (36 more workgroups than fit beside the chain -- they start on its 18 CUs when it has ended, at N = 10^4 with 6 ms still to go --
        // were measured: 15.4-15.6 ms either way.  What ran last then was the inverse's row chain, not a lack of workgroups.)
        q.nfast = std::max(0, std::min(exec_wgs / 4, g_chol_exec_fast >= 0 ? g_chol_exec_fast : (T <= 48 && per_cu > 1.0 ? (int)(112 * (per_cu - 1.0)) : 0)));
        int pairs_ = g_chol_exec_pairs >= 0 ? g_chol_exec_pairs : (T >= 72 ? 2 : 1);
        if (pairs_ >= 2 && !(pairs_ == 2 && g->ex_bulk4_ok)) pairs_ = 1;   // (more than two tiles per claim: never checked, never faster)
        q.stride[0] = 1; q.stride[1] = 1; q.stride[2] = pairs_ ? 2 : 1; q.stride[EX_QBULK] = pairs_ >= 2 ? 2 * std::min(pairs_, 4) : (pairs_ ? 2 : 1);
        q.stride[EX_QROWS] = q.stride[EX_QWAVE] = g_chol_exec_inv_pairs ? 2 : 1;
        q.fill_inv = g_chol_exec_fill_inv;
        q.patience_ticks = (unsigned)g_chol_exec_patience_us * 100u;
        HIPCHK(hipStreamWaitEvent(g->col_stream, g->ev_panels, 0));
        // (Holding this launch back until the chain's workgroups are resident -- hipStreamWaitValue32 on a word they count themselves into:
        // the kernel then starts ~10 us behind them -- was built against the time-outs of refits that share the device with other host
        // threads' work: it cost 0.1 ms at N = 10^4 and the time-outs stayed.  What causes those is streams of several handles sharing a
        // hardware queue, where a kernel waits for the END of the one before it; the per-device lock in refit_once removed most of them.)
        hipLaunchKernelGGL(k_chol_exec, dim3(exec_wgs), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), g->col_stream, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(g->ev_inv, g->col_stream));
        HIPCHK(hipStreamWaitEvent(g->stream, g->ev_inv, 0));
    }
    g->w_done = g->ex_qbeg[EX_QROWS + 1] > g->ex_qbeg[EX_QROWS];
    return 0;
}

// multiprocessors of the current device (the dataflow form needs its persistent workgroups resident at the same time)
static int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    int& c = cus[dev & 63];
    if (c == 0 && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c = 0;
    return c;
}
// The launch-chained factorisation as a stage of its own: the matrix, its scratch and the 128 x 128 diagonal inverses are a workspace,
// so that the same code factorises the model's cK (refit_once) and a matrix the model does not own (the joint sampler's Sigma).
// Streams and events are the handle's.
struct FactorWs {
    double *L, *S, *W, *WT;     // ld x ld matrix (lower tiles) and panel scratch; diagonal inverses W_kk at W + k wstep, W_kk' at WT + k wstep
    int64_t ld, ldw, wstep;
    int* info;
};
static FactorWs model_factor_ws(bohip_gp* g) {
    return FactorWs{g->dL, g->dS, g->dW, g->dWT, g->ld, g->ld, (int64_t)TILE * (g->ld + 1), g->dinfo};
}
static int factor_launch_chain(bohip_gp* g, const FactorWs& ws, int T) {
    const int64_t ld = ws.ld;
    // Right-looking on 128-column panels, with the trailing update applied in two tiers: inside an outer block
    // of OB panels only the block's own remaining columns are updated after every panel (K = 128); everything to
    // the right of the outer block is updated ONCE per outer block with K = 128 * OB.  The C tiles of the bulk
    // are therefore read-modified-written T/OB times instead of T times and the bulk contraction is OB x deeper.
    const int OB = 4;
    bool side_pending = false;
    // The bulk update of the columns right of the NEXT block runs on the side stream.  Run as one launch it shares the chip
    // with the next block's whole diagonal chain and slows the chain's small GEMMs 3-6x (N = 10^4: 90-120 us instead of
    // 15-25 us each).  So it is cut into pieces of equal area, and piece j is released by an event recorded just before the
    // j-th diagonal-block kernel of the next block starts: the pieces fill the ~70 us during which that single-workgroup
    // kernel leaves the chip idle and are (mostly) gone when the chain's GEMMs arrive.
    struct Pending { int ob = 0, oe = 0, c0 = 0, rest = 0, next = 0, pieces = 0; int cut[9] = {0}; } pend;
    auto bulk_params = [&](int pob, int poe, int r0t, int c0t, int mt, int nct) {
        GemmNTParams b{};  // A[i, j] -= L[i, pob:poe] L[j, pob:poe]'  on rows >= r0t, columns [c0t, c0t + nct)
        b.A = ws.S + (int64_t)r0t * TILE * ld + (int64_t)pob * TILE; b.lda = ld;
        b.B = ws.S + (int64_t)c0t * TILE * ld + (int64_t)pob * TILE; b.ldb = ld;
        b.C = ws.L + (int64_t)r0t * TILE * ld + (int64_t)c0t * TILE; b.ldc = ld;
        b.mt = mt; b.nt64 = 2 * nct; b.kc = (poe - pob) * (TILE / KC); b.alpha = -1.0; b.beta = 1.0;
        b.diag_skip = 1; b.row0 = (int64_t)r0t * TILE; b.col0 = (int64_t)c0t * TILE;
        return b;
    };
    auto release_piece = [&](bool gated) -> int {   // next piece of the pending bulk update -> side stream
        if (pend.next >= pend.pieces) return 0;
        if (gated) {
            HIPCHK(hipEventRecord(g->ev_gate, g->stream));
            HIPCHK(hipStreamWaitEvent(g->side_stream, g->ev_gate, 0));
        }
        const int a = pend.cut[pend.next], b = pend.cut[pend.next + 1];
        ++pend.next;
        if (b > a)   // columns [c0 + a, c0 + b) of the pending region, rows from the first of them down
            CHK(launch_gemm_nt(g, bulk_params(pend.ob, pend.oe, pend.c0 + a, pend.c0 + a, pend.rest - a, b - a), 1, g->side_stream));
        if (pend.next == pend.pieces) HIPCHK(hipEventRecord(g->ev_bulk, g->side_stream));
        return 0;
    };
    for (int ob = 0; ob < T; ob += OB) {
        const int oe = std::min(T, ob + OB);
        for (int kb = ob; kb < oe; ++kb) {
            double* Lkk = ws.L + (int64_t)kb * TILE * (ld + 1);
            double* Wkk = ws.W + (int64_t)kb * ws.wstep;
            CHK(release_piece(true));
            hipLaunchKernelGGL(k_potf2_inv, dim3(1), dim3(PF_THREADS), POTF2_LDS_BYTES, g->stream, Lkk, ld, Wkk,
                               ws.WT + (int64_t)kb * ws.wstep, ws.ldw, ws.info, kb * TILE);
            HIPCHK(hipGetLastError());
            const int rem = T - kb - 1;
            if (rem == 0) break;
            const int64_t poff = (int64_t)(kb + 1) * TILE * ld + (int64_t)kb * TILE;
            double* panel = ws.S + poff;  // solved panel L[kb+1:, kb] lives in the scratch matrix until the final copy
            GemmNTParams p{};  // panel solve L[i,kb] = A[i,kb] * inv(L_kk)'   (out of place: dL -> dS)
            p.A = ws.L + poff; p.lda = ld; p.B = Wkk; p.ldb = ws.ldw; p.C = panel; p.ldc = ld;
            p.mt = rem; p.nt64 = 2; p.kc = TILE / KC; p.alpha = 1.0; p.beta = 0.0;
            CHK(launch_gemm_nt(g, p));
            const int inner_cols = oe - kb - 1;  // remaining panels of this outer block
            if (inner_cols > 0) {
                GemmNTParams u{};  // A[i, j] -= L[i,kb] L[j,kb]'  for j in (kb, oe), i >= j
                u.A = panel; u.lda = ld; u.B = panel; u.ldb = ld;
                u.C = ws.L + (int64_t)(kb + 1) * TILE * (ld + 1); u.ldc = ld;
                u.mt = rem; u.nt64 = 2 * inner_cols; u.kc = TILE / KC; u.alpha = -1.0; u.beta = 1.0;
                u.diag_skip = 1; u.row0 = (int64_t)(kb + 1) * TILE; u.col0 = (int64_t)(kb + 1) * TILE;
                CHK(launch_gemm_nt(g, u));
            }
        }
        while (pend.next < pend.pieces) CHK(release_piece(false));   // a short last block: whatever is left goes now
        const int rem = T - oe;
        if (rem > 0) {
            // Bulk update with the OB solved panels: the columns of the NEXT outer block on the critical stream, everything
            // to their right in gated pieces on the side stream.  Hazards: (1) the side stream needs the panels -> ev_panels;
            // (2) the next block's columns were last written by the previous block's pieces -> ev_bulk (after the last one).
            const int nxt = std::min(OB, rem), rest = rem - nxt;
            if (rest > 0) {
                HIPCHK(hipEventRecord(g->ev_panels, g->stream));
                HIPCHK(hipStreamWaitEvent(g->side_stream, g->ev_panels, 0));
            }
            if (side_pending) HIPCHK(hipStreamWaitEvent(g->stream, g->ev_bulk, 0));
            CHK(launch_gemm_nt(g, bulk_params(ob, oe, oe, oe, rem, nxt)));
            if (rest > 0) {
                pend = Pending{};
                pend.ob = ob; pend.oe = oe; pend.c0 = oe + nxt; pend.rest = rest; pend.next = 0;
                pend.pieces = g_bulk_pieces > 0 ? std::min({g_bulk_pieces, nxt, rest}) : 1;
                // equal-area cuts of the lower-triangular region: the area left of column c is c rest - c (c - 1) / 2
                const double total = 0.5 * rest * (rest + 1.0);
                for (int q = 0, c = 0; q <= pend.pieces; ++q) {
                    const double want = total * q / pend.pieces;
                    while (c < rest && c * (double)rest - 0.5 * c * (c - 1.0) < want - 1e-9) ++c;
                    pend.cut[q] = q == pend.pieces ? rest : c;
                }
                if (pend.pieces == 1) CHK(release_piece(false));   // ungated single launch (small problems, BOHIP_BULK_PIECES=0)
                side_pending = true;
            } else {
                side_pending = false;
            }
        }
    }
    if (side_pending) HIPCHK(hipStreamWaitEvent(g->stream, g->ev_bulk, 0));
    if (T > 1) {
        hipLaunchKernelGGL(k_copy_offdiag_tiles, dim3(T * (T - 1) / 2), dim3(256), 0, g->stream, ws.S, ws.L, ld, T);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

static int refit_once(bohip_gp* g, double jitter);
// Full rebuild.  A factorisation that fails (BOHIP_E_NOTPD) is reported as such unless jitter escalation was asked for
// (bohip_gp_set_jitter / BOHIP_JITTER): then the diagonal gets jitter_rel x mean(diag) more, x10 per further try -- the shape
// of GaussianProcesses.jl's make_posdef! (UPSTREAM-UNVERIFIED, hence off by default; oracle twin: oracle.py fit_with_jitter).
static int refit(bohip_gp* g) {
    g->jitter_steps_last = 0;
    g->jitter_last = 0.0;
    int rc = refit_once(g, 0.0);
    if (rc != BOHIP_E_NOTPD || g->jitter_tries <= 0 || !(g->jitter_rel > 0.0)) return rc;
    const double mean_diag = std::exp(2.0 * g->logsig) + std::exp(2.0 * g->lognoise);   // stationary kernels: every diagonal entry
    double jit = g->jitter_rel * mean_diag;
    for (int t = 1; t <= g->jitter_tries; ++t, jit *= 10.0) {
        rc = refit_once(g, jit);
        if (rc != BOHIP_E_NOTPD) {
            if (rc == 0) { g->jitter_steps_last = t; g->jitter_last = jit; }
            return rc;
        }
    }
    return rc;
}
static int refit_once(bohip_gp* g, double jitter) {
    CHK(one_time_kernel_setup());
    const int64_t N = g->n;
    if (N == 0) {
        g->stale = false;
        g->n_factored = 0;
        return 0;
    }
    const int64_t Npad = round_up(N + 1, TILE), ld = g->ld;
    const int T = (int)(Npad / TILE);
    const KernelHyper hp = make_hyper(g);
    const double noise = std::exp(2.0 * g->lognoise) + std::numeric_limits<double>::epsilon() + jitter;
    if (g->mirror_dirty) {   // a staged append failed after the mirrors advanced: the host copies are the truth
        HIPCHK(hipMemcpyAsync(g->dX, g->hX.data(), (size_t)N * g->d * 8, hipMemcpyHostToDevice, g->stream));
        HIPCHK(hipMemcpyAsync(g->dy, g->hy.data(), (size_t)N * 8, hipMemcpyHostToDevice, g->stream));
        if (g->weighted) CHK(upload_site_weights(g));
        HIPCHK(hipStreamSynchronize(g->stream));
        g->mirror_dirty = false;
    }
    HIPCHK(hipMemsetAsync(g->dinfo, 0, sizeof(int), g->stream));
    t_begin(g, "build_cov");
    {
        const int rpb = 32;
        dim3 grid((Npad + 255) / 256, (Npad + rpb - 1) / rpb);
        dispatch_dt(g->d, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            LAUNCH_FAM(fam_low(hp), (k_build_cov<DT, true>), (k_build_cov<DT, false>), grid, dim3(256), 0, g->stream, g->dX, N, Npad, hp, noise,
                       g->dL, ld, rpb);
        });
    }
    HIPCHK(hipGetLastError());
    t_end(g);
    if (g->weighted) {   // replicated sites: cK_w = K + noise diag(1 / r_i), the jitter of this try included
        t_begin(g, "rep_diag");
        hipLaunchKernelGGL(k_rep_diag, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, g->stream, g->dL, ld, (int64_t)0, N, hp.sigma2, noise,
                           g->dinvr);
        HIPCHK(hipGetLastError());
        t_end(g);
    }
    // Which form.  The executor makes progress only while the chain kernel's workgroups (9 + solve followers + 6 gated updaters) are
    // resident TOGETHER, one per CU (they fill the LDS), with CUs left over for the executor's own: on a device or partition that
    // cannot hold them the launch chain is used.  T range: from TWO row tiles on with the inverse queues -- at T = 2, 3 the executor has
    // no factorisation task at all (every tile is inside the chain kernel's window) but it grows W = L^-1 behind the chain: N = 200 0.15
    // instead of 0.21 ms, N = 300 0.20 instead of 0.28 -- and from FOUR without them, the first T with a factorisation task.
    const int cus = device_cus();
    const bool exec_ok = T >= (g_chol_inv_g > 0 ? 2 : 4) && cus >= 9 + g_chol_nsf + 6 + 8;
    const bool df_size = g_chol_df != 0 && exec_ok && T <= g_chol_df_tmax;
    bool paused = false;
    if (df_size)   // the pause after a time-out counts refits that WOULD have used a dataflow form, nothing else
        for (int sk = g_chol_df_skip.load(std::memory_order_relaxed); sk > 0;)
            if (g_chol_df_skip.compare_exchange_weak(sk, sk - 1, std::memory_order_relaxed)) { paused = true; break; }
    const bool want_df = !paused && df_size;
    // (stage name: with the executor's inverse queues the factorisation and W = L^-1 are ONE stage)
    // One dataflow refit per device at a time (see below): the host lock of this process and the file lock between processes, taken before
    // the stage begins.  Round 6: when ANOTHER PROCESS keeps the file lock for the whole wait this refit takes the launch-chained form instead
    // of going ahead unlocked (two processes' persistent kernels on one chip are what the 200 ms time-outs of profiles/r06_soak.txt are made of).
    std::unique_lock<std::mutex> df_lock;
    DfFileLock df_file;
    bool df_go = want_df;
    if (df_go) {
        df_lock = std::unique_lock<std::mutex>(g_df_mutex[g->device & 63]);
        df_file.acquire(g->device, T);
        if (df_file.contended) {
            df_go = false;
            df_lock.unlock();
            g->chol_lock_skips++;
        }
    }
    t_begin(g, df_go && g_chol_inv_g > 0 ? "cholesky+inverse" : "cholesky");
    if (df_go) {
        // One dataflow refit per device at a time: its persistent workgroups must be resident together, and two refits from two host threads
        // (several models on one GPU, the logical shards of bohip_mgp_*) take each other's CUs -- every other one then sat out its 200 ms
        // time-out and fell back (tools/w_stress.py: 6 time-outs in 64 refits on 8 threads).  The refit is synchronous anyway (the abort word is
        // read back below), so a host lock from the first launch to that read costs nothing a contended chip would not have cost.
        g->w_done = false;
        g->chol_form_last = 4;
        CHK(cholesky_exec(g, T));
        t_end(g);
        if (!g->w_done) {   // (without the inverse queues: the chain's inverter has left the diagonal blocks W_kk, the levels follow)
            t_begin(g, "tri_inverse");
            for (int h = 1; h < T; h *= 2) CHK(inverse_level(g, g->stream, 0, T, h));
            t_end(g);
        }
        t_begin(g, "alpha");
        CHK(compute_alpha(g));
        t_end(g);
        // the abort word and the pivot word come back through the pinned block behind the kernels: ONE host round trip per refit (three before:
        // this synchronisation, a blocking copy of the abort word, check_info's copy + synchronisation -- ~25 us of a 1.5 ms refit)
        unsigned aborted = 0;
        int* const pwords = g->pin.words;   // (null without the pinned block)
        if (pwords) {
            HIPCHK(hipMemcpyAsync(pwords, g->dchol_flags + chol_abort_word(T), sizeof(unsigned), hipMemcpyDeviceToHost, g->stream));
            HIPCHK(hipMemcpyAsync(pwords + 1, g->dinfo, sizeof(int), hipMemcpyDeviceToHost, g->stream));
        }
        HIPCHK(hipStreamSynchronize(g->stream));
        if (pwords) aborted = (unsigned)pwords[0];
        else HIPCHK(hipMemcpy(&aborted, g->dchol_flags + chol_abort_word(T), sizeof(unsigned), hipMemcpyDeviceToHost));
        df_file.release();
        df_lock.unlock();
        if (aborted) {
            // a flag never arrived (e.g. two of the streams share a hardware queue on this system, or a spinning launch kept a
            // persistent workgroup off the chip): every wait has returned, nothing hangs; the factor -- and any pivot failure it
            // reports, hence this check BEFORE check_info -- is garbage.  Fall back to the launch-chained form for the rest of
            // the process (BOHIP_CHOL_DF_STRICT=1: report it instead, for tests and tools).
            g->chol_fallbacks++;
            g->chol_abort_T = T;
            {
                // the chain kernel's waits leave the word address of the flag that never arrived (bit 31 set); the executor's tasks leave 1
                char which[96] = "counters of an executor task";
                if (aborted & 0x80000000u) {
                    const unsigned base_w = (unsigned)(reinterpret_cast<uintptr_t>(g->dchol_flags.get()) >> 2) | 0x80000000u;
                    snprintf(which, sizeof which, "flag word %u of %zu", (aborted - base_w) & 0x7fffffffu, chol_flag_words(T));
                }
                fprintf(stderr, "libbohip: dataflow factorisation (form %d, %d row tiles) timed out on a dependency (%s); using the launch-chained form for a while\n",
                        g->chol_form_last, T, which);
            }
            if (g_chol_df_dump) {   // diagnosis: which flags of the dataflow form never arrived
                std::vector<unsigned> hf(chol_flag_words(T));
                hipMemcpy(hf.data(), g->dchol_flags, hf.size() * sizeof(unsigned), hipMemcpyDeviceToHost);
                const CholFlags fl = chol_flags_layout(g, T);
                auto at = [&](const unsigned* p) { return hf[(size_t)(p - g->dchol_flags)]; };
                fprintf(stderr, "  abort word 0x%x, words behind it:", aborted);
                for (int w_ = 1; w_ < 8; ++w_) fprintf(stderr, " %u", hf[chol_abort_word(T) + w_]);
                fprintf(stderr, "\n");
                for (int k = 0; k < T; ++k) {
                    fprintf(stderr, "  block %2d: panel", k);
                    for (int p = 0; p < CH_PANELS; ++p) fprintf(stderr, " %u", at(fl.panel + k * CH_PANELS + p));
                    fprintf(stderr, " | crit %u rest %u col %u farall %u colall %u | rows with xp[7] unset:", at(fl.crit + k), at(fl.rest + k), at(fl.col + k), at(fl.farall + k), at(fl.colall + k));
                    for (int i = k + 1; i < T; ++i) {
                        const unsigned* x = fl.xp + ((size_t)k * T + i) * CH_PANELS;
                        if (at(x + CH_PANELS - 1) == 0u) { int p0 = 0; while (p0 < CH_PANELS && at(x + p0) != 0u) ++p0; fprintf(stderr, " %d(p%d)", i, p0); }
                    }
                    fprintf(stderr, " | colr<8:");
                    for (int i = k + 2; i < T; ++i) if (at(fl.colr + (size_t)k * T + i) < 8u) fprintf(stderr, " %d(%u)", i, at(fl.colr + (size_t)k * T + i));
                    fprintf(stderr, "\n");
                }
            }
            if (g_chol_df_strict) return fail(BOHIP_E_HIP, "dataflow factorisation timed out on a dependency (BOHIP_CHOL_DF_STRICT)");
            {
                const int bo = std::min(1024, 2 * g_chol_df_backoff.load(std::memory_order_relaxed) + 8);
                g_chol_df_backoff.store(bo, std::memory_order_relaxed);
                g_chol_df_skip.store(bo + 1, std::memory_order_relaxed);   // (+1: the repeat of this very refit)
            }
            g->stale = true;
            return refit_once(g, jitter);
        }
        if (pwords) {
            if (pwords[1] != 0) {
                g->pivot = pwords[1];
                g->stale = true;
                return fail(BOHIP_E_NOTPD, "kernel matrix not positive definite at pivot " + std::to_string(pwords[1]));
            }
            g->pivot = 0;
        } else {
            CHK(check_info(g));
        }
        g->stale = false;
        g->n_factored = N;
        g->refits++;
        // a dataflow refit went through: the next time-out starts from half the pause (one transient episode late in a long
        // process must not cost 1024 refits on the slow form)
        for (int bo = g_chol_df_backoff.load(std::memory_order_relaxed); bo > 0;)
            if (g_chol_df_backoff.compare_exchange_weak(bo, bo / 2, std::memory_order_relaxed)) break;
        return 0;
    }
    g->chol_form_last = 0;
    CHK(factor_launch_chain(g, model_factor_ws(g), T));
    t_end(g);
    t_begin(g, "tri_inverse");
    for (int h = 1; h < T; h *= 2) CHK(inverse_level(g, g->stream, 0, T, h));   // recursive doubling over the whole matrix after the factorisation
    t_end(g);
    t_begin(g, "alpha");
    CHK(compute_alpha(g));
    t_end(g);
    CHK(check_info(g));
    g->stale = false;
    g->n_factored = N;
    g->refits++;
    return 0;
}

// out[r][j] = (W rows[r])[j] for r < P <= 32: one launch, workgroups of 8 rows of W x 8 right-hand sides
static int launch_rows_trimv(bohip_gp* g, const double* W, int64_t N0, const double* rows, int P, double* out, int upper) {
    if (N0 <= 0 || P <= 0) return 0;
    // one workgroup per CU walks its share of the 8-row blocks of W (k_trimv_stream, kernels_linalg.hip); 16 right-hand sides per pass
    const int64_t nblk = (N0 + 7) / 8;
    const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::max(device_cus(), 1), nblk));
    hipLaunchKernelGGL(k_trimv_stream<TRIMV_D>, dim3(wgs, (unsigned)((P + 15) / 16)), dim3(TRIMV_THREADS), trimv_lds_bytes(TRIMV_D), g->stream,
                       W, g->ld, N0, rows, g->ld, P, out, g->ld, upper, (const unsigned*)nullptr);   // (no go word: never part of an ascent pass)
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- A2': incremental extension by p new observations (already in dX/dy and the host mirror) ----------
// defer_info != nullptr: the pivot word is copied there (pinned) behind the kernels and looked at by the caller after ITS synchronisation
// (one host round trip less per append)
static int append_incremental(bohip_gp* g, int64_t N0, int64_t p, int* defer_info = nullptr) {
    CHK(one_time_kernel_setup());
    const int64_t N1 = N0 + p, Npad1 = round_up(N1 + 1, TILE), ld = g->ld;
    const KernelHyper hp = make_hyper(g);
    // (a refit that needed jitter J put J on every diagonal entry: the appended rows carry it too, so that the factor
    // stays the factor of ONE matrix -- cK + J I -- that the oracle's fit_with_jitter reproduces)
    const double noise = std::exp(2.0 * g->lognoise) + std::numeric_limits<double>::epsilon() + g->jitter_last;
    HIPCHK(hipMemsetAsync(g->dinfo, 0, sizeof(int), g->stream));
    t_begin(g, "append_cov_rows");
    LAUNCH_FAM(fam_low(hp), k_cov_rows<true>, k_cov_rows<false>, dim3((Npad1 + 255) / 256, Npad1 - N0), dim3(256), 0, g->stream, g->dX,
               N0, N1, Npad1, hp, noise, g->dL, g->dW, g->dWT, ld);
    HIPCHK(hipGetLastError());
    t_end(g);
    if (g->weighted) {   // replicated sites: the new rows' diagonal entries, as refit_once sets them
        t_begin(g, "rep_diag");
        hipLaunchKernelGGL(k_rep_diag, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, g->stream, g->dL, ld, N0, N1, hp.sigma2, noise, g->dinvr);
        HIPCHK(hipGetLastError());
        t_end(g);
    }
    t_begin(g, "append_L21");
    CHK(launch_rows_trimv(g, g->dW, N0, g->dL + N0 * ld, (int)p, g->dApp, 0));
    HIPCHK(hipMemcpy2DAsync(g->dL + N0 * ld, ld * 8, g->dApp, ld * 8, N0 * 8, p, hipMemcpyDeviceToDevice, g->stream));
    t_end(g);
    t_begin(g, "append_schur_chol");
    const double* schur_in = nullptr;
    if (p >= 3) {      // the Schur complement's inner products, one workgroup each (same bits as k_schur_chol's own loop, which p <= 2 keeps: one launch less)
        HIPCHK(g->dschur.reserve((size_t)APPEND_PMAX * APPEND_PMAX, g->stream));
        hipLaunchKernelGGL(k_schur_dots, dim3((unsigned)(p * (p + 1) / 2)), dim3(256), 0, g->stream, g->dL, ld, N0, (int)p, g->dschur);
        schur_in = g->dschur;
    }
    hipLaunchKernelGGL(k_schur_chol, dim3(1), dim3(256), 0, g->stream, g->dL, g->dW, g->dWT, ld, N0, (int)p, g->dinfo, schur_in);
    HIPCHK(hipGetLastError());
    t_end(g);
    t_begin(g, "append_W21");
    double* Tm = g->dApp + (int64_t)APP_UT_ROW0 * ld;   // T = L21 W11, row-wise on W' (k >= c)
    CHK(launch_rows_trimv(g, g->dWT, N0, g->dL + N0 * ld, (int)p, Tm, 1));
    hipLaunchKernelGGL(k_apply_w22, dim3((N0 + 255) / 256), dim3(256), 0, g->stream, g->dW, g->dWT, ld, N0, (int)p, Tm, ld);
    HIPCHK(hipGetLastError());
    t_end(g);
    t_begin(g, "alpha");
    if (g_append_alpha_inc && g->alpha_inc_run < 256) {      // (every 256 appends the full product: the increments' rounding does not accumulate without bound)
        g->alpha_inc_run++;
        // alpha_new = [alpha_old + W21' u2; W22' u2] (kernels_linalg.hip k_alpha_append_*); BOHIP_APPEND_ALPHA_INC=0: the full product
        hipLaunchKernelGGL(k_alpha_append_u, dim3((unsigned)p), dim3(1024), 0, g->stream, g->dW, ld, N0, (int)p, g->dy, g->beta, g->dr, g->dt);
        hipLaunchKernelGGL(k_alpha_append_apply, dim3((unsigned)((N1 + 255) / 256)), dim3(256), 0, g->stream, g->dW, ld, N0, (int)p, g->dt, g->dalpha);
        HIPCHK(hipGetLastError());
    } else {
        CHK(compute_alpha(g));
    }
    t_end(g);
    if (defer_info) HIPCHK(hipMemcpyAsync(defer_info, g->dinfo, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    else CHK(check_info(g));
    g->n_factored = N1;
    g->appends++;
    return 0;
}

static int ensure_fresh(bohip_gp* g) {
    if (g->dL == nullptr || g->cap < g->n) CHK(alloc_model(g, std::max<int64_t>(g->n, 1)));   // a failed growth left no buffers
    if (g->stale || g->n_factored != g->n) return refit(g);
    return 0;
}

// ---- scoring --------------------------------------------------------------------------------------
static int64_t chunk_cap(const bohip_gp* g) {
    // A K*' chunk of about the size of the 256 MB Infinity Cache, in multiples of 512 candidates (8 XCDs x one 64-wide candidate
    // tile: k_trigemm_sq deals candidate tiles to XCDs round-robin).  Rounds 1-3 kept the chunk at 128 MB "so that it stays in the
    // cache next to W"; the sweep of round 4 (tools/chunk_sweep.py, profiles/r04_chunk_sweep.txt) says larger is better up to
    // ~200-330 MB -- fewer launches, each with more jobs per slot and a smaller share of ragged end -- and worse beyond:
    // N = 3000, R = 32768: 4096 per chunk 5.15 ms, 8192: 4.96, 16384: 5.09;  N = 10^4, R = 4096: 1024: 7.28, 2048: 6.49, 4096: 6.43;
    // N = 6000, R = 16384: 4096: 9.32, 8192: 9.42, 16384: 10.1;  N = 1000, R = 65536: 8192: 1.71, 32768: 1.57, 65536: 1.62.
    int64_t rows = (int64_t)(256.0 * 1024 * 1024 / (8.0 * g->ld));
    rows = std::max<int64_t>(1024, std::min<int64_t>(65536, rows / 512 * 512));
    return rows;
}
// Chunks of ONE batch are equal-sized multiples of 512 candidates: R = 32768 at N = 3000 is 8 x 4096, not 6 x 5376 + 512
// (a ragged last chunk is a launch with a few candidate tiles per XCD -- all tail; measured 5.39 against 5.08 ms).  Among the
// chunk counts that fit the cap the one that leaves the least padding wins, fewer chunks on a tie.
static int64_t chunk_rows(const bohip_gp* g, int64_t R) {
    if (g_chunk_rows_forced > 0) return std::min<int64_t>(round_up(std::max<int64_t>(R, 1), TILE), round_up(g_chunk_rows_forced, TILE));
    const int64_t cap = chunk_cap(g), R512 = round_up(std::max<int64_t>(R, 1), 512);
    if (R512 <= cap) return round_up(std::max<int64_t>(R, 1), TILE);   // one chunk (its buffer keeps the 128-row granularity)
    const int64_t nmin = (R512 + cap - 1) / cap;
    int64_t best_rows = cap, best_pad = INT64_MAX;
    for (int64_t n = nmin; n <= nmin + 4; ++n) {
        const int64_t rows = round_up((R512 + n - 1) / n, 512), pad = n * rows - R512;
        if (rows <= cap && pad < best_pad) { best_pad = pad; best_rows = rows; }
    }
    return best_rows;
}
static int ensure_score_scratch(bohip_gp* g, int64_t R) {
    const int64_t Rpad = round_up(std::max<int64_t>(R, 1), TILE);
    const int64_t T = g->ld / TILE;
    const int64_t rc = chunk_rows(g, R);
    g->score_chunk = rc;
    const int64_t SLACK = TILE;  // head-room so tile-granular writes past the last candidate stay inside the buffers
    const hipStream_t st = g->stream;
    bool grew = false;
    HIPCHK(g->dKsT.reserve((size_t)(rc + SLACK) * g->ld, st, Grow::Exact, &grew));
    if (grew) g->kst_rows = rc;
    HIPCHK(g->dq.reserve((size_t)(2 * T * (Rpad + SLACK)), st));   // two partial sums per row tile (k_trigemm_sq's row pieces)
    HIPCHK(g->dmu_raw.reserve((size_t)(Rpad + SLACK), st));
    for (DBuf<double>* b : {&g->dmu, &g->dvar, &g->dscore}) HIPCHK(b->reserve((size_t)Rpad, st));
    const int64_t tiles = Rpad / CTILE + 2;
    grew = false;
    HIPCHK(g->dfz_best.reserve((size_t)tiles, st));
    HIPCHK(g->dfz_cnt.reserve((size_t)(tiles + 1 + 16), st, Grow::Exact, &grew));   // + the job cursors of k_trigemm_sq_pull
    if (grew) {
        HIPCHK(hipMemsetAsync(g->dfz_cnt, 0, (size_t)(tiles + 1 + 16) * sizeof(unsigned), st));
        g->fz_tiles = tiles;
    }
    HIPCHK(g->dblock_best.reserve((size_t)((R + 255) / 256 + 1), st));
    return 0;
}
static int ensure_grad_scratch(bohip_gp* g) {
    const size_t n = (size_t)g->kst_rows * g->ld;
    bool grew = false;
    HIPCHK(g->dVT.reserve(n, g->stream, Grow::Exact, &grew));
    HIPCHK(g->dUT.reserve(n, g->stream));
    if (grew) HIPCHK(hipMemsetAsync(g->dVT, 0, n * 8, g->stream));  // padding columns (>= N) must stay zero
    return 0;
}
static int ensure_xs(bohip_gp* g, int64_t R) {
    HIPCHK(g->dXs.reserve(std::max<size_t>(1, (size_t)R * g->d), g->stream));
    return 0;
}

// ---- the plan of a posterior pass: values made once per pass and handed down, never left on the handle --------------------------
// The sizes every launch of a pass is written in.  Rpad: one tile of head-room for tile-granular writes (dq's leading dimension).
struct PassDims { int64_t N, Npad, R, Rpad, ld; int T; };
static int row_tiles(const bohip_gp* g) { return (int)(round_up(g->n + 1, TILE) / TILE); }   // T: the observations and the alpha row
static PassDims pass_dims(const bohip_gp* g, int64_t R) {
    const int T = row_tiles(g);
    return PassDims{g->n, (int64_t)T * TILE, R, round_up(R, TILE) + TILE, g->ld, T};
}
struct SplitPlan { int kz = 0, nsl = 0; };
enum class Route { Small, Split, Pruned, WholeK };   // small_pass_mfma, split_posterior, pruned_pass, chunk_pass
struct PassPlan {
    PassDims dm{};
    Route route = Route::WholeK;
    SplitPlan sp;        // Route::Split
    int prune_m = 0;     // Route::Pruned: row tiles of the bounding prefix
    int64_t chunk = 0;   // candidates per K*' chunk (chunk_rows)
    // row tiles behind dq once the pass has run (two partial sums each); 0: dq[r] is the finished sum -- what k_score is told
    int dq_tiles() const { return route == Route::WholeK || route == Route::Pruned ? dm.T : 0; }
};

// kp (the pruned pass): the kernel also leaves the per-wave partial sums of alpha_j K*'_j and of its absolute value (always 16
// candidates per block: the halving reduction is written for 16)
template <int DT>
static void launch_kstar(bohip_gp* g, const double* dXs, int64_t r0, int64_t r1, int64_t Npad, const KernelHyper& hp, const KstarParts* kp) {
    // 16 candidates per block: N/256 x R/16 blocks keep >= 8 waves per SIMD in flight (latency-bound loop); a handful of candidates:
    // two per block (ten in a row on 12 workgroups were a serial chain of ten `exp`s per thread)
    const int rb = r1 - r0 <= 32 && !kp ? 2 : 16;
    dim3 grid((Npad + 255) / 256, (r1 - r0 + rb - 1) / rb);
    if (kp)
        LAUNCH_FAM(fam_low(hp), (k_kstar<DT, true, true>), (k_kstar<DT, false, true>), grid, dim3(256), 0, g->stream, g->dX, g->n, Npad, dXs,
                   r0, r1, hp, g->dKsT, g->ld, rb, *kp);
    else
        LAUNCH_FAM(fam_low(hp), (k_kstar<DT, true>), (k_kstar<DT, false>), grid, dim3(256), 0, g->stream, g->dX, g->n, Npad, dXs, r0, r1, hp,
                   g->dKsT, g->ld, rb, KstarParts{});
}

// The row pieces of k_trigemm_sq (kernels_score.hip), heaviest first: whole row tiles, and a last tile whose live rows fit its
// upper half as a half piece.  A function of the number of row tiles and of where the alpha row sits -- nothing else, so a
// candidate's score does not depend on the batch it is scored in.  (Issuing tiles as two 64-row halves to even out the end of the
// launch was measured in round 4 and gave nothing: profiles/r04_trigemm_halve_sweep.txt, DESIGN.md.)
static void trigemm_pieces(int T, int64_t alpha_row, std::vector<int>& out) {
    struct P { double cost; int code; };
    std::vector<P> ps;
    for (int rt = 0; rt < T; ++rt) {
        const int64_t live = alpha_row + 1 - (int64_t)rt * TILE;   // live rows of this tile (the last one: up to the alpha row)
        if (live <= TILE / 2) ps.push_back({(rt + 0.5) / 2.0, rt | PIECE_UPPER_SOLO << 16});
        else ps.push_back({rt + 1.0, rt | PIECE_WHOLE << 16});
    }
    std::stable_sort(ps.begin(), ps.end(), [](const P& a, const P& b) { return a.cost > b.cost; });
    out.clear();
    for (const P& q : ps) out.push_back(q.code);
}
static int ensure_pieces(bohip_gp* g, int T, int64_t alpha_row) {
    if (g->pieces_T == T && g->pieces_alpha == alpha_row && g->dpieces) return 0;
    std::vector<int> ps;
    trigemm_pieces(T, alpha_row, ps);
    if (T > 65535) return fail(BOHIP_E_UNSUPPORTED, "too many row tiles");
    if (ps.size() > g->dpieces.capacity()) HIPCHK(g->dpieces.reserve(2 * ps.size() + 64, g->stream));   // (a table of its own rule: twice, and some)
    // (stream-ordered: a launch of an earlier call may still be reading the old table)
    g->hpieces = ps;
    HIPCHK(hipMemcpyAsync(g->dpieces, g->hpieces.data(), ps.size() * sizeof(int), hipMemcpyHostToDevice, g->stream));
    g->n_pieces = (int)ps.size();
    g->pieces_T = T; g->pieces_alpha = alpha_row;
    return 0;
}

static int ensure_clk(bohip_gp* g) {
    bool grew = false;
    HIPCHK(g->dclk.reserve(2, g->stream, Grow::Exact, &grew));
    if (grew) HIPCHK(hipMemsetAsync(g->dclk, 0, 2 * sizeof(unsigned long long), g->stream));
    return 0;
}
// V = W K* with the fused epilogue (k_trigemm_sq): one launch per K*' chunk.
static int launch_trigemm(bohip_gp* g, const PassDims& dm, int64_t r0, int64_t ncand, double* VT, FuseParams fz) {
    const int CT = (int)((ncand + CTILE - 1) / CTILE), n_local = (CT + 7) / 8;
    CHK(ensure_pieces(g, dm.T, dm.N));
    const int NP = g->n_pieces;
    fz.T = dm.T;
    if (g->timing) {   // core clock under the dominant kernel (BOHIP_INFO_KERNEL_CLOCK_MHZ)
        CHK(ensure_clk(g));
        fz.clk = g->dclk;
    }
    hipLaunchKernelGGL(k_trigemm_sq, dim3(8 * n_local * NP), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), g->stream, g->dW, g->ld,
                       g->dKsT, g->ld, g->dpieces, NP, CT, dm.N, g->dq, dm.Rpad, g->dmu_raw, r0, VT, g->ld, fz);
    HIPCHK(hipGetLastError());
    return 0;
}

static int launch_kstar_any(bohip_gp* g, const double* dXs, int64_t r0, int64_t r1, int64_t Npad, const KernelHyper& hp,
                            const KstarParts* kp = nullptr) {
    dispatch_dt(g->d, [&](auto dt) { launch_kstar<decltype(dt)::value>(g, dXs, r0, r1, Npad, hp, kp); });
    HIPCHK(hipGetLastError());
    return 0;
}

static int launch_gemm_u(bohip_gp* g, const PassDims& dm, int CT) {
    GemmNTParams p{};  // U'[r][j] = sum_i V'[r][i] W'[j][i] for the chunk's CT candidate tiles, dVT -> dUT  (B = W' upper-triangular: i >= j)
    p.A = g->dVT; p.lda = dm.ld; p.B = g->dWT; p.ldb = dm.ld; p.C = g->dUT; p.ldc = dm.ld;
    p.mt = CT; p.nt64 = 2 * dm.T; p.kc = dm.T * (TILE / KC); p.alpha = 1.0; p.beta = 0.0; p.klo_from_n = 1;
    return launch_gemm_nt(g, p);
}

// THE chunk loop, every whole-K pass: per chunk of pl.chunk candidates K*' -> k_trigemm_sq (dq's partials, dmu_raw; fz: its fused
// finish) [-> U' = V' W] -> finish(r0, r1).  V' is stored when v.VT is set: chunk-local (row_stride 0: dVT, which want_u needs) or for
// all candidates (chunk r0 at VT + r0 * row_stride: select_batch).  Returns the number of chunks, or the error code (< 0).
struct ChunkV { double* VT = nullptr; int64_t row_stride = 0; };
template <class Finish>
static int64_t chunk_pass(bohip_gp* g, const PassPlan& pl, const double* dXs, const KernelHyper& hp, ChunkV v, bool want_u, const FuseParams& fz, Finish&& finish) {
    const PassDims& dm = pl.dm;
    int64_t chunks = 0;
    for (int64_t r0 = 0; r0 < dm.R; r0 += pl.chunk, ++chunks) {
        const int64_t r1 = std::min(dm.R, r0 + pl.chunk);
        t_begin(g, "kstar");
        CHK(launch_kstar_any(g, dXs, r0, r1, dm.Npad, hp));
        t_end(g);
        t_begin(g, v.VT ? "trigemm_sq+V" : "trigemm_sq");
        CHK(launch_trigemm(g, dm, r0, r1 - r0, v.VT ? v.VT + r0 * v.row_stride : nullptr, fz));
        t_end(g);
        if (want_u) {
            t_begin(g, "gemm_U");
            CHK(launch_gemm_u(g, dm, (int)((r1 - r0 + TILE - 1) / TILE)));
            t_end(g);
        }
        CHK(finish(r0, r1));
    }
    return chunks;
}
static int no_finish(int64_t, int64_t) { return 0; }

// k_grad_finish with the observations split over workgroups: the splits' partial sums and the arrival counter of every candidate
static int ensure_small_counters(bohip_gp* g) {
    bool grew = false;
    HIPCHK(g->dgparts.reserve((size_t)SMALL_MAX * 16 * (2 * DMAX), g->stream));
    HIPCHK(g->dgcount.reserve(SMALL_MAX, g->stream, Grow::Exact, &grew));
    if (grew) HIPCHK(hipMemsetAsync(g->dgcount, 0, SMALL_MAX * sizeof(unsigned), g->stream));
    return 0;
}
static bool split_applicable(const bohip_gp* g);
static int64_t small_limit(const bohip_gp* g) {
    if (g_small_r >= 0) return g_small_r;
    // measured break-even with the MFMA path: whole-K jobs (N=500: > 256, N=3000: ~190, N=10000: ~110); where the split-K
    // form applies it wins earlier (N=1500: ~150, N=3000: ~95, N=10000: ~55)
    // (round 4, k_trimv_stream: the row-wise products take 16 right-hand sides per pass over W, so the break-even moves in steps of 16:
    // N = 1000: ~240, N = 3000: 80, N = 10^4: 32 -- tools/small_limit_sweep.py, profiles/r04_small_limit_sweep.txt)
    // (round 5, kernels_small.hip: 256 at N = 1000, 96 at N = 3000, 32 at N = 10^4 -- profiles/r05_small_limit_sweep.txt)
    if (split_applicable(g)) return std::min<int64_t>(SMALL_MAX, std::max<int64_t>(16, (20 + 260000 / std::max<int64_t>(g->n, 1)) / 16 * 16));
    return std::min<int64_t>(SMALL_MAX, 90 + 300000 / std::max<int64_t>(g->n, 1));
}
// the batch size the path decision is based on (see bohip_gp_set_batch_hint)
static int64_t path_R(const bohip_gp* g, int64_t R) { return std::max(R, g->batch_hint); }
// ---- round 5: the small-batch pass as two MFMA kernels (kernels_small.hip) ------------------------------------------------------------
#ifdef BOHIP_SMALL_TRACE
static unsigned long long* g_small_trace = nullptr;
extern "C" int bohip_debug_small_trace_read(unsigned long long* out) {   // measurement build only (tools/small_pass_trace.py)
    if (!g_small_trace) return -1;
    return hipMemcpy(out, g_small_trace, 8192 * 16 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif
template <int DT, int G>
static void launch_small_pass(bohip_gp* g, const SmallCommon& sc, const SmallCommon& scu, const SmallV& sv, const SmallU* su, const KernelHyper& hp,
                              int npass) {
    const bool lo = fam_low(hp);
    LAUNCH_FAM(lo, (k_small_v<DT, G, true>), (k_small_v<DT, G, false>), dim3((unsigned)sc.ntiles, (unsigned)npass), dim3(SP_THREADS), 0,
               g->stream, sc, sv, hp);
    if (su) {
        if (DT == 64 && su->sv.ap.acq == ACQ_LOGEI)   // (the instantiation of its own: kernels_small.hip k_small_u_logei64)
            LAUNCH_FAM(lo, (k_small_u_logei64<true>), (k_small_u_logei64<false>), dim3((unsigned)sc.ntiles, (unsigned)npass), dim3(SP_THREADS), 0,
                       g->stream, scu, *su, hp);
        else
            LAUNCH_FAM(lo, (k_small_u<DT, G, true>), (k_small_u<DT, G, false>), dim3((unsigned)sc.ntiles, (unsigned)npass), dim3(SP_THREADS), 0,
                       g->stream, scu, *su, hp);
    }
}
template <int DT>
static void launch_small_pass_g(bohip_gp* g, int G, const SmallCommon& sc, const SmallCommon& scu, const SmallV& sv, const SmallU* su,
                                const KernelHyper& hp, int npass) {
    if constexpr (DT <= 16) {     // (the wide-dimension instantiations are compiled for four MFMA groups only: build time)
        if (G == 1) return launch_small_pass<DT, 1>(g, sc, scu, sv, su, hp, npass);
        if (G == 2) return launch_small_pass<DT, 2>(g, sc, scu, sv, su, hp, npass);
        if (G == 3) return launch_small_pass<DT, 3>(g, sc, scu, sv, su, hp, npass);
    }
    launch_small_pass<DT, 4>(g, sc, scu, sv, su, hp, npass);
}
// What a pass of the free-running ascent (bohip_gp_acquire_max) asks of the gradient pass it rides on; empty for everybody else.
struct AscPass {
    const SmallFold* fold = nullptr;   // the ascent step this pass's gradient kernel may run in its last workgroup
    const unsigned* go = nullptr;      // the pass's big kernels return at once when the word is 0 (active start points: the adopt kernel and every step write it)
    bool* folded = nullptr;            // out: set when the step was taken (one pass of <= 16 candidates, d <= 16); else k_asc_step follows
};
// all R <= SMALL_MAX candidates: values (mu, sigma^2, score, arg-max record) and, with d_grad, the gradient of the score
static int small_pass_mfma(bohip_gp* g, const double* dXs, int64_t R, const AcqParams& ap, double* d_mu, double* d_var, double* d_score,
                           Best* d_best, int64_t best_off, double* d_grad, const AscPass& asc = AscPass{}) {
    const int N = (int)g->n, T = (N + TILE - 1) / TILE, P = (int)R, npass = (P + 15) / 16,
              DTm = dispatch_dt(g->d, [](auto dt) { return decltype(dt)::value; });
    // chunks per tile: every tile's partial sums cost one 16-KiB write and one read by the block's finisher, a column block's finisher adds up
    // to ceil(T / m) of them; BOHIP_SMALL_M overrides (tools/small_batch_bench.py sweeps it)
    // (one workgroup of these kernels per CU: all tiles of a pass are resident at once when there are no more tiles than CUs)
    int m = g_small_m;
    if (m <= 0) { const int cus = std::max(device_cus(), 1); for (m = 1; m < T && small_ntiles(T, m) > cus; ++m) {} }
    const int ntiles = small_ntiles(T, m);
    const size_t n_part = (size_t)npass * ntiles * 2048, n_v16 = (size_t)npass * T * 128 * 16, n_rec = (size_t)npass * T * 16,
                 n_g = (size_t)npass * ntiles * 16 * DTm, n_gm = (size_t)npass * T * 16 * DTm;
    layout::SmallWs ws;
    auto lay = [&](const void* base) { return layout::small(base, n_part, n_v16, n_rec, (size_t)npass * 32, SMALL_MAX, n_g, n_gm, &ws); };
    HIPCHK(g->dsm.reserve(lay(nullptr), g->stream, Grow::Quarter));
    lay(g->dsm);
    if (!g->dsm_cnt || T > g->sm_cnt_T) {   // the counters are laid out for 16 row tiles more than the call that grows them
        const int Tc = T + 16;
        // [V counters | U counters]
        const size_t words = 2 * ((size_t)(SMALL_MAX / 16) * (Tc + 1) + 1);
        HIPCHK(g->dsm_cnt.reserve(words, g->stream));
        HIPCHK(hipMemsetAsync(g->dsm_cnt, 0, words * sizeof(unsigned), g->stream));
        g->sm_cnt_T = Tc;
    }
    const KernelHyper hp = make_hyper(g);
    SmallCommon sc{};
    sc.A = g->dWT; sc.ld = g->ld; sc.N = N; sc.T = T; sc.m = m; sc.P = P; sc.part = ws.part; sc.ntiles = ntiles; sc.cnt = g->dsm_cnt;
    sc.X = g->dX; sc.Xs = dXs; sc.alpha = g->dalpha; sc.go = asc.go;
#ifdef BOHIP_SMALL_TRACE
    if (!g_small_trace) { HIPCHK(hipMalloc(&g_small_trace, 8192 * 16 * 8)); }
    HIPCHK(hipMemsetAsync(g_small_trace, 0, 8192 * 16 * 8, g->stream));
    sc.trace = g_small_trace;
#endif
    const size_t cnt_block = (size_t)(SMALL_MAX / 16) * (g->sm_cnt_T + 1) + 1;
    SmallV sv{};
    sv.v16 = ws.v16; sv.qpart = ws.qpart; sv.mupart = ws.mupart;
    sv.fstash = ws.fstash;
    sv.sigma2 = std::exp(2.0 * g->logsig); sv.beta = g->beta; sv.ap = ap;
    sv.mu_out = d_mu; sv.var_out = d_var; sv.score_out = d_score; sv.best_out = d_best; sv.idx_off = (long long)best_off;
    sv.finish = d_grad ? 0 : 1;
    SmallU su{};
    sv.ks16 = ws.ks16;
    su.v16 = sv.v16; su.sv = sv; su.gpart = ws.gpart; su.gmpart = ws.gmpart; su.grad = d_grad;
    if (asc.fold && d_grad && npass == 1 && g->d <= 16 && 16 * ((g->d + 1) / 2) <= SP_THREADS - 128) {
        su.fold = *asc.fold;
        if (asc.folded) *asc.folded = true;
    }
    const SmallU* sup = d_grad ? &su : nullptr;
    SmallCommon scu = sc;       // the U pass: W itself (contraction k >= c), its own partial planes and counters
    scu.A = g->dW; scu.cnt = g->dsm_cnt + cnt_block;
    const int G = (std::min(P, 16) + 3) / 4;
    t_begin(g, d_grad ? "small_V+U" : "small_V");
    dispatch_dt(g->d, [&](auto dt) { launch_small_pass_g<decltype(dt)::value>(g, G, sc, scu, sv, sup, hp, npass); });
    HIPCHK(hipGetLastError());
    t_end(g);
    return 0;
}

// ---- split-K posterior for batches too small to fill the chip with whole-K jobs (see k_split_combine_v) -----------
static bool split_applicable(const bohip_gp* g) {
    return g_split && row_tiles(g) >= 8;   // short K extents gain nothing
}
static SplitPlan split_plan(const bohip_gp* g, int64_t R) {
    SplitPlan sp;
    if (!split_applicable(g)) return sp;
    const int T = pass_dims(g, R).T;
    const int64_t CT64 = (path_R(g, R) + CTILE - 1) / CTILE;
    if (CT64 * T >= 512) return sp;                     // enough whole-K jobs for every workgroup slot
    const int units = std::max(2, (T + 7) / 8);         // 128-wide K units per slice
    int kz = units * (TILE / KC);
    int nsl = (T * (TILE / KC) + kz - 1) / kz;
    const int64_t Rc = round_up(R, TILE);
    while (nsl > 1 && (double)nsl * Rc * g->ld * 8.0 > 256.0 * 1024 * 1024) {   // keep the partial planes below 256 MB
        kz *= 2;
        nsl = (T * (TILE / KC) + kz - 1) / kz;
    }
    if (nsl < 2) return sp;
    sp.kz = kz; sp.nsl = nsl;
    return sp;
}
static int split_posterior(bohip_gp* g, const double* dXs, const PassPlan& pl, bool want_u) {
    CHK(one_time_kernel_setup());
    const SplitPlan& sp = pl.sp;
    const int64_t N = pl.dm.N, Npad = pl.dm.Npad, ld = pl.dm.ld, R = pl.dm.R, Rc = round_up(R, TILE);
    const int T = pl.dm.T;
    const KernelHyper hp = make_hyper(g);
    HIPCHK(g->dsplit.reserve((size_t)sp.nsl * Rc * ld, g->stream));
    if (want_u) CHK(ensure_grad_scratch(g));
    t_begin(g, "kstar");
    CHK(launch_kstar_any(g, dXs, 0, R, Npad, hp));
    t_end(g);
    t_begin(g, "split_V");
    GemmNTParams p{};   // partial V'[r][i] = sum over the slice's k of K*'[r][k] W[i][k]  (A = W row tiles, B = K*')
    p.A = g->dW; p.lda = ld; p.B = g->dKsT; p.ldb = ld; p.C = nullptr; p.CT = g->dsplit; p.ldct = ld;
    p.zA = (int64_t)sp.kz * KC; p.zB = (int64_t)sp.kz * KC; p.zCT = Rc * ld;
    p.mt = T; p.nt64 = (int)((R + CTILE - 1) / CTILE); p.kc = sp.kz; p.alpha = 1.0; p.beta = 0.0;
    p.khi_from_m = 1; p.kz = sp.kz; p.ktot = T * (TILE / KC);
    CHK(launch_gemm_nt(g, p, sp.nsl));
    hipLaunchKernelGGL(k_split_combine_v, dim3((unsigned)R), dim3(256), 0, g->stream, g->dsplit, Rc * ld, ld, sp.kz, N, g->dq,
                       g->dmu_raw, want_u ? g->dVT : nullptr, ld);
    HIPCHK(hipGetLastError());
    t_end(g);
    if (want_u) {
        t_begin(g, "split_U");
        GemmNTParams u{};   // partial U'[r][j] = sum over the slice's i of V'[r][i] W'[j][i]   (B = W' upper-triangular: i >= j)
        u.A = g->dVT; u.lda = ld; u.B = g->dWT; u.ldb = ld; u.C = g->dsplit; u.ldc = ld;
        u.zA = (int64_t)sp.kz * KC; u.zB = (int64_t)sp.kz * KC; u.zC = Rc * ld;
        u.mt = (int)(Rc / TILE); u.nt64 = 2 * T; u.kc = sp.kz; u.alpha = 1.0; u.beta = 0.0;
        u.klo_from_n = 1; u.kz = sp.kz; u.ktot = T * (TILE / KC);
        CHK(launch_gemm_nt(g, u, sp.nsl));
        hipLaunchKernelGGL(k_split_combine_u, dim3((unsigned)R), dim3(256), 0, g->stream, g->dsplit, Rc * ld, ld, sp.kz, sp.nsl, N,
                           g->dUT, ld);
        HIPCHK(hipGetLastError());
        t_end(g);
    }
    return 0;
}

// The posterior of a planned Split or WholeK pass (with want_u also U' in dUT), then finish(r0, r1) per chunk; split-K is one "chunk".
template <class Finish>
static int posterior_then(bohip_gp* g, const PassPlan& pl, const double* dXs, const KernelHyper& hp, bool want_u, Finish&& finish) {
    if (pl.route == Route::Split) {
        CHK(split_posterior(g, dXs, pl, want_u));
        return finish(0, pl.dm.R);
    }
    if (want_u) CHK(ensure_grad_scratch(g));
    const int64_t chunks = chunk_pass(g, pl, dXs, hp, ChunkV{want_u ? g->dVT.get() : nullptr, 0}, want_u, FuseParams{}, finish);
    return chunks < 0 ? (int)chunks : 0;
}

// ---- pruned arg-max: value-only calls (kernels_score.hip, "pruned arg-max") ---------------------------------------------------
constexpr int PRUNE_K1 = 64;          // candidates scored exactly in round 1 (one candidate tile)
constexpr int PRUNE_ROWS_CAP = 256;   // round 2's long form: k_trigemm_rows up to this many candidates, gathered rows + k_trigemm_sq beyond
constexpr int PRUNE_R2_GROUPS = 8;    // round 2's steady form: column groups in the grid (a workgroup loops over g, g + 8, ...)
constexpr int64_t PRUNE_R_MAX = 8192; // k_prune_select is one workgroup holding 8 keys a thread; larger batches keep the full pass
// row tiles of the bounding prefix: a function of T only (never of the batch): the smallest m >= 2 whose triangle holds >= 2 % of
// the contraction's, 0 (no pruning) when that leaves no row tile after it
static int prune_tiles(int T) {
    if (g_prune_m >= 0) return g_prune_m < T ? g_prune_m : 0;
    int m = 2;
    while ((double)m * (m + 1) < 0.02 * T * (T + 1)) ++m;
    return m < T ? m : 0;
}
// k_trigemm_rows's job table: the 64-row halves of the row pieces, heaviest (most chunks) first -- rt | hh << 16 | solo << 17.  The
// weight falls with rt, so the halves of the row tiles >= t0 are the table's first rows_halves_from(t0) entries.
static std::vector<int> rows_halves(const std::vector<int>& pieces) {
    std::vector<int> out;
    for (int c : pieces) {
        const int rt = c & 0xffff, mode = c >> 16;
        if (mode == PIECE_UPPER_SOLO) out.push_back(rt | 1 << 17);
        else { out.push_back(rt | 1 << 16); out.push_back(rt); }
    }
    std::stable_sort(out.begin(), out.end(), [](int a, int b) {   // chunks: 8 rt + 8 (lower half), 8 rt + 4 (upper, solo)
        return 8 * (a & 0xffff) + ((a >> 16) & 1) * 4 > 8 * (b & 0xffff) + ((b >> 16) & 1) * 4;
    });
    return out;
}
static int rows_halves_from(const std::vector<int>& hv, int t0) {
    int n = 0;
    while (n < (int)hv.size() && (hv[n] & 0xffff) >= t0) ++n;
    return n;
}
// groups: column groups in the grid, 0: as many as cnt_max candidates need (no workgroup takes a second one); a list longer than
// cnt_max is not this launch's.  pf, arrive: the round finishes in the launch (its last arriver); nullptr: the caller enqueues the finish.
static int launch_trigemm_rows(bohip_gp* g, const double* KsT, const int* halves, int NH, const int* list, const unsigned* cnt,
                               int cnt_max, double* q, int64_t ldq, double* mu, int groups = 0, const PruneFinish* pf = nullptr,
                               unsigned* arrive = nullptr) {
    if (NH <= 0 || cnt_max <= 0) return 0;
    RowsParams rp{};
    rp.W = g->dW; rp.ldw = g->ld; rp.KsT = KsT; rp.ldk = g->ld; rp.list = list; rp.cnt = cnt; rp.cnt_max = cnt_max;
    rp.halves = halves; rp.NH = NH; rp.G = groups > 0 ? groups : (cnt_max + RS_COLS - 1) / RS_COLS;
    rp.alpha_row = g->n; rp.q = q; rp.ldq = ldq; rp.mu = mu;
    if (pf) { rp.finish = 1; rp.arrive = arrive; rp.pf = *pf; }
    hipLaunchKernelGGL(k_trigemm_rows, dim3((unsigned)(8 * ((NH + 7) / 8) * rp.G)), dim3(RS_THREADS), RS_LDS_BYTES, g->stream, rp);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_trigemm_on(bohip_gp* g, const double* KsT, const int* pieces, int NP, int CT, double* q, int64_t ldq, double* mu_raw,
                             FuseParams fz) {
    const int n_local = (CT + 7) / 8;
    if (NP <= 0 || CT <= 0) return 0;
    if (g->timing && g->dclk) fz.clk = g->dclk;
    hipLaunchKernelGGL(k_trigemm_sq, dim3(8 * n_local * NP), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), g->stream, g->dW, g->ld, KsT,
                       g->ld, pieces, NP, CT, g->n, q, ldq, mu_raw, (int64_t)0, nullptr, g->ld, fz);
    HIPCHK(hipGetLastError());
    return 0;
}
// Phase A's job table (k_trigemm_sq_pa): the two 64-row halves of every row piece with rt < m, rt | hh << 16.  Every such piece is a
// whole tile and none holds the alpha row (m < T: the last tile is not in the prefix).  Order: sorted heaviest first (chunks: 8 rt + 8
// the lower half, 8 rt + 4 the upper), then the first third of the list swapped with the second.  At the bench shape all 384
// workgroups are resident at once, two to a CU where they share one, and the workgroups dealt last land beside the ones dealt
// first: heaviest-first pairs the lightest jobs with the heaviest and the launch lasts 24 chunks at a shared CU's pace (22.1 us);
// with the middle third first the heaviest run alone and the lightest sit beside the middle ones (20.2 us;
// profiles/prune_phase_a_ab.txt).  The order cannot change a result: one job writes one q row.
static std::vector<int> phase_a_jobs(const std::vector<int>& pieces, int m) {
    std::vector<int> out;
    for (int c : pieces)
        if ((c & 0xffff) < m) { out.push_back((c & 0xffff) | 1 << 16); out.push_back(c & 0xffff); }
    std::stable_sort(out.begin(), out.end(), [](int a, int b) {
        return 8 * (a & 0xffff) + (a >> 16) * 4 > 8 * (b & 0xffff) + (b >> 16) * 4;
    });
    if (g_pa_order == 1) std::rotate(out.begin(), out.begin() + out.size() / 3, out.begin() + 2 * (out.size() / 3));
    return out;
}
static int launch_phase_a(bohip_gp* g, const double* KsT, const int* jobs, int NJOBS, int CT, double* q, int64_t ldq) {
    const int n_local = (CT + 7) / 8;
    if (NJOBS <= 0 || CT <= 0) return 0;
    hipLaunchKernelGGL(k_trigemm_sq_pa, dim3(8 * n_local * NJOBS), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), g->stream, g->dW, g->ld,
                       KsT, g->ld, jobs, CT, q, ldq, g->timing && g->dclk ? g->dclk : nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}
// One chunk, value-only: K*' with the partial sums of the alpha row's product -> phase A (row tiles < m, every candidate) -> bounds ->
// select (the 64 highest bounds) -> round 1 (row tiles >= m, exact finish: L; the finish lists round 2: every other candidate
// whose bound is not below L) -> round 2 -> the record.  Six launches: a round is ONE k_trigemm_rows launch whose last workgroup to
// arrive finishes it (scores, merges the record; round 1 lists round 2 and, when it lists nobody, writes the result).  Round 2's
// steady form is a fixed grid whose workgroups loop over the column groups: right for a list of any length, slow for a long one.
// long_form (the host expects a long list: score_core) is round 2 as four launches: gathered rows + k_trigemm_sq past PRUNE_ROWS_CAP
// candidates, k_trigemm_rows up to it, k_prune_finish.  No host round trip: the lists and their lengths stay on the device and the
// surplus workgroups leave at once.
// ub_host (tests, bohip_debug_prune_bounds): stop after the bounds and copy them out.
static int pruned_pass(bohip_gp* g, const double* dXs, const PassPlan& pl, const AcqParams& ap, Best* d_best, int64_t best_off,
                       double* ub_host = nullptr, bool long_form = false) {
    CHK(one_time_kernel_setup());
    {
        bool grew = false;
        HIPCHK(g->hprune_stat.reserve(16, g->stream, Grow::Exact, &grew));
        if (grew) g->hprune_stat[0] = 0u;
    }
    const int64_t N = pl.dm.N, Npad = pl.dm.Npad, R = pl.dm.R, Rpad = pl.dm.Rpad, ld = pl.dm.ld;
    const int T = pl.dm.T, m = pl.prune_m;
    const int64_t P = Npad / 64;   // k_kstar's partial sums: one per wave of observations
    CHK(ensure_pieces(g, T, N));
    // phase A runs 64-row jobs that write no mu: no piece of the prefix may be a solo half or hold the alpha row
    if (m >= T) return fail(BOHIP_E_STATE, "pruned pass: the prefix holds the alpha row");
    for (int c : g->hpieces)
        if ((c & 0xffff) < m && c >> 16 != PIECE_WHOLE) return fail(BOHIP_E_STATE, "pruned pass: a half piece in the prefix");
    layout::PrunedWs ws;
    auto lay = [&](const void* base) {
        return layout::pruned(base, (size_t)Rpad * ld, (size_t)2 * T * Rpad, (size_t)Rpad, PRUNE_K1, (size_t)2 * P * Rpad, 5 * g->hpieces.size() + 8, &ws);
    };
    bool fresh = false;
    HIPCHK(g->dpr.reserve(lay(nullptr), g->stream, Grow::Exact, &fresh));
    lay(g->dpr);
    double *ks2 = ws.ks, *q2 = ws.q2, *mu2 = ws.mu2, *ub = ws.ub;
    int *l1 = ws.l1, *l2 = ws.l2, *mark = ws.mark, *pcs = ws.pcs;
    const KstarParts kp{g->dW + N * ld, ws.parts, Rpad};
    g->pr_ks_len = (size_t)((char*)ws.q2 - (char*)ws.ks);
    unsigned* cnt = ws.cnt;
    Best* rec = static_cast<Best*>(ws.rec);
    if (g->timing) CHK(ensure_clk(g));
    g->score_launches = 1;
    const KernelHyper hp = make_hyper(g);
    // K*' first: it needs none of the job tables, and the device has nothing else to do while the host builds them
    t_begin(g, "kstar");
    CHK(launch_kstar_any(g, dXs, 0, R, Npad, hp, &kp));
    t_end(g);
    std::vector<int> pa, pb;   // the full pass's row pieces (same modes, same order), split at row tile m
    for (int c : g->hpieces) ((c & 0xffff) < m ? pa : pb).push_back(c);
    const std::vector<int> ph = phase_a_jobs(g->hpieces, m);
    const std::vector<int> hv = rows_halves(g->hpieces);   // (after the pieces in the table)
    const int nh = rows_halves_from(hv, m);
    std::vector<int> both = pa;
    both.insert(both.end(), pb.begin(), pb.end());
    both.insert(both.end(), hv.begin(), hv.end());
    both.insert(both.end(), ph.begin(), ph.end());   // (last: the other tables keep their offsets)
    if (fresh || g->hpr_pieces != both || g->pr_pieces_at != pcs) {   // (the table's offset moves with the batch)
        g->pr_pieces_at = pcs;
        g->hpr_pieces = both;   // (kept alive until the stream has consumed the copy)
        HIPCHK(hipMemcpyAsync(pcs, g->hpr_pieces.data(), both.size() * sizeof(int), hipMemcpyHostToDevice, g->stream));
    }
    const double sigma2 = std::exp(2.0 * g->logsig);
    const int k1 = (int)std::min<int64_t>(PRUNE_K1, R);
    // ONE bracket from phase A to the record, under the dense pass's label: what bench.py's roofline divides by
    t_begin(g, "trigemm_sq");
    FuseParams fz{};
    fz.T = T;
    CHK(launch_phase_a(g, g->dKsT, pcs + pa.size() + pb.size() + hv.size(), (int)ph.size(), (int)((R + CTILE - 1) / CTILE), g->dq, Rpad));
    PruneBound bd{};
    bd.parts = kp.parts; bd.P = P; bd.ldp = Rpad; bd.Npad = Npad; bd.q = g->dq; bd.ldq = Rpad; bd.R = R; bd.m = m;
    bd.sigma2 = sigma2; bd.beta = g->beta; bd.ap = ap; bd.ub = ub;
    hipLaunchKernelGGL(k_prune_bound, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, g->stream, bd);
    if (ub_host) {
        t_end(g);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ub_host, ub, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        return 0;
    }
    static_assert(PRUNE_R_MAX <= (int64_t)SELECT_THREADS * SELECT_PER, "k_prune_select holds the whole batch in one workgroup");
    hipLaunchKernelGGL(k_prune_select, dim3(1), dim3(SELECT_THREADS), 0, g->stream, (const double*)ub, R, k1, l1, mark, cnt, rec);
    HIPCHK(hipGetLastError());
    PruneFinish pf{};
    pf.q = g->dq; pf.ldq = Rpad; pf.q2 = q2; pf.ldq2 = Rpad; pf.mu2 = mu2; pf.m = m; pf.T = T; pf.sigma2 = sigma2; pf.beta = g->beta;
    pf.ap = ap; pf.rec = rec;
    const int* hvd = pcs + pa.size() + pb.size();
    pf.ub = ub; pf.mark = mark; pf.R = R; pf.cnt2 = cnt + 1; pf.best_off = (long long)best_off;
    // Round 1 finishes in its own launch: the last workgroup to arrive scores, merges and lists round 2 (the tail), and when it
    // lists nobody it writes the call's result and the pinned word itself.
    pf.list = l1; pf.cnt = cnt; pf.list2 = l2; pf.best_out = d_best; pf.stat = g->hprune_stat;
    CHK(launch_trigemm_rows(g, g->dKsT, hvd, nh, l1, cnt, k1, q2, Rpad, mu2, 0, &pf, cnt + PRUNE_ARRIVE));
    const int64_t cap = R - k1;   // worst case of round 2's list
    pf.list = l2; pf.cnt = cnt + 1; pf.list2 = nullptr;
    if (cap > 0 && !long_form) {
        // steady form, ONE launch for a list of any length: a fixed grid whose workgroups loop over the column groups; its last
        // arriver finishes the round and writes the result.  An empty list: every workgroup leaves, round 1 has written it.
        CHK(launch_trigemm_rows(g, g->dKsT, hvd, nh, l2, cnt + 1, INT_MAX, q2, Rpad, mu2, PRUNE_R2_GROUPS, &pf, cnt + PRUNE_ARRIVE + 1));
    } else if (cap > 0) {
        // long form, when a long list is expected: the row-split kernel takes lists of up to PRUNE_ROWS_CAP candidates, the gathered
        // rows and k_trigemm_sq the longer ones -- both are enqueued and the device-side count picks (cnt[2]: k_trigemm_sq's
        // count, 0 when the list is short); the finish is a launch of its own
        if (cap > PRUNE_ROWS_CAP) {
            hipLaunchKernelGGL(k_prune_gather, dim3((unsigned)cap), dim3(256), 0, g->stream, (const int*)l2, (const unsigned*)(cnt + 1),
                               (const double*)g->dKsT, ld, Npad, ks2, PRUNE_ROWS_CAP, cnt + 2);
            fz.live = cnt + 2;
            CHK(launch_trigemm_on(g, ks2, pcs + pa.size(), (int)pb.size(), (int)((cap + CTILE - 1) / CTILE), q2, Rpad, mu2, fz));
        }
        CHK(launch_trigemm_rows(g, g->dKsT, hvd, nh, l2, cnt + 1, (int)std::min<int64_t>(cap, PRUNE_ROWS_CAP), q2, Rpad, mu2));
        hipLaunchKernelGGL(k_prune_finish, dim3(1), dim3(256), 0, g->stream, pf);
        HIPCHK(hipGetLastError());
    }
    t_end(g);
    return 0;
}

// Path choice for value-only calls that qualify.  Pruning pays when few candidates outside round 1 survive; when many do, phase A,
// the bounds and round 1 (k_trigemm_rows, ~60 us at N = 3000) come on top of the full contraction.  The last pruned call of the handle left
// the length of its round-2 list in pinned memory (read without a wait: an older call's figure is as good a guide).  When more than an
// eighth of the batch survived, the next PRUNE_BACKOFF calls take the full pass, then one call tries pruning again.  Either path gives
// the same record bit for bit, so the choice moves only time.
constexpr int PRUNE_BACKOFF = 31;
static bool prune_wanted(bohip_gp* g, int64_t R) {
    if (g->prune_skip > 0) { --g->prune_skip; return false; }
    g->prune_seen = 0u;
    if (g->hprune_stat) {
        const unsigned n2 = __atomic_load_n(g->hprune_stat.get(), __ATOMIC_RELAXED);
        g->prune_seen = n2;
        if ((int64_t)n2 > R / 8) {
            __atomic_store_n(g->hprune_stat.get(), 0u, __ATOMIC_RELAXED);
            g->prune_skip = PRUNE_BACKOFF - 1;
            g->prune_retry = true;   // (the word no longer says why: the call after the back-off expects a long list)
            return false;
        }
    }
    return true;
}

// The route of a pass over R candidates, chosen ONCE.  The caller says what it can take: the small pass, the split-K posterior (neither
// where V' must come in the chunk layout), and pruning -- Value: a call that wants the record alone; not for shards of a larger set
// (batch_hint); prune_wanted (the back-off: side effects) is asked last.  Probe: "would this size prune?", no hint, no back-off.
enum class Prune { No, Value, Probe };
struct RouteWants { bool small = true, split = true; Prune prune = Prune::No; };
static constexpr RouteWants WHOLE_K_ONLY{false, false, Prune::No};
static PassPlan choose_route(bohip_gp* g, int64_t R, RouteWants w) {
    PassPlan pl;
    pl.dm = pass_dims(g, R); pl.chunk = chunk_rows(g, R);
    if (w.small && path_R(g, R) <= small_limit(g) && R <= SMALL_MAX) pl.route = Route::Small;
    else if (w.split && (pl.sp = split_plan(g, R)).nsl > 0) pl.route = Route::Split;
    else if (const int m = w.prune != Prune::No ? prune_tiles(pl.dm.T) : 0;
             m > 0 && R <= PRUNE_R_MAX && R <= pl.chunk && (w.prune == Prune::Probe || (g->batch_hint == 0 && prune_wanted(g, R)))) {
        pl.route = Route::Pruned;
        pl.prune_m = m;
    }
    return pl;
}

// best_off: added to the winner's index (a shard of a larger candidate set reports GLOBAL columns)
static int score_core(bohip_gp* g, int acq_id, const double* acq_params, const double* dXs, int64_t R, double* d_mu,
                      double* d_var, double* d_score, Best* d_best, int64_t best_off = 0) {
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(ensure_fresh(g));
    CHK(ensure_score_scratch(g, R));
    AcqParams ap;
    CHK(make_acq(acq_id, acq_params, &ap));
    const bool record_only = d_best && !d_mu && !d_var && !d_score;
    const PassPlan pl = choose_route(g, R, RouteWants{true, true, record_only ? Prune::Value : Prune::No});
    if (pl.route == Route::Small) {   // small batches: scoring and arg-max ride on the pass's own kernel
        CHK(one_time_kernel_setup());
        return small_pass_mfma(g, dXs, R, ap, d_mu, d_var, d_score, d_best, best_off, nullptr);
    }
    if (pl.route == Route::Split) {   // a few hundred candidates: split-K posterior, then scoring and arg-max as launches of their own
        CHK(split_posterior(g, dXs, pl, false));
        const int nb = (int)((R + 255) / 256);
        t_begin(g, "score");
        hipLaunchKernelGGL(k_score, dim3(nb), dim3(256), 0, g->stream, g->dq, pl.dm.Rpad, pl.dq_tiles(), g->dmu_raw, R,
                           std::exp(2.0 * g->logsig), g->beta, ap, d_mu, d_var, d_score, d_best ? g->dblock_best : nullptr);
        if (d_best) hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, g->dblock_best, nb, d_best, (long long)best_off);
        HIPCHK(hipGetLastError());
        t_end(g);
        return 0;
    }
    if (pl.route == Route::Pruned) {
        // value-only: only the winner leaves the call -- candidates that provably cannot win are not contracted past m row tiles.
        // round 2's form (either gives the same record): the long one when the last figure read or a back-off announces a long list
        const bool want_long = g->prune_retry || g->prune_seen > (unsigned)PRUNE_ROWS_CAP;
        g->prune_retry = false;
        return pruned_pass(g, dXs, pl, ap, d_best, best_off, nullptr, g->prune_r2_form < 0 ? want_long : g->prune_r2_form == 1);
    }
    // whole-K jobs: scoring and arg-max ride in k_trigemm_sq's epilogue (the workgroup that completes a candidate tile
    // finishes it; the one that completes the last tile writes the record): no k_score / k_argmax_final launches
    FuseParams fz{};
    fz.tile_cnt = g->dfz_cnt; fz.total_cnt = g->dfz_cnt + g->fz_tiles; fz.tile_best = g->dfz_best;
    fz.tiles_total = (int)((R + CTILE - 1) / CTILE); fz.R_total = R;
    fz.sigma2 = std::exp(2.0 * g->logsig); fz.beta = g->beta; fz.ap = ap;
    fz.mu_out = d_mu; fz.var_out = d_var; fz.score_out = d_score; fz.best_out = d_best; fz.best_off = best_off;
    // The fused finish counts arrivals in counters its last waves leave at zero.  If an earlier call failed between two of
    // its launches they are not: every later call would then miss its "last arrival" and write no result.  So a call that
    // did not enqueue all of its launches marks the counters dirty, and the next one clears them first.
    if (g->fz_dirty) HIPCHK(hipMemsetAsync(g->dfz_cnt, 0, (size_t)(g->fz_tiles + 1 + 16) * sizeof(unsigned), g->stream));
    g->fz_dirty = true;
    CHK(one_time_kernel_setup());
    const int64_t chunks = chunk_pass(g, pl, dXs, make_hyper(g), ChunkV{}, false, fz, no_finish);
    if (chunks < 0) return (int)chunks;
    g->score_launches = chunks;
    g->fz_dirty = false;
    return 0;
}

template <int DT>
static void launch_grad(bohip_gp* g, const double* dXs, int64_t r0, int64_t r1, const KernelHyper& hp, const AcqParams& ap,
                        double* d_grad, const double* UT, int S) {
    if constexpr (DT <= 16) {   // large batches: 4 candidates per workgroup share the observation stream
        if (r1 - r0 > SMALL_MAX) {
            LAUNCH_FAM(fam_low(hp), (k_grad_finish_tiled<DT, true>), (k_grad_finish_tiled<DT, false>), dim3((unsigned)((r1 - r0 + GC - 1) / GC)),
                       dim3(256), 0, g->stream, g->dX, g->n, dXs, r0, r1, hp, g->dalpha, UT, g->ld, g->dmu, g->dvar, ap, d_grad);
            return;
        }
    }
    LAUNCH_FAM(fam_low(hp), (k_grad_finish<DT, true>), (k_grad_finish<DT, false>), dim3((unsigned)(r1 - r0), (unsigned)S), dim3(256), 0,
               g->stream, g->dX, g->n, dXs, r0, r1, hp, g->dalpha, UT, g->ld, g->dmu, g->dvar, ap, d_grad, g->dgparts, g->dgcount);
}
// k_grad_finish and k_post_grad_finish split the observations of a small batch over *S workgroups per candidate (S > 1: their counters)
// (one 256-observation stride per workgroup -- (n + 255) / 256 splits -- was measured in round 4: 2 us of a 58 us pass, and the changed
// summation order moved the ascent's end points enough to graze the SciPy check's KKT bound at N = 600: not kept)
static int grad_obs_splits(bohip_gp* g, int64_t r0, int64_t r1, int* S) {
    *S = r1 - r0 <= SMALL_MAX ? (int)std::min<int64_t>(16, std::max<int64_t>(1, g->n / 768)) : 1;
    if (*S > 1) CHK(ensure_small_counters(g));
    return 0;
}
static int launch_grad_any(bohip_gp* g, const double* dXs, int64_t r0, int64_t r1, const KernelHyper& hp, const AcqParams& ap,
                           double* d_grad, const double* UT) {
    int S = 1;
    CHK(grad_obs_splits(g, r0, r1, &S));
    dispatch_dt(g->d, [&](auto dt) { launch_grad<decltype(dt)::value>(g, dXs, r0, r1, hp, ap, d_grad, UT, S); });
    HIPCHK(hipGetLastError());
    return 0;
}

// k_post_grad_finish (kernels_con.hip): launch_grad without the functor
template <int DT>
static void launch_post_grad(bohip_gp* g, const double* dXs, int64_t r0, int64_t r1, const KernelHyper& hp, double* d_jmu, double* d_jvar,
                             const double* UT, int S) {
    if constexpr (DT <= 16) {   // large batches: two candidates per workgroup share the observation stream (launch_grad's rule)
        if (r1 - r0 > SMALL_MAX) {
            LAUNCH_FAM(fam_low(hp), (k_post_grad_finish_tiled<DT, true>), (k_post_grad_finish_tiled<DT, false>),
                       dim3((unsigned)((r1 - r0 + GC - 1) / GC)), dim3(256), 0, g->stream, g->dX, g->n, dXs, r0, r1, hp, g->dalpha, UT, g->ld,
                       d_jmu, d_jvar);
            return;
        }
    }
    LAUNCH_FAM(fam_low(hp), (k_post_grad_finish<DT, true>), (k_post_grad_finish<DT, false>), dim3((unsigned)(r1 - r0), (unsigned)S), dim3(256), 0,
               g->stream, g->dX, g->n, dXs, r0, r1, hp, g->dalpha, UT, g->ld, d_jmu, d_jvar, g->dgparts, g->dgcount);
}

// A8: scores + gradients for R candidates (device pointers).  Per chunk: K*' -> V' (trigemm, V stored)
// -> U' = V' W (k_gemm) -> mu, sigma^2, score -> gradient.
static int score_grad_core(bohip_gp* g, int acq_id, const double* acq_params, const double* dXs, int64_t R, double* d_score,
                           double* d_grad, const AscPass& asc = AscPass{}) {
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(ensure_fresh(g));
    CHK(ensure_score_scratch(g, R));
    CHK(one_time_kernel_setup());
    AcqParams ap;
    CHK(make_acq(acq_id, acq_params, &ap));
    const PassPlan pl = choose_route(g, R, RouteWants{});
    const KernelHyper hp = make_hyper(g);
    if (pl.route == Route::Small) {  // the reference's default: a handful of L-BFGS restarts per call
        // two MFMA kernels (kernels_small.hip): K*' + V' + posterior finish, U' + gradient
        return small_pass_mfma(g, dXs, R, ap, g->dmu, g->dvar, d_score, nullptr, 0, d_grad, asc);
    }
    auto finish = [&](int64_t r0, int64_t r1) {
        t_begin(g, "score+grad");
        hipLaunchKernelGGL(k_score, dim3((unsigned)((r1 - r0 + 255) / 256)), dim3(256), 0, g->stream, g->dq + r0, pl.dm.Rpad, pl.dq_tiles(),
                           g->dmu_raw + r0, r1 - r0, std::exp(2.0 * g->logsig), g->beta, ap, g->dmu + r0, g->dvar + r0, d_score + r0,
                           (Best*)nullptr);
        CHK(launch_grad_any(g, dXs, r0, r1, hp, ap, d_grad, g->dUT));
        t_end(g);
        return 0;
    };
    return posterior_then(g, pl, dXs, hp, true, finish);
}

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char* bohip_last_error(void) { return g_err.c_str(); }
const char* bohip_version(void) { return "bohip 0.1 (gfx950, fp64 mfma 4x4x4)"; }
int bohip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bohip_gp_create(int64_t d, int64_t capacity, int kernel_id, int device, bohip_gp** out) {
    if (!out) return fail(BOHIP_E_ARG, "out is null");
    *out = nullptr;
    if (d < 1 || d > DMAX) return fail(BOHIP_E_ARG, "d must be in [1, 64]");
    if (capacity < 1) capacity = 1;
    if (kernel_id < 0 || kernel_id >= KERN_COUNT) return fail(BOHIP_E_ARG, "unknown kernel_id");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(BOHIP_E_NODEVICE, "no HIP device visible; libbohip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(BOHIP_E_ARG, "device ordinal out of range");
    HIPCHK(hipSetDevice(device));
    bohip_gp* g = new bohip_gp();
    g->device = device;
    g->d = (int)d;
    g->kern = kernel_id;
    for (int k = 0; k < DMAX; ++k) g->loglen[k] = 0.0;
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipError_t e = hipStreamCreateWithPriority(&g->own_stream, hipStreamNonBlocking, prio_hi);  // critical path of the factorisation
    // (reserving CUs for the critical stream with a CU mask on the side stream was measured and does not help)
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&g->side_stream, hipStreamNonBlocking, prio_lo);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_panels, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_bulk, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&g->col_stream, hipStreamNonBlocking, prio_hi);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_inv, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_gate, hipEventDisableTiming);
    if (e != hipSuccess) { delete g; return fail(BOHIP_E_HIP, hipGetErrorString(e)); }
    g->stream = g->own_stream;
    if (g->hpin.reserve(layout::pinned_small(nullptr, SMALL_R, DMAX, &g->pin) / sizeof(double), g->stream) != hipSuccess) g->pin = {};
    else layout::pinned_small(g->hpin, SMALL_R, DMAX, &g->pin);   // (without the block the small batches take the copies)
    if (g->dinfo.reserve(1, g->stream) != hipSuccess || g->dmll.reserve(DMAX + 4, g->stream) != hipSuccess ||
        g->dbest.reserve(4096, g->stream) != hipSuccess) {
        delete g;
        return fail(BOHIP_E_HIP, "hipMalloc failed");
    }
    int rc = alloc_model(g, capacity);
    if (rc != 0) {
        delete g;
        (void)hipGetLastError();   // (the runtime keeps a failed allocation's error until it is read: not for the next call's launch check)
        return rc;
    }
    if (const char* e = getenv("BOHIP_JITTER")) {   // "rel[,tries]": jitter escalation for every handle of the process (default: off)
        double rel = 0.0;
        int tries = 10;
        if (sscanf(e, "%lf,%d", &rel, &tries) >= 1 && rel > 0.0) { g->jitter_rel = rel; g->jitter_tries = std::min(32, std::max(1, tries)); }
    }
    *out = g;
    return 0;
}

// (the teardown is the handle's destructor: stream, communicator, every buffer, then the events and streams)
void bohip_gp_destroy(bohip_gp* g) { delete g; }

int bohip_gp_set_hyper(bohip_gp* g, const double* loglen, double logsig, double lognoise, double mean_const) {
    if (!g || !loglen) return fail(BOHIP_E_ARG, "null argument");
    const int nl = kern_iso(g->kern) ? 1 : g->d;
    for (int k = 0; k < nl; ++k) g->loglen[k] = loglen[k];
    if (kern_iso(g->kern))
        for (int k = 1; k < g->d; ++k) g->loglen[k] = loglen[0];
    g->logsig = logsig;
    g->lognoise = lognoise;
    g->beta = mean_const;
    g->stale = true;
    g->hyper_gen++;
    return 0;
}

// The host side of a weighted handle's new rows: 1 / r_i and r_i behind the mirrors' first n_old entries, and the sums of the
// sites' constant C (bohip_rep.h); _pop takes a failed growth back.
static void site_mirrors_push(bohip_gp* g, int64_t n_old, const int64_t* reps, const double* ss, int64_t p) {
    g->hinvr.resize((size_t)n_old, 1.0);
    g->hreps.resize((size_t)n_old, 1);
    for (int64_t i = 0; i < p; ++i) {
        const int64_t r = reps ? reps[i] : 1;
        g->hinvr.push_back(1.0 / (double)r);
        g->hreps.push_back(r);
        g->n_evals_extra += r - 1;
        g->sum_log_reps += std::log((double)r);
        if (ss) g->ss_total += ss[i];
    }
}
struct SiteSums { int64_t extra; double ss, slr; };
static void site_mirrors_pop(bohip_gp* g, int64_t n_old, const SiteSums& was) {
    g->hinvr.resize((size_t)n_old);
    g->hreps.resize((size_t)n_old);
    g->n_evals_extra = was.extra; g->ss_total = was.ss; g->sum_log_reps = was.slr;
}
// What bohip_gp_append and bohip_gp_append_sites (include/bohip_rep.h) share.  reps == nullptr: plain rows, r = 1 and s = 0 each; on
// an unweighted handle that is the whole of bohip_gp_append, launch for launch.  A weighted handle (the caller has turned it so) also
// keeps 1 / r_i beside X and y -- mirror, staged copy, device vector -- and the three sums of the sites' constant.
static int append_rows(bohip_gp* g, const double* X, const double* y, const int64_t* reps, const double* ss, int64_t p) {
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    int rc = 0;
    bool done = false;
    if (p > 0) {
        ++g->data_version;
        const int64_t n_old = g->n, n_new = g->n + p;
        const SiteSums was{g->n_evals_extra, g->ss_total, g->sum_log_reps};
        if (n_new > g->cap) {
            // growth: alloc_model re-uploads everything from the host mirrors, so they are extended first -- and rolled
            // back if the allocation fails (the handle then holds its old observations and no device buffers; the next
            // call that needs them allocates again, see ensure_fresh)
            g->hX.insert(g->hX.end(), X, X + p * g->d);
            g->hy.insert(g->hy.end(), y, y + p);
            g->n = n_new;
            if (g->weighted) site_mirrors_push(g, n_old, reps, ss, p);
            const int arc = alloc_model(g, std::max<int64_t>(2 * g->cap, n_new));
            if (arc != 0) {
                g->hX.resize((size_t)n_old * g->d);
                g->hy.resize((size_t)n_old);
                g->n = n_old;
                if (g->weighted) site_mirrors_pop(g, n_old, was);
                free_model(g);
                g->cap = 0;
                g->stale = true;
                return arc;
            }
        } else {
            // A few rows (what a BO iteration appends) go through the pinned block: the copies are then plain DMA commands in front of the
            // update's kernels, the pivot word comes back the same way, and the call synchronises ONCE (three times before: behind the
            // pageable copies, for the pivot word, at the end -- ~60 us of a 0.19 ms append).  Otherwise: the mirrors and n advance only
            // after the device holds the new rows, a failed copy leaves the handle unchanged.
            const bool staged = g->hpin && p <= SMALL_R && (size_t)p * g->d <= (size_t)SMALL_R * DMAX;
            int* pinfo = nullptr;
            if (staged) {
                double* sx = g->pin.grad;   // (the gradient area and the score area of the result block: idle during an append)
                double* sy = g->pin.score;
                std::memcpy(sx, X, (size_t)p * g->d * 8);
                std::memcpy(sy, y, (size_t)p * 8);
                HIPCHK(hipMemcpyAsync(g->dX + n_old * g->d, sx, (size_t)p * g->d * 8, hipMemcpyHostToDevice, g->stream));
                HIPCHK(hipMemcpyAsync(g->dy + n_old, sy, (size_t)p * 8, hipMemcpyHostToDevice, g->stream));
                if (g->weighted) {
                    double* sw = g->pin.mu;   // (idle during an append, like the two above)
                    for (int64_t i = 0; i < p; ++i) sw[i] = reps ? 1.0 / (double)reps[i] : 1.0;
                    HIPCHK(hipMemcpyAsync(g->dinvr + n_old, sw, (size_t)p * 8, hipMemcpyHostToDevice, g->stream));
                }
                pinfo = g->pin.words;
                *pinfo = 0;
            } else {
                HIPCHK(hipMemcpyAsync(g->dX + n_old * g->d, X, (size_t)p * g->d * 8, hipMemcpyHostToDevice, g->stream));
                HIPCHK(hipMemcpyAsync(g->dy + n_old, y, (size_t)p * 8, hipMemcpyHostToDevice, g->stream));
                if (g->weighted) {
                    std::vector<double> w((size_t)p);
                    for (int64_t i = 0; i < p; ++i) w[i] = reps ? 1.0 / (double)reps[i] : 1.0;
                    HIPCHK(hipMemcpy(g->dinvr + n_old, w.data(), (size_t)p * 8, hipMemcpyHostToDevice));
                }
                HIPCHK(hipStreamSynchronize(g->stream));  // caller's buffers are only valid during the call
            }
            g->hX.insert(g->hX.end(), X, X + p * g->d);
            g->hy.insert(g->hy.end(), y, y + p);
            g->n = n_new;
            if (g->weighted) site_mirrors_push(g, n_old, reps, ss, p);
            if (!g->stale && g->n_factored == n_old && n_old > 0 && p <= APPEND_PMAX) {
                rc = append_incremental(g, n_old, p, pinfo);
                if (rc != 0) { g->stale = true; g->mirror_dirty = staged; }   // (staged: the rows' copies were only queued -- the device may not hold them)
                done = true;
                if (rc == 0 && pinfo) {
                    const hipError_t e = hipStreamSynchronize(g->stream);
                    if (e != hipSuccess) { g->stale = true; g->mirror_dirty = true; return fail(BOHIP_E_HIP, hipGetErrorString(e)); }
                    t_collect(g);
                    if (*pinfo != 0) {
                        g->pivot = *pinfo;
                        g->stale = true;
                        return fail(BOHIP_E_NOTPD, "kernel matrix not positive definite at pivot " + std::to_string(*pinfo));
                    }
                    g->pivot = 0;
                    return 0;
                }
            }
        }
    }
    if (!done) rc = ensure_fresh(g);
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return rc;
}

int bohip_gp_append(bohip_gp* g, const double* X, const double* y, int64_t p) {
    if (!g || p < 0 || (p > 0 && (!X || !y))) return fail(BOHIP_E_ARG, "bad arguments");
    return append_rows(g, X, y, nullptr, nullptr, p);
}

// ---- replicated sites (include/bohip_rep.h) ------------------------------------------------------------------------
int bohip_gp_append_sites(bohip_gp* g, const double* X, const double* ybar, const int64_t* reps, const double* ss, int64_t p) {
    if (!g || p < 0 || (p > 0 && (!X || !ybar || !reps || !ss))) return fail(BOHIP_E_ARG, "bad arguments");
    bool any = false;
    for (int64_t i = 0; i < p; ++i) {
        if (reps[i] < 1) return fail(BOHIP_E_ARG, "site " + std::to_string(i) + ": reps must be >= 1");
        if (!std::isfinite(ss[i]) || ss[i] < 0.0) return fail(BOHIP_E_ARG, "site " + std::to_string(i) + ": ss must be finite and >= 0");
        if (reps[i] == 1 && ss[i] != 0.0) return fail(BOHIP_E_ARG, "site " + std::to_string(i) + ": one evaluation has no within-site sum of squares (ss must be 0)");
        any = any || reps[i] > 1;
    }
    if (!g->weighted && !any) return append_rows(g, X, ybar, nullptr, nullptr, p);   // all r = 1: bohip_gp_append itself
    if (!g->weighted) {
        // the handle turns weighted: the rows it holds are sites of one evaluation (their diagonal entries, hence the factor, stand)
        HIPCHK(hipSetDevice(g->device));
        g->hinvr.assign((size_t)g->n, 1.0);
        g->hreps.assign((size_t)g->n, 1);
        g->n_evals_extra = 0; g->ss_total = 0.0; g->sum_log_reps = 0.0;
        g->weighted = true;
        g->ens_factor_ok = false;
        const int rc = upload_site_weights(g);
        if (rc != 0) { g->mirror_dirty = true; g->stale = true; return rc; }
    }
    return append_rows(g, X, ybar, reps, ss, p);
}
int bohip_gp_sites_info(const bohip_gp* g, int64_t* n_sites, int64_t* n_evals, double* ss_total, double* sum_log_reps, int* weighted) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    if (n_sites) *n_sites = g->n;
    if (n_evals) *n_evals = g->n + (g->weighted ? g->n_evals_extra : 0);
    if (ss_total) *ss_total = g->weighted ? g->ss_total : 0.0;
    if (sum_log_reps) *sum_log_reps = g->weighted ? g->sum_log_reps : 0.0;
    if (weighted) *weighted = g->weighted ? 1 : 0;
    return 0;
}
int bohip_gp_get_reps(const bohip_gp* g, int64_t* reps_out) {
    if (!g || (g->n > 0 && !reps_out)) return fail(BOHIP_E_ARG, "null argument");
    for (int64_t i = 0; i < g->n; ++i) reps_out[i] = g->weighted ? g->hreps[(size_t)i] : 1;
    return 0;
}
// The part of the log marginal likelihood of ALL evaluations that the collapsed model does not see, and its derivative by logNoise:
//   C = -1/2 (N_tot - n) log(2 pi nu) - 1/2 sum log r_i - (sum s_i) / (2 nu),   nu = exp(2 logNoise) + eps + jitter_last
static void site_constant(const bohip_gp* g, double* Cval, double* dC_dlognoise) {
    const double s2 = std::exp(2.0 * g->lognoise), nu = s2 + std::numeric_limits<double>::epsilon() + g->jitter_last;
    const double m = (double)g->n_evals_extra;
    *Cval = -0.5 * m * std::log(2.0 * M_PI * nu) - 0.5 * g->sum_log_reps - g->ss_total / (2.0 * nu);
    if (dC_dlognoise) *dC_dlognoise = 2.0 * s2 * (-m / (2.0 * nu) + g->ss_total / (2.0 * nu * nu));
}

int bohip_gp_refit(bohip_gp* g) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    int rc = refit(g);
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return rc;
}

int bohip_gp_dims(const bohip_gp* g, int64_t* d, int64_t* n) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    if (d) *d = g->d;
    if (n) *n = g->n;
    return 0;
}
int bohip_gp_maxy(const bohip_gp* g, double* maxy) {
    if (!g || !maxy) return fail(BOHIP_E_ARG, "null argument");
    double m = -INFINITY;
    for (double v : g->hy) if (v > m) m = v;
    *maxy = m;
    return 0;
}
int bohip_gp_get_xy(const bohip_gp* g, double* X, double* y) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    if (X && g->n) std::memcpy(X, g->hX.data(), (size_t)g->n * g->d * 8);
    if (y && g->n) std::memcpy(y, g->hy.data(), (size_t)g->n * 8);
    return 0;
}

int bohip_gp_mll(bohip_gp* g, double* mll) {
    if (!g || !mll) return fail(BOHIP_E_ARG, "null argument");
    HIPCHK(hipSetDevice(g->device));
    if (g->n == 0) { *mll = 0.0; return 0; }
    CHK(ensure_fresh(g));
    hipLaunchKernelGGL(k_mll, dim3(1), dim3(256), 0, g->stream, g->dL, g->ld, g->n, g->dr, g->dalpha, g->dmll);
    HIPCHK(hipGetLastError());
    double* const pm = g->hpin ? g->pin.score : mll;     // (through the pinned block: a plain DMA command)
    HIPCHK(hipMemcpyAsync(pm, g->dmll, 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    *mll = *pm;
    if (g->weighted) {   // replicated sites: the likelihood of every evaluation, not of the site means alone
        double Cv;
        site_constant(g, &Cv, nullptr);
        *mll += Cv;
    }
    return 0;
}

// cK^-1 = W'W into the lower 128-tiles of dS:  (W'W)_ij = sum_{k >= max(i,j)} W'[i][k] W'[j][k]  (both gradients: the marginal
// likelihood's and the leave-one-out log-probability's)
static int kinv_into_scratch(bohip_gp* g) {
    const int64_t ld = g->ld;
    const int T = row_tiles(g);
    t_begin(g, "kinv");
    GemmNTParams p{};
    p.A = g->dWT; p.lda = ld; p.B = g->dWT; p.ldb = ld; p.C = g->dS; p.ldc = ld;
    p.mt = T; p.nt64 = 2 * T; p.kc = T * (TILE / KC); p.alpha = 1.0; p.beta = 0.0;
    p.klo_from_m = 1; p.klo_from_n = 1; p.diag_skip = 1; p.row0 = 0; p.col0 = 0;
    CHK(launch_gemm_nt(g, p));
    t_end(g);
    return 0;
}

int bohip_gp_mll_grad(bohip_gp* g, double* mll, double* d_lognoise, double* d_mean, double* d_kern) {
    if (!g || !mll || !d_lognoise || !d_mean || !d_kern) return fail(BOHIP_E_ARG, "null argument");
    HIPCHK(hipSetDevice(g->device));
    const int iso = kern_iso(g->kern), nl = iso ? 1 : g->d;
    if (g->n == 0) {
        *mll = 0.0; *d_lognoise = 0.0; *d_mean = 0.0;
        for (int k = 0; k <= nl; ++k) d_kern[k] = 0.0;
        return 0;
    }
    CHK(ensure_fresh(g));
    const int64_t N = g->n, ld = g->ld;
    const int NP = g->d + 3;
    hipLaunchKernelGGL(k_mll, dim3(1), dim3(256), 0, g->stream, g->dL, ld, N, g->dr, g->dalpha, g->dmll);
    CHK(kinv_into_scratch(g));
    t_begin(g, "dmll_reduce");
    const int rpb = 32;
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)((N + rpb - 1) / rpb));
    const int64_t nblocks = (int64_t)grid.x * grid.y;
    HIPCHK(g->ddmll_parts.reserve((size_t)nblocks * NP, g->stream));
    const KernelHyper hp = make_hyper(g);
    const double noise_var = std::exp(2.0 * g->lognoise);
    dispatch_dt(g->d, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        LAUNCH_FAM(fam_low(hp), (k_dmll_parts<DT, true>), (k_dmll_parts<DT, false>), grid, dim3(256), 0, g->stream, g->dX, N, hp, noise_var,
                   g->dS, ld, g->dalpha, rpb, g->ddmll_parts);
    });
    const int nout = nl + 3;
    hipLaunchKernelGGL(k_dmll_final, dim3(nout), dim3(256), 0, g->stream, g->ddmll_parts, nblocks, NP, g->d, iso, g->dmll + 1);
    if (g->weighted)   // replicated sites: slot 1 is sigma^2 sum_i (alpha_i^2 - cK_w^-1_ii) / r_i (behind k_dmll_final on the stream: its slot 1 is replaced)
        hipLaunchKernelGGL(k_rep_noise_sum, dim3(1), dim3(256), 0, g->stream, g->dalpha, g->dS, ld, N, g->dinvr, g->dmll + 1);
    HIPCHK(hipGetLastError());
    t_end(g);
    double hbuf[DMAX + 4];
    double* const h = g->hpin ? g->pin.grad : hbuf;     // (the pinned block's gradient area: a plain DMA command)
    HIPCHK(hipMemcpyAsync(h, g->dmll, 8 * (size_t)(nout + 1), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    *mll = h[0]; *d_lognoise = h[1]; *d_mean = h[2];
    for (int k = 0; k <= nl; ++k) d_kern[k] = h[3 + k];
    if (g->weighted) {   // 2 sigma^2 sum_i G_ii / r_i with G_ii = 1/2 (alpha_i^2 - cK_w^-1_ii), then the sites' constant and its derivative
        double Cv, dC;
        site_constant(g, &Cv, &dC);
        *mll += Cv;
        *d_lognoise = noise_var * h[1] + dC;
    }
    return 0;
}

// ---- leave-one-out cross-validation (kernels_loo.hip, include/bohip_loo.h) ----------------------------------------
static int ensure_loo(bohip_gp* g, layout::LooWs* w) {
    const size_t nv = (size_t)g->ld + 256;   // (as dalpha / dr / dt: k_trimv_stream reads whole chunks of 256, masked by index)
    HIPCHK(g->loo_ws.reserve(layout::loo(nullptr, DMAX + 4, nv, w), g->stream));
    layout::loo(g->loo_ws, DMAX + 4, nv, w);
    return 0;
}
// kappa from the resident W', then every per-point value and their sum into w.out[0]: the two launches both symbols share
static int loo_values(bohip_gp* g, const layout::LooWs& w) {
    const int64_t N = g->n;
    t_begin(g, "loo_kappa");
    hipLaunchKernelGGL(k_loo_kappa, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, g->stream, g->dWT, g->ld, N, w.kappa);
    hipLaunchKernelGGL(k_loo_finish, dim3(1), dim3(256), 0, g->stream, g->dy, g->dalpha, w.kappa, N, w.mu, w.var, w.logp, w.q, w.sc, w.out);
    HIPCHK(hipGetLastError());
    t_end(g);
    return 0;
}

int bohip_gp_loo(bohip_gp* g, double* mu, double* var, double* logp, double* total) {
    if (!g || !total) return fail(BOHIP_E_ARG, "null argument");
    HIPCHK(hipSetDevice(g->device));
    if (g->n == 0) { *total = 0.0; return 0; }
    t_reset(g);
    CHK(ensure_fresh(g));
    layout::LooWs w;
    CHK(ensure_loo(g, &w));
    CHK(loo_values(g, w));
    const size_t nb = (size_t)g->n * 8;
    if (mu) HIPCHK(hipMemcpyAsync(mu, w.mu, nb, hipMemcpyDeviceToHost, g->stream));
    if (var) HIPCHK(hipMemcpyAsync(var, w.var, nb, hipMemcpyDeviceToHost, g->stream));
    if (logp) HIPCHK(hipMemcpyAsync(logp, w.logp, nb, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(total, w.out, 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

int bohip_gp_loo_grad(bohip_gp* g, double* total, double* d_lognoise, double* d_mean, double* d_kern) {
    if (!g || !total || !d_lognoise || !d_mean || !d_kern) return fail(BOHIP_E_ARG, "null argument");
    CHK(refuse_weighted(g, "bohip_gp_loo_grad"));
    HIPCHK(hipSetDevice(g->device));
    const int iso = kern_iso(g->kern), nl = iso ? 1 : g->d;
    if (g->n == 0) {
        *total = 0.0; *d_lognoise = 0.0; *d_mean = 0.0;
        for (int k = 0; k <= nl; ++k) d_kern[k] = 0.0;
        return 0;
    }
    t_reset(g);
    CHK(ensure_fresh(g));
    CHK(one_time_kernel_setup());
    const int64_t N = g->n, ld = g->ld;
    const int T = row_tiles(g), NP = g->d + 3;
    layout::LooWs w;
    CHK(ensure_loo(g, &w));
    HIPCHK(g->dZ.reserve((size_t)ld * ld, g->stream));
    CHK(loo_values(g, w));
    t_begin(g, "loo_b");
    CHK(launch_rows_trimv(g, g->dW, N, w.q, 1, w.t, 0));    // b = cK^-1 q = W'(W q), as alpha
    CHK(launch_rows_trimv(g, g->dWT, N, w.t, 1, w.b, 1));
    t_end(g);
    CHK(kinv_into_scratch(g));
    t_begin(g, "loo_m");
    {
        // Z = cK^-1 diag(sqrt c) over the whole padded square, then M = Z Z' over the full contraction range into the lower
        // 128-tiles of dS (cK^-1 is dead once Z exists)
        const unsigned nt = (unsigned)(T * (TILE / 64));
        hipLaunchKernelGGL(k_loo_scale, dim3(nt, nt), dim3(256), 0, g->stream, g->dS, ld, N, w.sc, g->dZ);
        HIPCHK(hipGetLastError());
        GemmNTParams p{};
        p.A = g->dZ; p.lda = ld; p.B = g->dZ; p.ldb = ld; p.C = g->dS; p.ldc = ld;
        p.mt = T; p.nt64 = 2 * T; p.kc = T * (TILE / KC); p.alpha = 1.0; p.beta = 0.0; p.diag_skip = 1; p.row0 = 0; p.col0 = 0;
        CHK(launch_gemm_nt(g, p));
    }
    t_end(g);
    t_begin(g, "dloo_reduce");
    const int rpb = 32;
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)((N + rpb - 1) / rpb));
    const int64_t nblocks = (int64_t)grid.x * grid.y;
    HIPCHK(g->ddmll_parts.reserve((size_t)nblocks * NP, g->stream));
    const KernelHyper hp = make_hyper(g);
    const double noise_var = std::exp(2.0 * g->lognoise);
    dispatch_dt(g->d, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        LAUNCH_FAM(fam_low(hp), (k_dloo_parts<DT, true>), (k_dloo_parts<DT, false>), grid, dim3(256), 0, g->stream, g->dX, N, hp, noise_var,
                   g->dS, ld, g->dalpha, w.b, rpb, g->ddmll_parts);
    });
    const int nout = nl + 3;
    hipLaunchKernelGGL(k_dmll_final, dim3(nout), dim3(256), 0, g->stream, g->ddmll_parts, nblocks, NP, g->d, iso, w.out + 1);
    HIPCHK(hipGetLastError());
    t_end(g);
    double h[DMAX + 4];
    HIPCHK(hipMemcpyAsync(h, w.out, 8 * (size_t)(nout + 1), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    *total = h[0]; *d_lognoise = h[1]; *d_mean = h[2];
    for (int k = 0; k <= nl; ++k) d_kern[k] = h[3 + k];
    return 0;
}

// ---- batched marginal likelihood (include/bohip_fit.h, kernels_fit.hip) ---------------------------------------------------------
static constexpr size_t FIT_WS_CAP_BYTES = (size_t)1 << 30;
// The observations as the device holds them: the batched fit and the marginalised acquisitions read dX / dy and nothing else of
// the model, and never refit.
static int ensure_observations_resident(bohip_gp* g) {
    if (g->dL == nullptr || g->cap < g->n) CHK(alloc_model(g, std::max<int64_t>(g->n, 1)));
    if (g->mirror_dirty) {
        HIPCHK(hipMemcpyAsync(g->dX, g->hX.data(), (size_t)g->n * g->d * 8, hipMemcpyHostToDevice, g->stream));
        HIPCHK(hipMemcpyAsync(g->dy, g->hy.data(), (size_t)g->n * 8, hipMemcpyHostToDevice, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        g->mirror_dirty = false;
    }
    return 0;
}
// The shapes of those calls: P parameters a setting, the padded order M and leading dimension ld of a setting's slab of `slab`
// doubles, and Hc settings a launch -- what the workspace cap (BOHIP_FIT_WS_MAX_MB) and the launch itself (per_launch: H, or
// min(H, 65535) where the settings are the y dimension of a grid) allow.
struct FitPlan { int iso, P, M, ld; size_t slab; int64_t Hc; };
static FitPlan fit_plan(const bohip_gp* g, int64_t per_launch) {
    FitPlan p;
    p.iso = kern_iso(g->kern); p.P = 2 + (p.iso ? 2 : g->d + 1);
    p.M = (int)round_up(g->n, FIT_NB); p.ld = p.M + 8;
    p.slab = (size_t)(2 * p.M + 1) * p.ld;
    size_t cap = FIT_WS_CAP_BYTES;
    if (const char* e = getenv("BOHIP_FIT_WS_MAX_MB")) cap = std::min(cap, (size_t)std::max(1, atoi(e)) << 20);
    p.Hc = std::max<int64_t>(1, std::min<int64_t>(per_launch, (int64_t)(cap / (p.slab * 8))));
    return p;
}
static int ensure_fit_ws(bohip_gp* g, const FitPlan& p) {
    HIPCHK(g->fit_ws.reserve((size_t)p.Hc * p.slab, g->stream));
    return 0;
}
// the block of bohip_gp_score_ens and, with its two gradient members, of bohip_gp_score_ens_grad (layout::ens_io)
static int ensure_ens_io(bohip_gp* g, int64_t H, int P, int64_t Rc, int64_t R, int64_t nblk, bool with_grad, layout::EnsIo<Best>* io) {
    auto lay = [&](const void* base) {
        return layout::ens_io(base, (size_t)H, (size_t)P, (size_t)Rc, (size_t)g->d, (size_t)R, (size_t)nblk, with_grad ? (size_t)g->d : 0, io);
    };
    HIPCHK(g->ens_io.reserve(lay(nullptr), g->stream));
    lay(g->ens_io);
    return 0;
}
extern "C++" {
// What every kernel over settings reads, for the settings from h0 on: the observations, the launch's rows of theta and pivot (of the
// call's io block), the slabs and the plan's shapes -- on any of FitArgs, EnsFactorArgs, EnsScoreArgs, EnsGradArgs (y where it has one)
template <class A, class = void>
struct has_y : std::false_type {};
template <class A>
struct has_y<A, std::void_t<decltype(std::declval<A&>().y)>> : std::true_type {};
template <class A>
static void fill_fit_args(A& a, const bohip_gp* g, const FitPlan& pl, const double* d_theta, long long* d_pivot, int64_t h0) {
    a.X = g->dX; a.theta = d_theta + (size_t)h0 * pl.P; a.ws = g->fit_ws; a.pivot = d_pivot + h0;
    if constexpr (has_y<A>::value) a.y = g->dy;
    a.slab = (long long)pl.slab; a.N = (int)g->n; a.M = pl.M; a.ld = pl.ld; a.d = g->d; a.fam = kern_family(g->kern); a.iso = pl.iso; a.P = pl.P;
}
template <int DT, bool LOO>
static int fit_launch(bohip_gp* g, const FitArgs& a, int64_t Hc) {
    static bool done[64] = {false};
    CHK(once_per_device(done, g->device, [&]() -> int {
        const int most = (int)fit_lds_bytes(BOHIP_FIT_NMAX, DT);
        HIPCHK(hipFuncSetAttribute((const void*)k_mll_batch<DT, true, LOO>, hipFuncAttributeMaxDynamicSharedMemorySize, most));
        HIPCHK(hipFuncSetAttribute((const void*)k_mll_batch<DT, false, LOO>, hipFuncAttributeMaxDynamicSharedMemorySize, most));
        return 0;
    }));
    LAUNCH_FAM(fam_low(a.fam), (k_mll_batch<DT, true, LOO>), (k_mll_batch<DT, false, LOO>), dim3((unsigned)Hc), dim3(FIT_THREADS),
               fit_lds_bytes(a.M, DT), g->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
}   // extern "C++"

int bohip_gp_mll_batch_dims(bohip_gp* g, int64_t* P, int64_t* nmax) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    if (P) *P = 2 + (kern_iso(g->kern) ? 2 : g->d + 1);
    if (nmax) *nmax = BOHIP_FIT_NMAX;
    return 0;
}

// Both batched objectives (bohip_gp_mll_grad_batch, and with loo bohip_gp_loo_grad_batch of include/bohip_loo_batch.h): the plan, the
// workspace, theta up, one launch per Hc settings, the rows down.  value: mll[H] or total[H]; logp: leave-one-out only.
static int fit_batch(bohip_gp* g, bool loo, int64_t H, const double* theta, double* value, double* grad, double* logp, int64_t* pivot) {
    if (!g || !theta || !value) return fail(BOHIP_E_ARG, "null argument");
    CHK(refuse_weighted(g, loo ? "bohip_gp_loo_grad_batch" : "bohip_gp_mll_grad_batch"));
    if (H < 1) return fail(BOHIP_E_ARG, "H must be >= 1");
    if (g->n == 0) return fail(BOHIP_E_STATE, "no observations");
    if (g->n > BOHIP_FIT_NMAX)
        return fail(BOHIP_E_UNSUPPORTED, std::string("the batched ") + (loo ? "leave-one-out objective" : "marginal likelihood") + " takes at most " +
                                             std::to_string(BOHIP_FIT_NMAX) + " observations, the model has " + std::to_string(g->n) + " (" +
                                             (loo ? "bohip_gp_loo_grad" : "bohip_gp_mll_grad") + " has no limit)");
    HIPCHK(hipSetDevice(g->device));
    CHK(ensure_observations_resident(g));
    const FitPlan pl = fit_plan(g, H);
    const int P = pl.P;
    const int64_t Hc = pl.Hc, N = g->n;
    g->ens_factor_ok = false;   // (the slabs are about to be written)
    CHK(ensure_fit_ws(g, pl));
    layout::FitIo io;
    HIPCHK(g->fit_io.reserve(layout::fit_io(nullptr, (size_t)H, (size_t)P, FIT_STAGES, &io), g->stream));
    layout::fit_io(g->fit_io, (size_t)H, (size_t)P, FIT_STAGES, &io);
    layout::LooBatchIo lio{nullptr};
    if (logp) {
        HIPCHK(g->loo_batch_io.reserve(layout::loo_batch_io(nullptr, (size_t)H, (size_t)N, &lio), g->stream));
        layout::loo_batch_io(g->loo_batch_io, (size_t)H, (size_t)N, &lio);
    }
    double *d_theta = io.theta, *d_value = io.mll, *d_grad = io.grad;
    long long* d_pivot = io.pivot;
    unsigned long long* d_stamps = io.stamps;
    const bool trace = getenv("BOHIP_FIT_TRACE") != nullptr;   // tools: the stage times of the first workgroup on stderr
    HIPCHK(hipMemcpyAsync(d_theta, theta, (size_t)H * P * 8, hipMemcpyHostToDevice, g->stream));
    for (int64_t h0 = 0; h0 < H; h0 += Hc) {
        FitArgs a{};
        fill_fit_args(a, g, pl, d_theta, d_pivot, h0);
        a.mll = d_value + h0;
        a.grad = grad ? d_grad + (size_t)h0 * P : nullptr;
        a.logp = logp ? lio.logp + (size_t)h0 * N : nullptr;
        a.stamps = (trace && h0 == 0) ? d_stamps : nullptr;
        const int64_t hc = std::min(Hc, H - h0);
        CHK(dispatch_dt(g->d, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            return loo ? fit_launch<DT, true>(g, a, hc) : fit_launch<DT, false>(g, a, hc);
        }));
    }
    HIPCHK(hipMemcpyAsync(value, d_value, (size_t)H * 8, hipMemcpyDeviceToHost, g->stream));
    if (grad) HIPCHK(hipMemcpyAsync(grad, d_grad, (size_t)H * P * 8, hipMemcpyDeviceToHost, g->stream));
    if (logp) HIPCHK(hipMemcpyAsync(logp, lio.logp, (size_t)H * N * 8, hipMemcpyDeviceToHost, g->stream));
    if (pivot) {
        static_assert(sizeof(long long) == sizeof(int64_t), "pivot words");
        HIPCHK(hipMemcpyAsync(pivot, d_pivot, (size_t)H * 8, hipMemcpyDeviceToHost, g->stream));
    }
    unsigned long long st[FIT_STAGES] = {0};
    if (trace) HIPCHK(hipMemcpyAsync(st, d_stamps, sizeof(st), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (trace) {   // wall_clock64 ticks at 100 MHz; a stage that did not run (value only, failed row) keeps its old stamp
        auto us = [&](int i) { return st[i] >= st[i - 1] ? (double)(st[i] - st[i - 1]) * 0.01 : 0.0; };
        if (loo)
            std::fprintf(stderr, "bohip loo stages N=%lld d=%d H=%lld us: build %.1f chol %.1f value %.1f inverse %.1f product %.1f grad %.1f\n",
                         (long long)g->n, g->d, (long long)H, us(1), us(2), us(3), us(4), grad ? us(5) : 0.0, grad ? us(6) : 0.0);
        else
            std::fprintf(stderr, "bohip fit stages N=%lld d=%d H=%lld us: build %.1f chol %.1f value %.1f inverse %.1f grad %.1f\n", (long long)g->n,
                         g->d, (long long)H, us(1), us(2), us(3), grad ? us(4) : 0.0, grad ? us(5) : 0.0);
    }
    return 0;
}

int bohip_gp_mll_grad_batch(bohip_gp* g, int64_t H, const double* theta, double* mll, double* grad, int64_t* pivot) {
    return fit_batch(g, false, H, theta, mll, grad, nullptr, pivot);
}

int bohip_gp_loo_grad_batch(bohip_gp* g, int64_t H, const double* theta, double* total, double* grad, double* logp, int64_t* pivot) {
    return fit_batch(g, true, H, theta, total, grad, logp, pivot);
}

// ---- acquisition marginalised over hyper-parameter settings (include/bohip_ens.h, kernels_ens.hip) --------------------------------
extern "C++" {
template <int DT>
static int ens_attrs(bohip_gp* g) {
    static bool done[64] = {false};
    return once_per_device(done, g->device, [&]() -> int {
        const int f = (int)fit_lds_bytes(BOHIP_FIT_NMAX, DT), s = (int)ens_score_lds_bytes(BOHIP_FIT_NMAX, DT);
        HIPCHK(hipFuncSetAttribute((const void*)k_ens_factor<DT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, f));
        HIPCHK(hipFuncSetAttribute((const void*)k_ens_factor<DT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, f));
        HIPCHK(hipFuncSetAttribute((const void*)k_ens_score<DT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, s));
        HIPCHK(hipFuncSetAttribute((const void*)k_ens_score<DT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, s));
        return 0;
    });
}
template <int DT>
static int ens_factor_launch(bohip_gp* g, const EnsFactorArgs& a, int64_t Hc) {
    CHK(ens_attrs<DT>(g));
    LAUNCH_FAM(fam_low(a.fam), (k_ens_factor<DT, true>), (k_ens_factor<DT, false>), dim3((unsigned)Hc), dim3(FIT_THREADS), fit_lds_bytes(a.M, DT),
               g->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
template <int DT>
static int ens_score_launch(bohip_gp* g, const EnsScoreArgs& a, int64_t Hc) {
    CHK(ens_attrs<DT>(g));
    const dim3 grid((unsigned)((a.R + ENS_TC - 1) / ENS_TC), (unsigned)Hc);
    LAUNCH_FAM(fam_low(a.fam), (k_ens_score<DT, true>), (k_ens_score<DT, false>), grid, dim3(ENS_THREADS), ens_score_lds_bytes(a.M, DT), g->stream,
               a);
    HIPCHK(hipGetLastError());
    return 0;
}
// the gradient's launch (include/bohip_ens_grad.h, kernels_ens.hip: k_ens_alpha, k_ens_grad, k_ens_reduce_grad)
template <int DT>
static int ens_grad_launch(bohip_gp* g, const EnsGradArgs& a, int64_t Hc) {
    static bool done[64] = {false};
    CHK(once_per_device(done, g->device, [&]() -> int {
        const int s = (int)ens_grad_lds_bytes(BOHIP_FIT_NMAX, DT);
        HIPCHK(hipFuncSetAttribute((const void*)k_ens_grad<DT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, s));
        HIPCHK(hipFuncSetAttribute((const void*)k_ens_grad<DT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, s));
        return 0;
    }));
    const dim3 grid((unsigned)((a.R + ENS_TC - 1) / ENS_TC), (unsigned)Hc);
    LAUNCH_FAM(fam_low(a.fam), (k_ens_grad<DT, true>), (k_ens_grad<DT, false>), grid, dim3(ENS_THREADS), ens_grad_lds_bytes(a.M, DT), g->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
}   // extern "C++"

// The one driver of bohip_gp_score_ens (with_grad false: grad and each_grad are not read) and bohip_gp_score_ens_grad: the checks, the
// plan, the factor step, the candidate-chunk loop, the reduce tail, the copies and the alive / NOTPD epilogue.  The gradient form adds
// ens_alpha (k_ens_alpha after every factor launch), d more planes a candidate, k_ens_grad for k_ens_score, k_ens_reduce_grad, two
// outputs -- and the factor reuse: it alone remembers the factors it leaves (resident settings only) and skips the factor step on a
// call with the same observations and byte-identical theta.  The value form clears that memory and never sets it.
static int ens_drive(bohip_gp* g, bool with_grad, int acq_id, const double* acq_params, int64_t H, const double* theta, const double* weights,
                     const double* xs, int64_t R, double* scores, double* grad, double* each, double* each_grad, double* mu, double* var,
                     int64_t* pivot, bohip_best* best) {
    if (!g || !theta || !xs || !best || (with_grad && !grad)) return fail(BOHIP_E_ARG, "null argument");
    CHK(refuse_weighted(g, with_grad ? "bohip_gp_score_ens_grad" : "bohip_gp_score_ens"));
    if (H < 1) return fail(BOHIP_E_ARG, "H must be >= 1");
    if (R < 1) return fail(BOHIP_E_ARG, "R must be >= 1");
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "unknown acq_id (Thompson draws are not averaged)");
    AcqParams ap;
    CHK(make_acq(acq_id, acq_params, &ap));
    if (weights) {
        double s = 0.0;
        for (int64_t h = 0; h < H; ++h) {
            if (!(weights[h] >= 0.0 && weights[h] < INFINITY)) return fail(BOHIP_E_ARG, "weights must be finite and >= 0");
            s += weights[h];
        }
        if (!(s > 0.0)) return fail(BOHIP_E_ARG, "the weights sum to 0");
    }
    if (g->n == 0) return fail(BOHIP_E_STATE, "no observations");
    if (g->n > BOHIP_FIT_NMAX)
        return fail(BOHIP_E_UNSUPPORTED, "the marginalised acquisition takes at most " + std::to_string(BOHIP_FIT_NMAX) + " observations, the model has " +
                                             std::to_string(g->n));
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_observations_resident(g));
    const FitPlan pl = fit_plan(g, std::min<int64_t>(H, 65535));   // (settings are the y dimension of the score kernels' grid)
    const int P = pl.P, M = pl.M, d = g->d;
    const int64_t Hc = pl.Hc;
    const bool resident = H <= Hc;   // every setting's factor fits the workspace at once: factor once, before the candidate chunks
    // the slabs hold these very factors: every setting at once, left by a gradient call for byte-identical theta and the same
    // observations (M follows from the observations; the kernel and d of a handle never change)
    const bool reuse = with_grad && resident && g->ens_factor_ok && g->ens_version == g->data_version &&
                       g->ens_theta.size() == (size_t)H * P && g->ens_pivot.size() == (size_t)H &&
                       std::memcmp(g->ens_theta.data(), theta, (size_t)H * P * 8) == 0;
    g->ens_factor_ok = false;   // (the slabs are about to be written; whatever fails below: the next call factors)
    CHK(ensure_fit_ws(g, pl));   // (never grows on a reuse: the same theta and M ask for the same bytes)
    if (with_grad) HIPCHK(g->ens_alpha.reserve((size_t)Hc * M, g->stream));
    // candidates per chunk: the H x Rc planes -- each, mu, var and with the gradient its d components -- stay within 64 MiB (at least
    // one tile, at most 16384 candidates)
    const int64_t planes = with_grad ? 3 + (int64_t)d : 3;
    const int64_t Rc = std::min<int64_t>(
        round_up(R, ENS_TC), std::max<int64_t>(ENS_TC, std::min<int64_t>(16384, (((int64_t)64 << 20) / (8 * planes * H)) / ENS_TC * ENS_TC)));
    int64_t nblk = 0;
    for (int64_t r0 = 0; r0 < R; r0 += Rc) nblk += (std::min(Rc, R - r0) + 255) / 256;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(Best) == 16, "pivot words, records");
    layout::EnsIo<Best> io;
    CHK(ensure_ens_io(g, H, P, Rc, R, nblk, with_grad, &io));
    HIPCHK(hipMemcpyAsync(io.theta, theta, (size_t)H * P * 8, hipMemcpyHostToDevice, g->stream));
    if (weights) HIPCHK(hipMemcpyAsync(io.w, weights, (size_t)H * 8, hipMemcpyHostToDevice, g->stream));
    if (reuse) HIPCHK(hipMemcpyAsync(io.pivot, g->ens_pivot.data(), (size_t)H * 8, hipMemcpyHostToDevice, g->stream));
    auto factor = [&](int64_t h0, int64_t hc) -> int {
        EnsFactorArgs a{};
        fill_fit_args(a, g, pl, io.theta, io.pivot, h0);
        t_begin(g, "ens_factor");
        CHK(dispatch_dt(d, [&](auto dt) { return ens_factor_launch<decltype(dt)::value>(g, a, hc); }));
        t_end(g);
        if (!with_grad) return 0;
        t_begin(g, "ens_alpha");
        hipLaunchKernelGGL(k_ens_alpha, dim3((unsigned)hc), dim3(256), 0, g->stream, g->fit_ws, io.pivot + h0, g->ens_alpha, (long long)pl.slab, M,
                           pl.ld);
        HIPCHK(hipGetLastError());
        t_end(g);
        return 0;
    };
    if (resident && !reuse) CHK(factor(0, H));
    int64_t blk0 = 0;
    for (int64_t r0 = 0; r0 < R; r0 += Rc) {
        const int64_t rc = std::min(Rc, R - r0);
        HIPCHK(hipMemcpyAsync(io.xs, xs + (size_t)r0 * d, (size_t)rc * d * 8, hipMemcpyHostToDevice, g->stream));
        for (int64_t h0 = 0; h0 < H; h0 += Hc) {
            const int64_t hc = std::min(Hc, H - h0);
            if (!resident) CHK(factor(h0, hc));
            EnsGradArgs a{};   // (k_ens_score takes its EnsScoreArgs base)
            fill_fit_args(a, g, pl, io.theta, io.pivot, h0);
            a.xs = io.xs; a.each = io.each + (size_t)h0 * Rc; a.mu = io.mu + (size_t)h0 * Rc; a.var = io.var + (size_t)h0 * Rc;
            a.ldr = Rc; a.R = rc; a.ap = ap;
            if (with_grad) { a.alpha = g->ens_alpha; a.geach = io.geach + (size_t)h0 * Rc * d; }
            t_begin(g, with_grad ? "ens_grad" : "ens_score");
            CHK(dispatch_dt(d, [&](auto dt) {
                return with_grad ? ens_grad_launch<decltype(dt)::value>(g, a, hc) : ens_score_launch<decltype(dt)::value>(g, a, hc);
            }));
            t_end(g);
        }
        t_begin(g, "ens_reduce");
        if (r0 == 0) hipLaunchKernelGGL(k_ens_weights, dim3(1), dim3(64), 0, g->stream, weights ? io.w : nullptr, io.pivot, (long long)H, io.wt);
        const int nb256 = (int)((rc + 255) / 256);
        hipLaunchKernelGGL(k_ens_reduce, dim3(nb256), dim3(256), 0, g->stream, io.each, (long long)Rc, io.wt, (long long)H, (long long)rc,
                           (long long)r0, io.scores, io.blk + blk0);
        if (with_grad)
            hipLaunchKernelGGL(k_ens_reduce_grad, dim3((unsigned)((rc * d + 255) / 256)), dim3(256), 0, g->stream, io.geach, (long long)(Rc * d),
                               io.wt, (long long)H, (long long)(rc * d), io.grad + (size_t)r0 * d);
        HIPCHK(hipGetLastError());
        t_end(g);
        blk0 += nb256;
        for (auto pr : {std::make_pair(each, io.each), std::make_pair(mu, io.mu), std::make_pair(var, io.var)})
            if (pr.first)
                HIPCHK(hipMemcpy2DAsync(pr.first + r0, (size_t)R * 8, pr.second, (size_t)Rc * 8, (size_t)rc * 8, (size_t)H, hipMemcpyDeviceToHost,
                                        g->stream));
        if (with_grad && each_grad)
            HIPCHK(hipMemcpy2DAsync(each_grad + (size_t)r0 * d, (size_t)R * d * 8, io.geach, (size_t)Rc * d * 8, (size_t)rc * d * 8, (size_t)H,
                                    hipMemcpyDeviceToHost, g->stream));
        if (r0 + Rc < R) HIPCHK(hipStreamSynchronize(g->stream));   // the chunk's planes and d_xs are free again
    }
    t_begin(g, "ens_reduce");
    hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, io.blk, (int)nblk, io.best, 0LL);
    HIPCHK(hipGetLastError());
    t_end(g);
    std::vector<long long> hpiv((size_t)H);
    Best hb{-INFINITY, -1};
    HIPCHK(hipMemcpyAsync(hpiv.data(), io.pivot, (size_t)H * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(&hb, io.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    if (scores) HIPCHK(hipMemcpyAsync(scores, io.scores, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (with_grad) HIPCHK(hipMemcpyAsync(grad, io.grad, (size_t)R * d * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    if (with_grad && resident) {   // the slabs and alpha now hold every setting's factor
        g->ens_theta.assign(theta, theta + (size_t)H * P);
        g->ens_pivot = hpiv;
        g->ens_version = g->data_version;
        g->ens_factor_ok = true;
    }
    if (pivot) for (int64_t h = 0; h < H; ++h) pivot[h] = hpiv[(size_t)h];
    double alive_w = 0.0;
    int64_t alive = 0;
    for (int64_t h = 0; h < H; ++h)
        if (hpiv[(size_t)h] == 0) { ++alive; alive_w += weights ? weights[h] : 1.0; }
    if (alive == 0 || !(alive_w > 0.0)) {
        best->val = -INFINITY; best->idx = -1;
        if (scores) for (int64_t j = 0; j < R; ++j) scores[j] = NAN;
        if (with_grad) for (int64_t j = 0; j < R * d; ++j) grad[j] = NAN;
        return fail(BOHIP_E_NOTPD, alive == 0 ? "the factorisation failed at every hyper-parameter setting"
                                              : "the factorisation failed at every hyper-parameter setting of positive weight");
    }
    best->val = hb.val; best->idx = hb.idx;
    return 0;
}

int bohip_gp_score_ens(bohip_gp* g, int acq_id, const double* acq_params, int64_t H, const double* theta, const double* weights,
                       const double* xs, int64_t R, double* scores, double* each, double* mu, double* var, int64_t* pivot,
                       bohip_best* best) {
    return ens_drive(g, false, acq_id, acq_params, H, theta, weights, xs, R, scores, nullptr, each, nullptr, mu, var, pivot, best);
}

int bohip_gp_score_ens_grad(bohip_gp* g, int acq_id, const double* acq_params, int64_t H, const double* theta, const double* weights,
                            const double* xs, int64_t R, double* scores, double* grad, double* each, double* each_grad, double* mu,
                            double* var, int64_t* pivot, bohip_best* best) {
    if (!grad) return fail(BOHIP_E_ARG, "null argument");
    return ens_drive(g, true, acq_id, acq_params, H, theta, weights, xs, R, scores, grad, each, each_grad, mu, var, pivot, best);
}

int bohip_gp_predict_dev(bohip_gp* g, const double* dXs, int64_t R, double* d_mu, double* d_var) {
    if (!g || !dXs || R < 0) return fail(BOHIP_E_ARG, "bad arguments");
    if (R == 0) return 0;
    HIPCHK(hipSetDevice(g->device));
    return score_core(g, BOHIP_ACQ_MAXMEAN, nullptr, dXs, R, d_mu, d_var, nullptr, nullptr);
}

int bohip_gp_score_dev(bohip_gp* g, int acq_id, const double* acq_params, const double* dXs, int64_t R,
                       double* d_score, bohip_best* d_best) {
    if (!g || !dXs || R < 0) return fail(BOHIP_E_ARG, "bad arguments");
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "unknown acq_id");
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    if (R == 0) {
        if (d_best) {
            Best b{-INFINITY, -1};
            HIPCHK(hipMemcpyAsync(d_best, &b, sizeof(b), hipMemcpyHostToDevice, g->stream));
            HIPCHK(hipStreamSynchronize(g->stream));
        }
        return 0;
    }
    return score_core(g, acq_id, acq_params, dXs, R, nullptr, nullptr, d_score, reinterpret_cast<Best*>(d_best));
}

// Candidates of a small host call (R <= SMALL_R): the kernels read them straight from the pinned, device-visible block -- no copy
// command in front of the scoring pass (measured, same box, alternating: bohip_gp_predict 46.6 -> 45.2 us, bohip_gp_score_grad 63.5 -> 59.8 us at
// N = 3000; polling hipStreamQuery before the blocking synchronisation: no difference beyond the 43-51 us run-to-run spread).
// Every caller synchronises the stream before it returns, so the block is free again at the next call.
static const double* small_candidates_in_place(bohip_gp* g, const double* Xs, int64_t R) {
    if (!g->hpin || R > SMALL_R || g->d > DMAX || !g_small_zero_copy) return nullptr;
    std::memcpy(g->pin.cand, Xs, (size_t)R * g->d * 8);
    return g->pin.cand;
}

int bohip_gp_predict(bohip_gp* g, const double* Xs, int64_t R, double* mu, double* var) {
    if (!g || R < 0 || (R > 0 && (!Xs || !mu || !var))) return fail(BOHIP_E_ARG, "bad arguments");
    if (R == 0) return 0;
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    const double* xin = small_candidates_in_place(g, Xs, R);
    if (!xin) HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    if (R <= SMALL_R && g->hpin) {   // results land in pinned host memory, no copy commands
        double *pmu = g->pin.mu, *pvar = g->pin.var;
        CHK(score_core(g, BOHIP_ACQ_MAXMEAN, nullptr, xin ? xin : g->dXs, R, pmu, pvar, nullptr, nullptr));
        HIPCHK(hipStreamSynchronize(g->stream));
        std::memcpy(mu, pmu, (size_t)R * 8);
        std::memcpy(var, pvar, (size_t)R * 8);
        t_collect(g);
        return 0;
    }
    CHK(score_core(g, BOHIP_ACQ_MAXMEAN, nullptr, g->dXs, R, g->dmu, g->dvar, nullptr, nullptr));
    HIPCHK(hipMemcpyAsync(mu, g->dmu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(var, g->dvar, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// Stages shared by bohip_gp_predict_cov and bohip_gp_sample_joint: K*', V' = K*'W' (stored), V'V on the MFMA engine (lower
// 128-tiles of dVV, leading dimension cov_ld).  `who` names the caller in the message of the one-chunk limit.
static int posterior_vv(bohip_gp* g, const double* Xs, int64_t R, const char* who, PassPlan* plan) {   // *plan: the pass that ran
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_fresh(g));
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    const PassPlan pl = *plan = choose_route(g, R, WHOLE_K_ONLY);
    if (R > pl.chunk)
        return fail(BOHIP_E_UNSUPPORTED, std::string(who) + ": R exceeds one candidate chunk (" + std::to_string(chunk_cap(g)) + ")");
    CHK(ensure_grad_scratch(g));
    CHK(one_time_kernel_setup());
    const int64_t Rp = round_up(R, TILE);
    const int T = pl.dm.T, CT = (int)(Rp / TILE);
    {
        bool grew = false;
        HIPCHK(g->dVV.reserve((size_t)Rp * Rp, g->stream));
        HIPCHK(g->dcov.reserve((size_t)Rp * Rp, g->stream, Grow::Exact, &grew));
        if (grew) g->cov_ld = Rp;   // (a smaller call keeps the leading dimension the buffers were made for)
    }
    const KernelHyper hp = make_hyper(g);
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    const int64_t chunks = chunk_pass(g, pl, g->dXs, hp, ChunkV{g->dVT, 0}, false, FuseParams{}, no_finish);   // (one chunk)
    if (chunks < 0) return (int)chunks;
    t_begin(g, "gemm_VV");
    GemmNTParams p{};  // (V'V)[r][s] = sum_i V'[r][i] V'[s][i], lower 128-tiles
    p.A = g->dVT; p.lda = g->ld; p.B = g->dVT; p.ldb = g->ld; p.C = g->dVV; p.ldc = g->cov_ld;
    p.mt = CT; p.nt64 = 2 * CT; p.kc = T * (TILE / KC); p.alpha = 1.0; p.beta = 0.0; p.diag_skip = 1;
    CHK(launch_gemm_nt(g, p));
    t_end(g);
    return 0;
}
// the latent mean of the candidates of posterior_vv -> dmu (dvar: the clamped variance, unused by the joint forms)
static int posterior_mean(bohip_gp* g, const PassPlan& pl) {
    const int64_t R = pl.dm.R;
    AcqParams ap{BOHIP_ACQ_MAXMEAN, 0.0, 0.0};
    hipLaunchKernelGGL(k_score, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, g->stream, g->dq, pl.dm.Rpad, pl.dq_tiles(), g->dmu_raw, R,
                       std::exp(2.0 * g->logsig), g->beta, ap, g->dmu, g->dvar, (double*)nullptr, (Best*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}
// Sigma = K** - V'V of the candidates of posterior_vv into dcov, with the leading dimension ldo
static int launch_post_cov(bohip_gp* g, int64_t R, int64_t ldo) {
    const KernelHyper hp = make_hyper(g);
    dim3 grid((unsigned)((R + 255) / 256), (unsigned)((R + 15) / 16));
    dispatch_dt(g->d, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        LAUNCH_FAM(fam_low(hp), (k_post_cov<DT, true>), (k_post_cov<DT, false>), grid, dim3(256), 0, g->stream, g->dXs, R, hp, g->dVV,
                   g->cov_ld, g->dcov, ldo);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int bohip_gp_predict_cov(bohip_gp* g, const double* Xs, int64_t R, double* mu, double* cov) {
    if (!g || R < 0 || (R > 0 && (!Xs || !mu || !cov))) return fail(BOHIP_E_ARG, "bad arguments");
    if (R == 0) return 0;
    PassPlan pl;
    CHK(posterior_vv(g, Xs, R, "predict_cov", &pl));
    t_begin(g, "post_cov");
    CHK(posterior_mean(g, pl));
    CHK(launch_post_cov(g, R, R));   // (the caller's matrix: R x R, dense)
    t_end(g);
    HIPCHK(hipMemcpyAsync(mu, g->dmu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(cov, g->dcov, (size_t)R * R * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// ---- joint posterior draws over a candidate set (kernels_sample.hip; reference myrand(model, X::Matrix), src/models/gp.jl:7) ----
// the S x R draws (also the matrix bohip_gp_qei_select uploads)
static int ensure_sample_matrix(bohip_gp* g, size_t fneed) {
    HIPCHK(g->sjF.reserve(fneed, g->stream, Grow::Half));
    return 0;
}
static int ensure_thompson(bohip_gp* g, int64_t S) {   // S arg-max records
    HIPCHK(g->dthompson.reserve((size_t)S, g->stream));
    return 0;
}
static int ensure_sample(bohip_gp* g, int64_t Rp, int64_t R, int64_t S, bool want_samples, size_t part_recs) {
    if (g->sj_rows < Rp || !g->sjWT) {   // the four grow together, by half and in whole tiles: sj_rows is also their leading dimension
        const hipStream_t st = g->stream;
        const int64_t rows = std::max<int64_t>(Rp, round_up(g->sj_rows + g->sj_rows / 2, TILE)), ld = rows + 16;
        g->sj_rows = 0;
        const size_t mat = (size_t)ld * ld, inv = (size_t)rows * TILE;
        HIPCHK(hipStreamSynchronize(st));   // all four go before any comes back: the peak stays at one set
        for (DBuf<double>* b : {&g->sjL, &g->sjS, &g->sjW, &g->sjWT}) b->release();
        HIPCHK(g->sjL.reserve(mat, st));
        HIPCHK(g->sjS.reserve(mat, st));
        HIPCHK(g->sjW.reserve(inv, st));
        HIPCHK(g->sjWT.reserve(inv, st));
        // tiles above the diagonal tiles of the matrix, and the far triangles of the diagonal inverses, are never written: zero once
        HIPCHK(hipMemsetAsync(g->sjL, 0, mat * 8, st));
        HIPCHK(hipMemsetAsync(g->sjS, 0, mat * 8, st));
        HIPCHK(hipMemsetAsync(g->sjW, 0, inv * 8, st));
        HIPCHK(hipMemsetAsync(g->sjWT, 0, inv * 8, st));
        g->sj_rows = rows;
    }
    HIPCHK(g->sj_scal.reserve(1, g->stream));
    HIPCHK(g->sj_info.reserve(1, g->stream));
    CHK(ensure_sample_matrix(g, want_samples ? (size_t)S * R : 0));
    HIPCHK(g->sj_part.reserve(part_recs, g->stream, Grow::Half));
    return ensure_thompson(g, S);
}

// The draw itself, shared by bohip_gp_sample_joint and bohip_gp_qei_batch (`who` names the caller in messages).  keepF: the
// draw kernels store the S x R matrix in g->sjF.  `post` enqueues what the caller wants behind the draw kernels of EVERY try --
// before the copies and the try's one synchronisation -- so a call that needs no jitter synchronises once.
extern "C++" {
template <class Post>
static int sample_joint_core(bohip_gp* g, const char* who, const double* Xs, int64_t R, int64_t S, uint64_t seed, double jitter_rel,
                             int max_tries, bool keepF, double* mu, double* chol, double* samples, bohip_best* best,
                             double* jitter_used, int* tries_used, Post&& post) {
    const std::string pre = std::string(who) + ": ";
    if (!(jitter_rel >= 0.0) || !std::isfinite(jitter_rel)) return fail(BOHIP_E_ARG, pre + "jitter_rel must be finite and not negative");
    if (max_tries < 0) return fail(BOHIP_E_ARG, pre + "max_tries must not be negative");
    PassPlan pl;
    CHK(posterior_vv(g, Xs, R, who, &pl));
    const int64_t Rp = round_up(R, TILE);
    const int CT = (int)(Rp / TILE);
    const bool mfma = S >= g_sample_mfma_min;
    const int ntiles = (int)((R + (mfma ? SM_ROWS : SROWS) - 1) / (mfma ? SM_ROWS : SROWS));
    CHK(ensure_sample(g, Rp, R, S, keepF, (size_t)S * ntiles));
    const int64_t ld = g->sj_rows + 16;
    const FactorWs ws{g->sjL, g->sjS, g->sjW, g->sjWT, ld, TILE, (int64_t)TILE * TILE, g->sj_info};
    const KernelHyper hp = make_hyper(g);
    const dim3 cgrid((unsigned)((Rp + 255) / 256), (unsigned)(Rp / 16));
    t_begin(g, "post_cov+jitter");
    CHK(posterior_mean(g, pl));
    dispatch_dt(g->d, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        LAUNCH_FAM(fam_low(hp), (k_sample_cov<DT, true>), (k_sample_cov<DT, false>), cgrid, dim3(256), 0, g->stream, g->dXs, R, Rp, hp,
                   g->dVV, g->cov_ld, g->dcov, g->cov_ld, ws.L, ld);
    });
    hipLaunchKernelGGL(k_sample_diagmax, dim3(1), dim3(256), 0, g->stream, g->dcov, g->cov_ld, R, g->sj_scal);
    HIPCHK(hipGetLastError());
    t_end(g);
    double jit = 0.0;
    int tries = 0;
    for (;;) {
        HIPCHK(hipMemsetAsync(g->sj_info, 0, sizeof(int), g->stream));
        if (tries > 0) {   // Sigma is kept (dcov): the workspace again, with the jitter on the diagonal
            t_begin(g, "post_cov+jitter");
            hipLaunchKernelGGL(k_sample_rejit, cgrid, dim3(256), 0, g->stream, g->dcov, g->cov_ld, R, Rp, jit, ws.L, ld);
            HIPCHK(hipGetLastError());
            t_end(g);
        }
        // the launch-chained form, without the inverse queues: only the diagonal inverses the panel solves use.  It touches
        // nothing of the model (no flag block, no refit lock: it has no persistent workgroups).
        t_begin(g, "sample_cholesky");
        CHK(factor_launch_chain(g, ws, CT));
        t_end(g);
        t_begin(g, "sample_draw");
        double* const dF = keepF ? g->sjF : nullptr;
        if (mfma) {
            hipLaunchKernelGGL(k_sample_mfma, dim3((unsigned)ntiles, (unsigned)((S + SM_DRAWS - 1) / SM_DRAWS)), dim3(256), 0, g->stream,
                               ws.L, ld, R, S, seed, g->dmu, dF, g->sj_part, ntiles);
        } else if (S == 1) {
            hipLaunchKernelGGL(k_sample_rows<1>, dim3((unsigned)ntiles, 1), dim3(256), 0, g->stream, ws.L, ld, R, S, seed, g->dmu, dF,
                               g->sj_part, ntiles);
        } else {
            hipLaunchKernelGGL(k_sample_rows<4>, dim3((unsigned)ntiles, (unsigned)((S + 3) / 4)), dim3(256), 0, g->stream, ws.L, ld, R, S,
                               seed, g->dmu, dF, g->sj_part, ntiles);
        }
        hipLaunchKernelGGL(k_sample_best, dim3((unsigned)S), dim3(64), 0, g->stream, g->sj_part, ntiles, g->dthompson);
        HIPCHK(hipGetLastError());
        t_end(g);
        CHK(post());
        // everything the caller asked for is copied behind the kernels, so a call that needs no jitter synchronises once
        int info = 0;
        double scale = 0.0;
        HIPCHK(hipMemcpyAsync(&info, g->sj_info, sizeof(int), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipMemcpyAsync(&scale, g->sj_scal, 8, hipMemcpyDeviceToHost, g->stream));
        if (mu) HIPCHK(hipMemcpyAsync(mu, g->dmu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
        if (best) HIPCHK(hipMemcpyAsync(best, g->dthompson, (size_t)S * sizeof(Best), hipMemcpyDeviceToHost, g->stream));
        if (samples) HIPCHK(hipMemcpyAsync(samples, g->sjF, (size_t)S * R * 8, hipMemcpyDeviceToHost, g->stream));
        if (chol) {   // dVV is free once Sigma exists
            hipLaunchKernelGGL(k_sample_pack, dim3((unsigned)((R + 255) / 256), (unsigned)R), dim3(256), 0, g->stream, ws.L, ld, R, g->dVV);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(chol, g->dVV, (size_t)R * R * 8, hipMemcpyDeviceToHost, g->stream));
        }
        HIPCHK(hipStreamSynchronize(g->stream));
        if (info == 0) break;
        const double next = std::max(10.0 * jit, jitter_rel * scale);
        if (tries >= max_tries || !(next > jit)) {
            g->pivot = info;
            t_collect(g);
            return fail(BOHIP_E_NOTPD, pre + "posterior covariance not positive definite at pivot " + std::to_string(info) +
                                           " (jitter " + std::to_string(jit) + " after " + std::to_string(tries) + " tries)");
        }
        jit = next;
        ++tries;
    }
    if (jitter_used) *jitter_used = jit;
    if (tries_used) *tries_used = tries;
    t_collect(g);
    return 0;
}
}   // extern "C++"

int bohip_gp_sample_joint(bohip_gp* g, const double* Xs, int64_t R, int64_t S, uint64_t seed, double jitter_rel, int max_tries,
                          double* mu, double* chol, double* samples, bohip_best* best, double* jitter_used, int* tries_used) {
    if (!g || !Xs || R < 1 || S < 1) return fail(BOHIP_E_ARG, "sample_joint: bad arguments (R and S must be at least 1)");
    return sample_joint_core(g, "sample_joint", Xs, R, S, seed, jitter_rel, max_tries, samples != nullptr, mu, chol, samples, best,
                             jitter_used, tries_used, [] { return 0; });
}

// ---- greedy Monte-Carlo q-EI over the resident draws (kernels_qei.hip, include/bohip_qei.h) ------------------------
static constexpr size_t QEI_MAX_BYTES = (size_t)8 << 30;   // the S x R matrix plus the partials
static constexpr int64_t QEI_GRID_S = (int64_t)QEI_B * 65535;   // grid.y holds the draw blocks
static int64_t qei_max_draws(int64_t R) {
    // S R + ceil(S / 32) R doubles <= 8 GiB  <=  S (1 + 1/32) R + R
    const double per = 8.0 * (double)R;
    const int64_t s = (int64_t)std::floor(((double)QEI_MAX_BYTES - per) / (per * (1.0 + 1.0 / QEI_B)));
    return std::max<int64_t>(0, std::min(s, QEI_GRID_S));
}
static int qei_check(const char* who, int64_t R, int64_t S, double tau, int64_t q, const void* idx, const void* gain) {
    const std::string pre = std::string(who) + ": ";
    if (!idx || !gain) return fail(BOHIP_E_ARG, pre + "null argument");
    if (R < 1 || S < 1 || q < 1) return fail(BOHIP_E_ARG, pre + "R, S and q must be at least 1");
    if (q > R) return fail(BOHIP_E_ARG, pre + "q exceeds the number of candidates R");
    if (!std::isfinite(tau)) return fail(BOHIP_E_ARG, pre + "tau must be finite");
    return 0;
}
static int qei_check_size(const char* who, int64_t R, int64_t S) {
    if (S > qei_max_draws(R))
        return fail(BOHIP_E_UNSUPPORTED, std::string(who) + ": S x R draws and their partial sums exceed 8 GiB (or 65535 blocks of draws); the "
                                             "largest S at R = " + std::to_string(R) + " is " + std::to_string(qei_max_draws(R)));
    return 0;
}
static int ensure_qei(bohip_gp* g, int64_t R, int64_t S, int64_t q, QeiWs* w) {
    const size_t NB = (size_t)((S + QEI_B - 1) / QEI_B), NT = (size_t)((R + QEI_PICK - 1) / QEI_PICK);
    auto lay = [&](const void* base) { return layout::qei(base, (size_t)S, NB * (size_t)R, NT, (size_t)q, w); };
    HIPCHK(g->qei_ws.reserve(lay(nullptr), g->stream, Grow::Half));
    lay(g->qei_ws);
    return 0;
}
// the q rounds over g->sjF, back to back on the handle's stream, and the two small copies behind them (no synchronisation)
static int qei_rounds(bohip_gp* g, const QeiWs& w, int64_t R, int64_t S, double tau, int64_t q, int64_t* idx, double* gain) {
    static_assert(sizeof(long long) == sizeof(int64_t), "idx crosses as int64_t");
    t_begin(g, "qei_select");
    hipLaunchKernelGGL(k_qei_init, dim3((unsigned)((std::max(S, q) + 255) / 256)), dim3(256), 0, g->stream, w, S, tau, q);
    const dim3 ggrid((unsigned)((R + QEI_COLS - 1) / QEI_COLS), (unsigned)((S + QEI_B - 1) / QEI_B));
    const dim3 pgrid((unsigned)((R + QEI_PICK - 1) / QEI_PICK));
    for (int64_t k = 0; k < q; ++k) {
        hipLaunchKernelGGL(k_qei_gain, ggrid, dim3(QEI_COLS), 0, g->stream, g->sjF, R, S, w);
        hipLaunchKernelGGL(k_qei_pick, pgrid, dim3(QEI_PICK), 0, g->stream, g->sjF, R, S, k, w);
    }
    HIPCHK(hipGetLastError());
    t_end(g);
    HIPCHK(hipMemcpyAsync(idx, w.idx, (size_t)q * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(gain, w.gain, (size_t)q * 8, hipMemcpyDeviceToHost, g->stream));
    return 0;
}

int bohip_gp_qei_batch(bohip_gp* g, const double* Xs, int64_t R, int64_t S, uint64_t seed, double jitter_rel, int max_tries, double tau,
                       int64_t q, int64_t* idx, double* gain, double* samples, double* jitter_used, int* tries_used) {
    if (!g || !Xs) return fail(BOHIP_E_ARG, "qei_batch: null argument");
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");   // (first: the default tau, max y, does not exist then)
    CHK(qei_check("qei_batch", R, S, tau, q, idx, gain));
    CHK(qei_check_size("qei_batch", R, S));
    HIPCHK(hipSetDevice(g->device));
    QeiWs w{};
    CHK(ensure_qei(g, R, S, q, &w));
    return sample_joint_core(g, "qei_batch", Xs, R, S, seed, jitter_rel, max_tries, true, nullptr, nullptr, samples, nullptr, jitter_used,
                             tries_used, [&] { return qei_rounds(g, w, R, S, tau, q, idx, gain); });
}

int bohip_gp_qei_select(bohip_gp* g, const double* samples, int64_t S, int64_t R, double tau, int64_t q, int64_t* idx, double* gain) {
    if (!g || !samples) return fail(BOHIP_E_ARG, "qei_select: null argument");
    CHK(qei_check("qei_select", R, S, tau, q, idx, gain));
    CHK(qei_check_size("qei_select", R, S));
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    QeiWs w{};
    CHK(ensure_qei(g, R, S, q, &w));
    CHK(ensure_sample_matrix(g, (size_t)S * R));
    HIPCHK(hipMemcpyAsync(g->sjF, samples, (size_t)S * R * 8, hipMemcpyHostToDevice, g->stream));
    CHK(qei_rounds(g, w, R, S, tau, q, idx, gain));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// ---- the knowledge gradient over a candidate set (kernels_kg.hip, include/bohip_kg.h) ------------------------------
static_assert(KG_RMAX == BOHIP_KG_RMAX, "the kernel's LDS plan and the header agree");
struct KgWs {
    double* kg;     // [E]
    Best* best;
    int* nseg;      // [E]
    double* a;      // [R]      the caller's lines only
    double* B;      // [E][R]
};
static int kg_check(const char* who, const void* p0, const void* p1, const void* kg, int64_t R, int64_t E) {
    const std::string pre = std::string(who) + ": ";
    if (R < 1 || E < 1) return fail(BOHIP_E_ARG, pre + "R and E must be at least 1");
    if (E > R) return fail(BOHIP_E_ARG, pre + "E exceeds the number of candidates R");
    if (!p0 || !p1 || !kg) return fail(BOHIP_E_ARG, pre + "null argument");
    return 0;
}
static int kg_check_size(const char* who, int64_t R) {
    if (R > BOHIP_KG_RMAX)
        return fail(BOHIP_E_UNSUPPORTED, std::string(who) + ": R exceeds BOHIP_KG_RMAX (" + std::to_string(BOHIP_KG_RMAX) +
                                             "): a point's lines live in one workgroup's LDS");
    return 0;
}
static int ensure_kg(bohip_gp* g, int64_t R, int64_t E, bool lines, KgWs* w) {
    auto lay = [&](const void* base) { return layout::kg(base, (size_t)E, lines ? (size_t)R : 0, w); };
    HIPCHK(g->kg_ws.reserve(lay(nullptr), g->stream, Grow::Half));
    lay(g->kg_ws);
    return 0;
}
// the march of every evaluation point and the record, on the handle's stream, and the small copies behind them (no synchronisation)
static int kg_march(bohip_gp* g, bool scale, const KgWs& w, const double* da, const double* dB, int64_t ldb, int64_t R, int64_t E, double nu,
                    double* kg, int32_t* nseg, bohip_best* best) {
    static_assert(sizeof(int) == sizeof(int32_t), "nseg crosses as int32_t");
    t_begin(g, "kg");
    const dim3 grid((unsigned)E), block(KG_THREADS);
    if (scale) hipLaunchKernelGGL(k_kg<true>, grid, block, kg_lds_bytes(R), g->stream, da, dB, ldb, (int)R, nu, w.kg, w.nseg);
    else hipLaunchKernelGGL(k_kg<false>, grid, block, kg_lds_bytes(R), g->stream, da, dB, ldb, (int)R, nu, w.kg, w.nseg);
    if (best) hipLaunchKernelGGL(k_kg_best, dim3(1), dim3(256), 0, g->stream, w.kg, (int)E, w.best);
    HIPCHK(hipGetLastError());
    t_end(g);
    HIPCHK(hipMemcpyAsync(kg, w.kg, (size_t)E * 8, hipMemcpyDeviceToHost, g->stream));
    if (nseg) HIPCHK(hipMemcpyAsync(nseg, w.nseg, (size_t)E * 4, hipMemcpyDeviceToHost, g->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, w.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    return 0;
}

int bohip_gp_kg(bohip_gp* g, const double* Xs, int64_t R, int64_t E, double* kg, int32_t* nseg, double* mu, bohip_best* best) {
    CHK(kg_check("kg", g, Xs, kg, R, E));
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(kg_check_size("kg", R));
    HIPCHK(hipSetDevice(g->device));
    KgWs w{};
    CHK(ensure_kg(g, R, E, false, &w));
    PassPlan pl;
    CHK(posterior_vv(g, Xs, R, "kg", &pl));
    t_begin(g, "post_cov");
    CHK(posterior_mean(g, pl));
    // Sigma as bohip_gp_predict_cov computes it, with the leading dimension of the buffer (a multiple of 128): every row starts on
    // a 16-byte boundary for k_kg's loads
    CHK(launch_post_cov(g, R, g->cov_ld));
    t_end(g);
    const double nu = std::exp(2.0 * g->lognoise) + std::numeric_limits<double>::epsilon() + g->jitter_last;   // as on cK's diagonal
    CHK(kg_march(g, true, w, g->dmu, g->dcov, g->cov_ld, R, E, nu, kg, nseg, best));
    if (mu) HIPCHK(hipMemcpyAsync(mu, g->dmu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

int bohip_kg_lines(bohip_gp* g, const double* a, const double* B, int64_t R, int64_t E, double* kg, int32_t* nseg) {
    CHK(kg_check("kg_lines", a, B, kg, R, E));
    if (!g) return fail(BOHIP_E_ARG, "kg_lines: null argument");
    CHK(kg_check_size("kg_lines", R));
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(one_time_kernel_setup());
    KgWs w{};
    CHK(ensure_kg(g, R, E, true, &w));
    HIPCHK(hipMemcpyAsync(w.a, a, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(w.B, B, (size_t)E * R * 8, hipMemcpyHostToDevice, g->stream));
    CHK(kg_march(g, false, w, w.a, w.B, R, R, E, 0.0, kg, nseg, nullptr));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// ---- max-value entropy search over a candidate set (kernels_mes.hip, include/bohip_mes.h) --------------------------
static_assert(MES_KMAX == BOHIP_MES_KMAX && MES_RMAX == BOHIP_MES_RMAX, "the kernels' plan and the header agree");
struct MesBufs {
    double *mes, *dmu, *dvar;   // [R] each
    double *maxvals;            // [K]
    double *quant;              // [3]
    double *mu, *var;           // [R] each: the caller's candidates (bohip_mes_values / bohip_mes_gumbel)
    Best *blocks, *best;        // [ceil(R / 256)], [1]
    MesWs w;
};
static int mes_slices(int64_t R) { return R <= MES_SLICE ? 1 : (int)((R + MES_SLICE - 1) / MES_SLICE); }
static int mes_check_size(const char* who, int64_t R, int64_t K) {
    const std::string pre = std::string(who) + ": ";
    if (R < 1 || K < 1) return fail(BOHIP_E_ARG, pre + "R and K must be at least 1");
    return 0;
}
static int mes_check_limits(const char* who, int64_t R, int64_t K) {
    const std::string pre = std::string(who) + ": ";
    if (K > BOHIP_MES_KMAX)
        return fail(BOHIP_E_UNSUPPORTED, pre + "K exceeds BOHIP_MES_KMAX (" + std::to_string(BOHIP_MES_KMAX) +
                                             "): the max values live in a workgroup's LDS");
    if (R > BOHIP_MES_RMAX)
        return fail(BOHIP_E_UNSUPPORTED, pre + "R exceeds BOHIP_MES_RMAX (" + std::to_string(BOHIP_MES_RMAX) +
                                             "): the bracket of the max-value quantiles is guaranteed up to it");
    return 0;
}
// ONE block, see layout::mes
static int ensure_mes(bohip_gp* g, int64_t R, int64_t K, MesBufs* b) {
    const int nsl = mes_slices(R);
    auto lay = [&](const void* base) {
        return layout::mes(base, (size_t)R, (size_t)K, 2 * MES_STATE + 4, (size_t)3 * MES_BR_MAX, (size_t)2 * MES_NQ * MES_PROBES * nsl,
                           (size_t)((R + 255) / 256), b);
    };
    HIPCHK(g->mes_ws.reserve(lay(nullptr), g->stream, Grow::Half));
    lay(g->mes_ws);
    b->w.nsl = nsl;
    return 0;
}
// the Gumbel sampler on the device's (mu, var): bracket, 14 probe passes, the draw (no synchronisation, no copies)
static int mes_gumbel_stages(bohip_gp* g, const MesBufs& b, const double* dmu, const double* dvar, int64_t R, int64_t K, uint64_t seed,
                             double floor_value) {
    const int nbr = (int)std::min<int64_t>(MES_BR_MAX, (R + 255) / 256);
    t_begin(g, "mes_bracket");
    hipLaunchKernelGGL(k_mes_bracket<false>, dim3(nbr), dim3(256), 0, g->stream, dmu, dvar, R, nbr, b.w);
    hipLaunchKernelGGL(k_mes_bracket<true>, dim3(1), dim3(256), 0, g->stream, dmu, dvar, R, nbr, b.w);
    HIPCHK(hipGetLastError());
    t_end(g);
    t_begin(g, "mes_probe");
    const dim3 pgrid(MES_NQ * MES_PROBES, (unsigned)b.w.nsl);
    for (int pass = 0; pass < MES_PASSES; ++pass)
        hipLaunchKernelGGL(k_mes_probe, pgrid, dim3(256), 0, g->stream, dmu, dvar, R, pass, b.w);
    HIPCHK(hipGetLastError());
    t_end(g);
    t_begin(g, "mes_draw");
    hipLaunchKernelGGL(k_mes_draw, dim3(1), dim3(256), 0, g->stream, b.w, (int)K, seed, floor_value, b.quant, b.maxvals);
    HIPCHK(hipGetLastError());
    t_end(g);
    return 0;
}
// the functor over the candidates and the record, and the copies of what the caller asked for (no synchronisation)
static int mes_value_stages(bohip_gp* g, const MesBufs& b, const double* dmu, const double* dvar, int64_t R, int64_t K, bool grad,
                            double* mes, double* gmu, double* gvar, bohip_best* best) {
    const int nb = (int)((R + 255) / 256);
    t_begin(g, "mes_values");
    if (grad)
        hipLaunchKernelGGL(k_mes_values<true>, dim3(nb), dim3(256), 0, g->stream, dmu, dvar, R, b.maxvals, (int)K, b.mes, b.dmu, b.dvar,
                           best ? b.blocks : (Best*)nullptr);
    else
        hipLaunchKernelGGL(k_mes_values<false>, dim3(nb), dim3(256), 0, g->stream, dmu, dvar, R, b.maxvals, (int)K, b.mes, (double*)nullptr,
                           (double*)nullptr, best ? b.blocks : (Best*)nullptr);
    if (best) hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, b.blocks, nb, b.best, 0ll);
    HIPCHK(hipGetLastError());
    t_end(g);
    HIPCHK(hipMemcpyAsync(mes, b.mes, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (grad) {
        HIPCHK(hipMemcpyAsync(gmu, b.dmu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipMemcpyAsync(gvar, b.dvar, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    }
    if (best) HIPCHK(hipMemcpyAsync(best, b.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    return 0;
}

int bohip_gp_mes(bohip_gp* g, const double* Xs, int64_t R, int64_t K, int mode, uint64_t seed, double floor_value, double jitter_rel,
                 int max_tries, double* mes, double* maxvals, double* quantiles, double* mu, double* var, bohip_best* best,
                 double* jitter_used, int* tries_used) {
    CHK(mes_check_size("mes", R, K));
    if (mode != BOHIP_MES_GUMBEL && mode != BOHIP_MES_JOINT) return fail(BOHIP_E_ARG, "mes: unknown mode");
    if (!g || !Xs || !mes) return fail(BOHIP_E_ARG, "mes: null argument");
    if (floor_value != floor_value) return fail(BOHIP_E_ARG, "mes: floor_value must not be NaN");
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(mes_check_limits("mes", R, K));
    HIPCHK(hipSetDevice(g->device));
    if (mode == BOHIP_MES_JOINT && round_up(R, 512) > chunk_cap(g))
        return fail(BOHIP_E_UNSUPPORTED, "mes: joint mode: R exceeds one candidate chunk (" + std::to_string(chunk_cap(g)) + ")");
    MesBufs b{};
    CHK(ensure_mes(g, R, K, &b));
    auto copies = [&]() -> int {
        if (maxvals) HIPCHK(hipMemcpyAsync(maxvals, b.maxvals, (size_t)K * 8, hipMemcpyDeviceToHost, g->stream));
        if (mu) HIPCHK(hipMemcpyAsync(mu, g->dmu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
        if (var) HIPCHK(hipMemcpyAsync(var, g->dvar, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
        return 0;
    };
    if (mode == BOHIP_MES_JOINT) {
        if (quantiles) quantiles[0] = quantiles[1] = quantiles[2] = NAN;
        return sample_joint_core(g, "mes", Xs, R, K, seed, jitter_rel, max_tries, true, nullptr, nullptr, nullptr, nullptr, jitter_used,
                                 tries_used, [&]() -> int {
                                     t_begin(g, "mes_rowmax");
                                     hipLaunchKernelGGL(k_mes_rowmax, dim3((unsigned)K), dim3(256), 0, g->stream, g->sjF, R, floor_value,
                                                        b.maxvals);
                                     HIPCHK(hipGetLastError());
                                     t_end(g);
                                     CHK(mes_value_stages(g, b, g->dmu, g->dvar, R, K, false, mes, nullptr, nullptr, best));
                                     return copies();
                                 });
    }
    t_reset(g);
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    CHK(score_core(g, BOHIP_ACQ_MAXMEAN, nullptr, g->dXs, R, g->dmu, g->dvar, nullptr, nullptr));
    CHK(mes_gumbel_stages(g, b, g->dmu, g->dvar, R, K, seed, floor_value));
    CHK(mes_value_stages(g, b, g->dmu, g->dvar, R, K, false, mes, nullptr, nullptr, best));
    CHK(copies());
    if (quantiles) HIPCHK(hipMemcpyAsync(quantiles, b.quant, 3 * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (jitter_used) *jitter_used = 0.0;
    if (tries_used) *tries_used = 0;
    t_collect(g);
    return 0;
}

int bohip_mes_values(bohip_gp* g, const double* mu, const double* var, int64_t R, const double* maxvals, int64_t K, double* mes,
                     double* dmu, double* dvar, bohip_best* best) {
    CHK(mes_check_size("mes_values", R, K));
    if (!g || !mu || !var || !maxvals || !mes) return fail(BOHIP_E_ARG, "mes_values: null argument");
    if ((dmu == nullptr) != (dvar == nullptr)) return fail(BOHIP_E_ARG, "mes_values: dmu and dvar are given together or not at all");
    CHK(mes_check_limits("mes_values", R, K));
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    MesBufs b{};
    CHK(ensure_mes(g, R, K, &b));
    HIPCHK(hipMemcpyAsync(b.mu, mu, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(b.var, var, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(b.maxvals, maxvals, (size_t)K * 8, hipMemcpyHostToDevice, g->stream));
    CHK(mes_value_stages(g, b, b.mu, b.var, R, K, dmu != nullptr, mes, dmu, dvar, best));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

int bohip_mes_gumbel(bohip_gp* g, const double* mu, const double* var, int64_t R, int64_t K, uint64_t seed, double floor_value,
                     double* quantiles, double* maxvals) {
    CHK(mes_check_size("mes_gumbel", R, K));
    if (!g || !mu || !var || !quantiles || !maxvals) return fail(BOHIP_E_ARG, "mes_gumbel: null argument");
    if (floor_value != floor_value) return fail(BOHIP_E_ARG, "mes_gumbel: floor_value must not be NaN");
    CHK(mes_check_limits("mes_gumbel", R, K));
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    MesBufs b{};
    CHK(ensure_mes(g, R, K, &b));
    HIPCHK(hipMemcpyAsync(b.mu, mu, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(b.var, var, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    CHK(mes_gumbel_stages(g, b, b.mu, b.var, R, K, seed, floor_value));
    HIPCHK(hipMemcpyAsync(quantiles, b.quant, 3 * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(maxvals, b.maxvals, (size_t)K * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// ---- constrained optimisation (kernels_con.hip, include/bohip_con.h) ---------------------------------------------
static_assert(CON_CMAX == BOHIP_CON_CMAX && CON_FEAS == BOHIP_CON_FEASIBILITY, "the kernels' plan and the header agree");
struct ConBufs {
    double *mu, *var, *pmu, *pvar;   // [(C + 1) R] each: the moments and the partials of the score
    double *value, *logfeas;         // [R] each
    double *jmu, *jvar;              // [(C + 1) R d] each: the models' Jacobians (gradient route only)
    double *grad;                    // [R d]
    Best *blocks, *best;             // [CON_GRID_MAX], [1]
};
// ONE block on the handle, see layout::con
static int ensure_con(bohip_gp* g, int64_t C, int64_t R, bool jac, ConBufs* b) {
    auto lay = [&](const void* base) { return layout::con(base, (size_t)(C + 1) * R, (size_t)R, CON_GRID_MAX, jac ? (size_t)g->d : 0, b); };
    HIPCHK(g->con_ws.reserve(lay(nullptr), g->stream, Grow::Half));
    lay(g->con_ws);
    return 0;
}

static int launch_post_grad_any(bohip_gp* g, const double* dXs, int64_t r0, int64_t r1, const KernelHyper& hp, double* d_jmu, double* d_jvar,
                                const double* UT) {
    int S = 1;
    CHK(grad_obs_splits(g, r0, r1, &S));
    dispatch_dt(g->d, [&](auto dt) { launch_post_grad<decltype(dt)::value>(g, dXs, r0, r1, hp, d_jmu, d_jvar, UT, S); });
    HIPCHK(hipGetLastError());
    return 0;
}

// The posterior of R candidates (device pointers) on g's stream: mu, sigma^2 and, with d_jmu, the two Jacobians [r][d].  The routes of
// score_grad_core without its fused small pass (the finish of that pass has the functor inside kernels at their register limit): the
// split-K posterior where split_plan says so, K*' chunks otherwise.  Without d_jmu the same launches less V' / U': the moments of a
// value call are those of a gradient call bit for bit.
static int posterior_grad_core(bohip_gp* g, const double* dXs, int64_t R, double* d_mu, double* d_var, double* d_jmu, double* d_jvar) {
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(ensure_fresh(g));
    CHK(ensure_score_scratch(g, R));
    CHK(one_time_kernel_setup());
    const bool jac = d_jmu != nullptr;
    const PassPlan pl = choose_route(g, R, RouteWants{false, true, Prune::No});
    const KernelHyper hp = make_hyper(g);
    const AcqParams ap{ACQ_MAXMEAN, 0.0, 0.0};
    const double sigma2 = std::exp(2.0 * g->logsig);
    auto finish = [&](int64_t r0, int64_t r1) {
        t_begin(g, "con_post");
        hipLaunchKernelGGL(k_score, dim3((unsigned)((r1 - r0 + 255) / 256)), dim3(256), 0, g->stream, g->dq + r0, pl.dm.Rpad, pl.dq_tiles(),
                           g->dmu_raw + r0, r1 - r0, sigma2, g->beta, ap, d_mu + r0, d_var + r0, (double*)nullptr, (Best*)nullptr);
        HIPCHK(hipGetLastError());
        if (jac) CHK(launch_post_grad_any(g, dXs, r0, r1, hp, d_jmu, d_jvar, g->dUT));
        t_end(g);
        return 0;
    };
    return posterior_then(g, pl, dXs, hp, jac, finish);
}

static int con_make_params(const char* who, int acq_id, const double* acq_params, int64_t C, const double* thresholds, const int* senses,
                           ConParams* cp) {
    const std::string pre = std::string(who) + ": ";
    if (C < 0 || C > BOHIP_CON_CMAX) return fail(BOHIP_E_ARG, pre + "C must be in [0, " + std::to_string(BOHIP_CON_CMAX) + "]");
    if (C > 0 && (!thresholds || !senses)) return fail(BOHIP_E_ARG, pre + "thresholds and senses are required");
    if (acq_id != BOHIP_ACQ_EI && acq_id != BOHIP_ACQ_PI && acq_id != BOHIP_ACQ_LOGEI && acq_id != BOHIP_CON_FEASIBILITY)
        return fail(BOHIP_E_ARG, pre + "acq_id must be EI, PI, LogEI or BOHIP_CON_FEASIBILITY: a signed score has no product form");
    if (acq_id != BOHIP_CON_FEASIBILITY && !acq_params) return fail(BOHIP_E_ARG, pre + "acq_params required for this acquisition");
    *cp = ConParams{};
    cp->acq = acq_id; cp->C = (int)C; cp->p0 = acq_id != BOHIP_CON_FEASIBILITY ? acq_params[0] : 0.0;
    for (int64_t c = 0; c < C; ++c) {
        if (!std::isfinite(thresholds[c])) return fail(BOHIP_E_ARG, pre + "threshold " + std::to_string(c) + " is not finite");
        if (senses[c] != 1 && senses[c] != -1) return fail(BOHIP_E_ARG, pre + "sense " + std::to_string(c) + " must be +1 or -1");
        cp->thr[c] = thresholds[c]; cp->sense[c] = (double)senses[c];
    }
    return 0;
}
// The optional half of a stage's launch (k_con_combine and k_ehvi end in the same arguments), chosen in ONE place: the GRAD
// instantiation with the partials' and the Jacobians' planes where either is asked for, else the plain one with nulls; the gradient
// with jac; the per-block records with want_best.
struct StageOuts {
    bool grad_form;
    double *pmu, *pvar;
    const double *jmu, *jvar;
    int64_t jplane;
    double* grad;
    Best* blocks;
};
static StageOuts stage_outs(const bohip_gp* g, const ConBufs& b, int64_t R, bool partials, bool jac, bool want_best) {
    StageOuts o{};
    o.grad_form = partials || jac;
    if (o.grad_form) { o.pmu = b.pmu; o.pvar = b.pvar; o.jmu = b.jmu; o.jvar = b.jvar; o.jplane = R * g->d; }
    o.grad = jac ? b.grad : nullptr;
    o.blocks = want_best ? b.blocks : nullptr;
    return o;
}
// the end of a stage opened with t_begin: the record of its nb blocks
static int stage_end(bohip_gp* g, const ConBufs& b, int nb, bool want_best) {
    if (want_best) hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, b.blocks, nb, b.best, 0ll);
    HIPCHK(hipGetLastError());
    t_end(g);
    return 0;
}
// the combine and the record on g's stream (no synchronisation, no copies)
static int con_combine_stage(bohip_gp* g, const ConParams& cp, const ConBufs& b, int64_t R, bool partials, bool jac, bool want_best) {
    const int nb = (int)std::min<int64_t>(CON_GRID_MAX, (R + 255) / 256);
    const StageOuts o = stage_outs(g, b, R, partials, jac, want_best);
    t_begin(g, "con_combine");
    hipLaunchKernelGGL(o.grad_form ? k_con_combine<true> : k_con_combine<false>, dim3(nb), dim3(256), 0, g->stream, cp, (const double*)b.mu,
                       (const double*)b.var, R, R, b.value, b.logfeas, o.pmu, o.pvar, o.jmu, o.jvar, o.jplane, g->d, o.grad, o.blocks);
    return stage_end(g, b, nb, want_best);
}

// ---- several models at the same candidates (bohip_gp_score_con, bohip_gp_score_mo) ------------------------------------------------------
static hipError_t event_of(bohip_gp* m) { return m->ev_con ? hipSuccess : hipEventCreateWithFlags(&m->ev_con, hipEventDisableTiming); }

// Row c of b's moments (and, with jac, Jacobians) is the posterior of models[c] at the R candidates Xs (host), every model on its OWN
// stream and with no host wait: the candidates go to the device once, into the owner's dXs on the owner's stream (whatever the caller
// put on that stream before is ahead of them); a handle other than the owner waits for that copy -- and has its timing reset -- at its
// first appearance only, an event is recorded after each of its passes, and the owner's stream waits for all of them before this
// returns, so the caller's stage goes on the owner's stream.  A handle may appear more than once, the owner included.  skip_row0:
// models[0] is not evaluated and row 0 of mu and var is filled with 0xff bytes (NaN).  The caller has ensure_con's block on the
// owner and ends the call with multi_download.
static int multi_posterior(bohip_gp* owner, bohip_gp* const* models, int64_t n, bool skip_row0, const double* Xs, int64_t R, bool jac,
                           const ConBufs& b) {
    const int d = owner->d;
    const int64_t c0 = skip_row0 ? 1 : 0;
    t_reset(owner);
    CHK(ensure_xs(owner, R));
    HIPCHK(hipMemcpyAsync(owner->dXs, Xs, (size_t)R * d * 8, hipMemcpyHostToDevice, owner->stream));
    if (std::any_of(models + c0, models + n, [&](bohip_gp* m) { return m != owner; })) {
        HIPCHK(event_of(owner));
        HIPCHK(hipEventRecord(owner->ev_con, owner->stream));
    }
    if (skip_row0) {
        HIPCHK(hipMemsetAsync(b.mu, 0xff, (size_t)R * 8, owner->stream));
        HIPCHK(hipMemsetAsync(b.var, 0xff, (size_t)R * 8, owner->stream));
    }
    for (int64_t c = c0; c < n; ++c) {
        bohip_gp* m = models[c];
        if (m != owner && std::find(models + c0, models + c, m) == models + c) {
            t_reset(m);
            HIPCHK(hipStreamWaitEvent(m->stream, owner->ev_con, 0));
        }
        const size_t o = (size_t)c * R;
        CHK(posterior_grad_core(m, owner->dXs, R, b.mu + o, b.var + o, jac ? b.jmu + o * d : nullptr, jac ? b.jvar + o * d : nullptr));
        if (m != owner) { HIPCHK(event_of(m)); HIPCHK(hipEventRecord(m->ev_con, m->stream)); }
    }
    for (int64_t c = c0; c < n; ++c)
        if (models[c] != owner) HIPCHK(hipStreamWaitEvent(owner->stream, models[c]->ev_con, 0));
    return 0;
}
// ... and the end of such a call, after the stage: the value, the gradient, every row of the moments and the record where asked
// for, the one synchronisation, and the stage times of every handle that took part (a handle other than the owner once per
// appearance, as ever: after the first collection there is nothing left, so one that appears twice reads empty)
static int multi_download(bohip_gp* owner, bohip_gp* const* models, int64_t n, const ConBufs& b, int64_t R, double* score, double* grad,
                          double* mu, double* var, bohip_best* best) {
    const size_t m_bytes = (size_t)n * R * 8;
    if (score) HIPCHK(hipMemcpyAsync(score, b.value, (size_t)R * 8, hipMemcpyDeviceToHost, owner->stream));
    if (grad) HIPCHK(hipMemcpyAsync(grad, b.grad, (size_t)R * owner->d * 8, hipMemcpyDeviceToHost, owner->stream));
    if (mu) HIPCHK(hipMemcpyAsync(mu, b.mu, m_bytes, hipMemcpyDeviceToHost, owner->stream));
    if (var) HIPCHK(hipMemcpyAsync(var, b.var, m_bytes, hipMemcpyDeviceToHost, owner->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, b.best, sizeof(Best), hipMemcpyDeviceToHost, owner->stream));
    HIPCHK(hipStreamSynchronize(owner->stream));
    t_collect(owner);
    for (int64_t c = 0; c < n; ++c)
        if (models[c] != owner) t_collect(models[c]);
    return 0;
}

int bohip_gp_predict_grad(bohip_gp* g, const double* Xs, int64_t R, double* mu, double* var, double* dmu, double* dvar) {
    if (!g || R < 0 || (R > 0 && (!Xs || !mu || !var || !dmu || !dvar))) return fail(BOHIP_E_ARG, "predict_grad: bad arguments");
    if (R == 0) return 0;
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_xs(g, R));
    ConBufs b{};
    CHK(ensure_con(g, 0, R, true, &b));
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    CHK(posterior_grad_core(g, g->dXs, R, b.mu, b.var, b.jmu, b.jvar));
    HIPCHK(hipMemcpyAsync(mu, b.mu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(var, b.var, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(dmu, b.jmu, (size_t)R * g->d * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(dvar, b.jvar, (size_t)R * g->d * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// A stage on the caller's moments (bohip_con_values, bohip_mo_ehvi_values; the callers have validated): `rows` x R of mu and var up
// into ensure_con's block, stage(b) on g's stream, then value, logfeas where asked for, the partials [rows][R] with dmu, the record
// with best, and the one synchronisation.  R == 0 touches no device.
extern "C++" {
template <class Stage>
static int moments_to_values(bohip_gp* g, int64_t rows, const double* mu, const double* var, int64_t R, Stage&& stage, double* value,
                             double* logfeas, double* dmu, double* dvar, bohip_best* best) {
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    ConBufs b{};
    CHK(ensure_con(g, rows - 1, R, false, &b));
    const size_t m = (size_t)rows * R * 8;
    HIPCHK(hipMemcpyAsync(b.mu, mu, m, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(b.var, var, m, hipMemcpyHostToDevice, g->stream));
    CHK(stage(b));
    HIPCHK(hipMemcpyAsync(value, b.value, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (logfeas) HIPCHK(hipMemcpyAsync(logfeas, b.logfeas, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (dmu) {
        HIPCHK(hipMemcpyAsync(dmu, b.pmu, m, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipMemcpyAsync(dvar, b.pvar, m, hipMemcpyDeviceToHost, g->stream));
    }
    if (best) HIPCHK(hipMemcpyAsync(best, b.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}
}   // extern "C++"

int bohip_con_values(bohip_gp* g, int acq_id, const double* acq_params, int64_t C, const double* thresholds, const int* senses,
                     const double* mu, const double* var, int64_t R, double* value, double* logfeas, double* dmu, double* dvar,
                     bohip_best* best) {
    if (!g) return fail(BOHIP_E_ARG, "con_values: null handle");
    ConParams cp;
    CHK(con_make_params("con_values", acq_id, acq_params, C, thresholds, senses, &cp));
    if (R < 0 || (R > 0 && (!mu || !var || !value))) return fail(BOHIP_E_ARG, "con_values: bad arguments");
    if ((dmu == nullptr) != (dvar == nullptr)) return fail(BOHIP_E_ARG, "con_values: dmu and dvar are given together or not at all");
    auto stage = [&](const ConBufs& b) { return con_combine_stage(g, cp, b, R, dmu != nullptr, false, best != nullptr); };
    return moments_to_values(g, C + 1, mu, var, R, stage, value, logfeas, dmu, dvar, best);
}

int bohip_gp_score_con(bohip_gp* obj, int acq_id, const double* acq_params, int64_t C, bohip_gp* const* cons, const double* thresholds,
                       const int* senses, const double* Xs, int64_t R, double* score, double* logfeas, double* grad, double* mu,
                       double* var, bohip_best* best) {
    if (!obj) return fail(BOHIP_E_ARG, "score_con: null objective handle");
    ConParams cp;
    CHK(con_make_params("score_con", acq_id, acq_params, C, thresholds, senses, &cp));
    if (C > 0 && !cons) return fail(BOHIP_E_ARG, "score_con: cons is null");
    for (int64_t c = 0; c < C; ++c) {
        if (!cons[c]) return fail(BOHIP_E_ARG, "score_con: constraint handle " + std::to_string(c) + " is null");
        if (cons[c]->d != obj->d) return fail(BOHIP_E_ARG, "score_con: constraint " + std::to_string(c) + " has another dimension");
        if (cons[c]->device != obj->device) return fail(BOHIP_E_ARG, "score_con: constraint " + std::to_string(c) + " lives on another device");
    }
    if (R < 0 || (R > 0 && !Xs)) return fail(BOHIP_E_ARG, "score_con: bad arguments");
    const bool feas = acq_id == BOHIP_CON_FEASIBILITY;
    if (!feas && obj->n == 0) return fail(BOHIP_E_STATE, "score_con: the objective has no observations");
    for (int64_t c = 0; c < C; ++c)
        if (cons[c]->n == 0) return fail(BOHIP_E_STATE, "score_con: constraint " + std::to_string(c) + " has no observations");
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    HIPCHK(hipSetDevice(obj->device));
    const bool jac = grad != nullptr;
    ConBufs b{};
    CHK(ensure_con(obj, C, R, jac, &b));
    bohip_gp* models[BOHIP_CON_CMAX + 1] = {obj};   // row 0 the objective (not computed under "Feasibility"), row c + 1 constraint c
    std::copy_n(cons, C, models + 1);
    CHK(multi_posterior(obj, models, C + 1, feas, Xs, R, jac, b));
    CHK(con_combine_stage(obj, cp, b, R, false, jac, best != nullptr));
    if (logfeas) HIPCHK(hipMemcpyAsync(logfeas, b.logfeas, (size_t)R * 8, hipMemcpyDeviceToHost, obj->stream));
    return multi_download(obj, models, C + 1, b, R, score, grad, mu, var, best);
}

// ---- two-objective optimisation (kernels_mo.hip, include/bohip_mo.h) ----------------------------------------------
static_assert(MO_FRONT_MAX == BOHIP_MO_FRONT_MAX && MO_G == BOHIP_MO_GROUP, "the kernel's plan and the header agree");

// host only: the observations that strictly dominate ref and are not weakly dominated by another, ascending in f1; no device call
int bohip_mo_front(const double* Y, int64_t n, const double* ref, double* front, int64_t cap, int64_t* n_front, double* hv) {
    if (n < 0 || cap < 0 || !ref || (n > 0 && !Y) || (cap > 0 && !front)) return fail(BOHIP_E_ARG, "mo_front: bad arguments");
    if (!std::isfinite(ref[0]) || !std::isfinite(ref[1])) return fail(BOHIP_E_ARG, "mo_front: the reference point is not finite");
    std::vector<std::pair<double, double>> pts;
    for (int64_t i = 0; i < n; ++i) {
        const double a = Y[i], b = Y[n + i];
        if (!std::isfinite(a) || !std::isfinite(b)) return fail(BOHIP_E_ARG, "mo_front: observation " + std::to_string(i) + " is not finite");
        if (a > ref[0] && b > ref[1]) pts.emplace_back(a, b);
    }
    // descending in f1, ties descending in f2: a point stays if its f2 exceeds every f2 seen so far (of equal points the first)
    std::sort(pts.begin(), pts.end(), [](const std::pair<double, double>& p, const std::pair<double, double>& q) {
        return p.first > q.first || (p.first == q.first && p.second > q.second);
    });
    std::vector<std::pair<double, double>> keep;
    double top = -INFINITY;
    for (const auto& p : pts)
        if (p.second > top) { keep.push_back(p); top = p.second; }
    std::reverse(keep.begin(), keep.end());
    const int64_t m = (int64_t)keep.size();
    if (n_front) *n_front = m;
    if (hv) {
        double a = 0.0, prev = ref[0];
        for (const auto& p : keep) { a += (p.first - prev) * (p.second - ref[1]); prev = p.first; }
        *hv = a;
    }
    if (cap == 0) return 0;
    if (cap < m) return fail(BOHIP_E_ARG, "mo_front: the front has " + std::to_string(m) + " points, cap is " + std::to_string(cap));
    for (int64_t i = 0; i < m; ++i) { front[i] = keep[i].first; front[cap + i] = keep[i].second; }
    return 0;
}

// validates the front and lays out what k_ehvi reads: c[0 .. n + 1] then b[0 .. n]
static int mo_make_front(const char* who, const double* front, int64_t n, const double* ref, std::vector<double>* out) {
    const std::string pre = std::string(who) + ": ";
    if (n < 0 || !ref || (n > 0 && !front)) return fail(BOHIP_E_ARG, pre + "bad front arguments");
    if (n > BOHIP_MO_FRONT_MAX)
        return fail(BOHIP_E_UNSUPPORTED, pre + "a front of " + std::to_string(n) + " points; at most " + std::to_string(BOHIP_MO_FRONT_MAX));
    if (!std::isfinite(ref[0]) || !std::isfinite(ref[1])) return fail(BOHIP_E_ARG, pre + "the reference point is not finite");
    for (int64_t i = 0; i < n; ++i) {
        const double a = front[i], b = front[n + i];
        if (!std::isfinite(a) || !std::isfinite(b)) return fail(BOHIP_E_ARG, pre + "front point " + std::to_string(i) + " is not finite");
        if (!(a > ref[0]) || !(b > ref[1])) return fail(BOHIP_E_ARG, pre + "front point " + std::to_string(i) + " is not strictly above ref");
        if (i > 0 && (!(a > front[i - 1]) || !(b < front[n + i - 1])))
            return fail(BOHIP_E_ARG, pre + "the front must ascend strictly in f1 and descend strictly in f2 (point " + std::to_string(i) + ")");
    }
    out->resize((size_t)(2 * n + 3));
    double* c = out->data();
    double* b = c + n + 2;
    c[0] = ref[0];
    for (int64_t i = 0; i < n; ++i) { c[i + 1] = front[i]; b[i] = front[n + i]; }
    c[n + 1] = INFINITY;
    b[n] = ref[1];
    return 0;
}
static int mo_upload_front(bohip_gp* g, const std::vector<double>& fr) {
    HIPCHK(g->mo_front.reserve((size_t)(2 * BOHIP_MO_FRONT_MAX + 3), g->stream));
    HIPCHK(hipMemcpyAsync(g->mo_front, fr.data(), fr.size() * 8, hipMemcpyHostToDevice, g->stream));
    return 0;
}
// the EHVI and the record on g's stream (no synchronisation, no copies); b is ensure_con's block with C = 1
static int mo_ehvi_stage(bohip_gp* g, int64_t n_front, const ConBufs& b, int64_t R, bool partials, bool jac, bool want_best) {
    const int nb = (int)std::min<int64_t>(MO_GRID_MAX, (R + MO_CAND - 1) / MO_CAND);
    const StageOuts o = stage_outs(g, b, R, partials, jac, want_best);
    t_begin(g, "mo_ehvi");
    hipLaunchKernelGGL(o.grad_form ? k_ehvi<true> : k_ehvi<false>, dim3(nb), dim3(256), 0, g->stream, (const double*)g->mo_front, (int)n_front,
                       (const double*)b.mu, (const double*)b.var, R, R, b.value, o.pmu, o.pvar, o.jmu, o.jvar, o.jplane, g->d, o.grad, o.blocks);
    return stage_end(g, b, nb, want_best);
}

int bohip_mo_ehvi_values(bohip_gp* g, const double* front, int64_t n_front, const double* ref, const double* mu, const double* var,
                         int64_t R, double* value, double* dmu, double* dvar, bohip_best* best) {
    if (!g) return fail(BOHIP_E_ARG, "mo_ehvi_values: null handle");
    std::vector<double> fr;
    CHK(mo_make_front("mo_ehvi_values", front, n_front, ref, &fr));
    if (R < 0 || (R > 0 && (!mu || !var || !value))) return fail(BOHIP_E_ARG, "mo_ehvi_values: bad arguments");
    if ((dmu == nullptr) != (dvar == nullptr)) return fail(BOHIP_E_ARG, "mo_ehvi_values: dmu and dvar are given together or not at all");
    auto stage = [&](const ConBufs& b) -> int {
        CHK(mo_upload_front(g, fr));
        return mo_ehvi_stage(g, n_front, b, R, dmu != nullptr, false, best != nullptr);
    };
    return moments_to_values(g, 2, mu, var, R, stage, value, nullptr, dmu, dvar, best);
}

int bohip_gp_score_mo(bohip_gp* obj0, bohip_gp* obj1, const double* front, int64_t n_front, const double* ref, const double* Xs,
                      int64_t R, double* score, double* grad, double* mu, double* var, bohip_best* best) {
    if (!obj0 || !obj1) return fail(BOHIP_E_ARG, "score_mo: null handle");
    if (obj1->d != obj0->d) return fail(BOHIP_E_ARG, "score_mo: the objectives differ in dimension");
    if (obj1->device != obj0->device) return fail(BOHIP_E_ARG, "score_mo: the objectives live on different devices");
    std::vector<double> fr;
    CHK(mo_make_front("score_mo", front, n_front, ref, &fr));
    if (R < 0 || (R > 0 && !Xs)) return fail(BOHIP_E_ARG, "score_mo: bad arguments");
    if (obj0->n == 0 || obj1->n == 0) return fail(BOHIP_E_STATE, "score_mo: an objective has no observations");
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    HIPCHK(hipSetDevice(obj0->device));
    const bool jac = grad != nullptr;
    ConBufs b{};
    CHK(ensure_con(obj0, 1, R, jac, &b));
    CHK(mo_upload_front(obj0, fr));   // (on obj0's stream, ahead of its posterior)
    bohip_gp* const models[2] = {obj0, obj1};
    CHK(multi_posterior(obj0, models, 2, false, Xs, R, jac, b));
    CHK(mo_ehvi_stage(obj0, n_front, b, R, false, jac, best != nullptr));
    return multi_download(obj0, models, 2, b, R, score, grad, mu, var, best);
}

// ---- two to four objectives (kernels_mom.hip, include/bohip_mom.h) -------------------------------------------------
static_assert(MOM_OBJ_MAX == BOHIP_MOM_OBJ_MAX && MOM_FRONT_MAX == BOHIP_MOM_FRONT_MAX && MOM_BOX_MAX == BOHIP_MOM_BOX_MAX &&
                  MOM_LANES == BOHIP_MOM_LANES && MOM_OBJ_MAX <= BOHIP_CON_CMAX + 1,
              "the kernel's plan and the header agree; ensure_con's block holds M rows");
using MomPt = std::array<int, BOHIP_MOM_OBJ_MAX>;   // a front point as level indices, 1 .. n_levels[m] - 2

// the non-dominated subset of pts in the first `dim` coordinates (weak dominance; of equal projections one): in descending
// lexicographic order whatever dominates a point stands before it, and dominance is transitive, so the kept ones decide
static std::vector<MomPt> mom_filter(std::vector<MomPt> pts, int dim) {
    auto key_gt = [dim](const MomPt& p, const MomPt& q) { return std::lexicographical_compare(q.begin(), q.begin() + dim, p.begin(), p.begin() + dim); };
    auto key_eq = [dim](const MomPt& p, const MomPt& q) { return std::equal(p.begin(), p.begin() + dim, q.begin()); };
    std::sort(pts.begin(), pts.end(), key_gt);
    pts.erase(std::unique(pts.begin(), pts.end(), key_eq), pts.end());
    std::vector<MomPt> keep;
    for (const MomPt& p : pts) {
        const bool dominated = std::any_of(keep.begin(), keep.end(), [&](const MomPt& k) {
            for (int c = 0; c < dim; ++c)
                if (k[c] < p[c]) return false;
            return true;
        });
        if (!dominated) keep.push_back(p);
    }
    return keep;
}
// the slabs of P (non-dominated in `dim` coordinates) along coordinate dim - 1: z[0] = 0 (ref), the distinct levels ascending, then
// nl - 1 (+Inf); slab j is [z[j], z[j + 1])
static std::vector<int> mom_slabs(const std::vector<MomPt>& P, int dim, int nl) {
    std::vector<int> z{0};
    for (const MomPt& p : P) z.push_back(p[dim - 1]);
    std::sort(z.begin(), z.end());
    z.erase(std::unique(z.begin(), z.end()), z.end());
    z.push_back(nl - 1);
    return z;
}
static std::vector<MomPt> mom_above(const std::vector<MomPt>& P, int dim, int zj) {
    std::vector<MomPt> Q;
    for (const MomPt& p : P)
        if (p[dim - 1] > zj) Q.push_back(p);
    return mom_filter(std::move(Q), dim - 1);
}
struct MomFront {
    int M = 0;
    std::vector<double> levels[BOHIP_MOM_OBJ_MAX];   // L_m
    std::vector<MomPt> pts;                          // the front in level indices
    int64_t n_boxes = 0;
    std::vector<int32_t> lo[BOHIP_MOM_OBJ_MAX], hi[BOHIP_MOM_OBJ_MAX];   // per box, filled up to `keep` boxes
};
// decomp(P, r) of bohip_mom.h, section 1: counts every box, stores the first `keep`
static void mom_decomp(MomFront* f, const std::vector<MomPt>& P, int dim, MomPt* lo, MomPt* hi, int64_t keep) {
    if (dim == 1) {
        int l = 0;
        for (const MomPt& p : P) l = std::max(l, p[0]);
        (*lo)[0] = l;
        (*hi)[0] = (int)f->levels[0].size() - 1;
        if (f->n_boxes < keep)
            for (int m = 0; m < f->M; ++m) { f->lo[m].push_back((*lo)[m]); f->hi[m].push_back((*hi)[m]); }
        ++f->n_boxes;
        return;
    }
    const std::vector<int> z = mom_slabs(P, dim, (int)f->levels[dim - 1].size());
    for (size_t j = 0; j + 1 < z.size(); ++j) {
        (*lo)[dim - 1] = z[j];
        (*hi)[dim - 1] = z[j + 1];
        mom_decomp(f, mom_above(P, dim, z[j]), dim - 1, lo, hi, keep);
    }
}
// HV_dim(P) of bohip_mom.h, section 1
static double mom_hv(const MomFront& f, const std::vector<MomPt>& P, int dim) {
    if (dim == 1) {
        int l = 0;
        for (const MomPt& p : P) l = std::max(l, p[0]);
        return f.levels[0][l] - f.levels[0][0];
    }
    const std::vector<int> z = mom_slabs(P, dim, (int)f.levels[dim - 1].size());
    const std::vector<double>& L = f.levels[dim - 1];
    double a = 0.0;
    for (size_t j = 0; j + 2 < z.size(); ++j) a += (L[z[j + 1]] - L[z[j]]) * mom_hv(f, mom_above(P, dim, z[j]), dim - 1);
    return a;
}
static int mom_check_common(const std::string& pre, int64_t M, const double* ref) {
    if (M < 2 || M > BOHIP_MOM_OBJ_MAX)
        return fail(BOHIP_E_ARG, pre + "M must be in [2, " + std::to_string(BOHIP_MOM_OBJ_MAX) + "], got " + std::to_string(M));
    if (!ref) return fail(BOHIP_E_ARG, pre + "ref is null");
    for (int64_t m = 0; m < M; ++m)
        if (!std::isfinite(ref[m])) return fail(BOHIP_E_ARG, pre + "the reference point is not finite");
    return 0;
}
// the levels and the index form of points known to be finite and strictly above ref (M x n of stride ld)
static void mom_index(const double* pts, int64_t ld, int64_t n, int64_t M, const double* ref, MomFront* f) {
    f->M = (int)M;
    f->pts.assign((size_t)n, MomPt{});
    for (int64_t m = 0; m < M; ++m) {
        std::vector<double>& L = f->levels[m];
        L.assign(pts + m * ld, pts + m * ld + n);
        std::sort(L.begin(), L.end());
        L.erase(std::unique(L.begin(), L.end()), L.end());
        L.insert(L.begin(), ref[m]);
        for (int64_t i = 0; i < n; ++i) f->pts[(size_t)i][m] = (int)(std::lower_bound(L.begin() + 1, L.end(), pts[m * ld + i]) - L.begin());
        L.push_back(INFINITY);
    }
}

// host only: the observations strictly above ref that no other weakly dominates, of equal ones one, lexicographic ascending
int bohip_mom_front(const double* Y, int64_t M, int64_t n, const double* ref, double* front, int64_t cap, int64_t* n_front, double* hv) {
    CHK(mom_check_common("mom_front: ", M, ref));
    if (n < 0 || cap < 0 || (n > 0 && !Y) || (cap > 0 && !front)) return fail(BOHIP_E_ARG, "mom_front: bad arguments");
    std::vector<double> above;   // M x k, stride n
    above.resize((size_t)(M * std::max<int64_t>(n, 1)));
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i) {
        bool in = true;
        for (int64_t m = 0; m < M; ++m) {
            if (!std::isfinite(Y[m * n + i])) return fail(BOHIP_E_ARG, "mom_front: observation " + std::to_string(i) + " is not finite");
            in = in && Y[m * n + i] > ref[m];
        }
        if (!in) continue;
        for (int64_t m = 0; m < M; ++m) above[(size_t)(m * n + k)] = Y[m * n + i];
        ++k;
    }
    MomFront f;
    mom_index(above.data(), n, k, M, ref, &f);
    std::vector<MomPt> keep = mom_filter(f.pts, (int)M);   // (index order is value order)
    std::reverse(keep.begin(), keep.end());
    const int64_t nf = (int64_t)keep.size();
    if (n_front) *n_front = nf;
    if (hv) *hv = mom_hv(f, keep, (int)M);
    if (cap == 0) return 0;
    if (cap < nf) return fail(BOHIP_E_ARG, "mom_front: the front has " + std::to_string(nf) + " points, cap is " + std::to_string(cap));
    for (int64_t i = 0; i < nf; ++i)
        for (int64_t m = 0; m < M; ++m) front[m * cap + i] = f.levels[m][(size_t)keep[(size_t)i][m]];
    return 0;
}

// validates a front (any order) and builds its levels and, with keep > 0, its boxes
static int mom_make_front(const char* who, int64_t M, const double* front, int64_t n, const double* ref, int64_t keep, MomFront* f) {
    const std::string pre = std::string(who) + ": ";
    CHK(mom_check_common(pre, M, ref));
    if (n < 0 || (n > 0 && !front)) return fail(BOHIP_E_ARG, pre + "bad front arguments");
    if (n > BOHIP_MOM_FRONT_MAX)
        return fail(BOHIP_E_UNSUPPORTED, pre + "a front of " + std::to_string(n) + " points; at most " + std::to_string(BOHIP_MOM_FRONT_MAX));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t m = 0; m < M; ++m) {
            if (!std::isfinite(front[m * n + i])) return fail(BOHIP_E_ARG, pre + "front point " + std::to_string(i) + " is not finite");
            if (!(front[m * n + i] > ref[m])) return fail(BOHIP_E_ARG, pre + "front point " + std::to_string(i) + " is not strictly above ref");
        }
    mom_index(front, n, n, M, ref, f);
    if ((int64_t)mom_filter(f->pts, (int)M).size() != n)
        return fail(BOHIP_E_ARG, pre + "the front holds a weakly dominated or a duplicated point");
    MomPt lo{}, hi{};
    mom_decomp(f, f->pts, (int)M, &lo, &hi, keep);
    return 0;
}

int bohip_mom_boxes(const double* front, int64_t M, int64_t n_front, const double* ref, double* levels, int64_t* n_levels, int32_t* boxes,
                    int64_t cap, int64_t* n_boxes) {
    if (cap < 0 || (cap > 0 && !boxes)) return fail(BOHIP_E_ARG, "mom_boxes: bad arguments");
    MomFront f;
    CHK(mom_make_front("mom_boxes", M, front, n_front, ref, cap, &f));
    if (n_boxes) *n_boxes = f.n_boxes;
    for (int64_t m = 0; m < M; ++m) {
        if (n_levels) n_levels[m] = (int64_t)f.levels[m].size();
        if (levels) std::copy(f.levels[m].begin(), f.levels[m].end(), levels + m * (n_front + 2));
    }
    if (f.n_boxes > BOHIP_MOM_BOX_MAX)
        return fail(BOHIP_E_UNSUPPORTED, "mom_boxes: " + std::to_string(f.n_boxes) + " boxes; at most " + std::to_string(BOHIP_MOM_BOX_MAX));
    if (cap == 0) return 0;
    if (cap < f.n_boxes) return fail(BOHIP_E_ARG, "mom_boxes: " + std::to_string(f.n_boxes) + " boxes, cap is " + std::to_string(cap));
    for (int64_t m = 0; m < M; ++m) {
        std::copy(f.lo[m].begin(), f.lo[m].end(), boxes + m * cap);
        std::copy(f.hi[m].begin(), f.hi[m].end(), boxes + (M + m) * cap);
    }
    return 0;
}

// what k_ehvi_boxes reads, built on the host: the level rows and the packed boxes
struct MomPlan {
    int M = 0, nbox = 0;
    MomLevels nl{};
    std::vector<double> key;         // what the plan was made from: M, n, ref, then the front
    std::vector<double> levels;      // [M][MOM_LEVELS]
    std::vector<unsigned> boxes;     // [M][nbox]: lo | hi << 16
};
// the plan of (front, ref): the one resident on g (bit-equal arguments in the same order; *resident says so) or a new one
static int mom_make_plan(bohip_gp* g, const char* who, int64_t M, const double* front, int64_t n, const double* ref,
                         std::shared_ptr<MomPlan>* out, bool* resident) {
    const std::string pre = std::string(who) + ": ";
    CHK(mom_check_common(pre, M, ref));
    if (n < 0 || (n > 0 && !front)) return fail(BOHIP_E_ARG, pre + "bad front arguments");
    if (n > BOHIP_MOM_FRONT_MAX)
        return fail(BOHIP_E_UNSUPPORTED, pre + "a front of " + std::to_string(n) + " points; at most " + std::to_string(BOHIP_MOM_FRONT_MAX));
    std::vector<double> key{(double)M, (double)n};
    key.insert(key.end(), ref, ref + M);
    key.insert(key.end(), front, front + M * n);
    *resident = g->mom_plan && g->mom_plan->key.size() == key.size() && std::memcmp(g->mom_plan->key.data(), key.data(), key.size() * 8) == 0;
    if (*resident) {
        *out = g->mom_plan;
        return 0;
    }
    MomFront f;
    CHK(mom_make_front(who, M, front, n, ref, BOHIP_MOM_BOX_MAX, &f));
    if (f.n_boxes > BOHIP_MOM_BOX_MAX)
        return fail(BOHIP_E_UNSUPPORTED, pre + std::to_string(f.n_boxes) + " boxes; at most " + std::to_string(BOHIP_MOM_BOX_MAX));
    auto p = std::make_shared<MomPlan>();
    p->M = (int)M;
    p->nbox = (int)f.n_boxes;
    p->key = std::move(key);
    p->levels.assign((size_t)(M * MOM_LEVELS), INFINITY);
    p->boxes.resize((size_t)(M * f.n_boxes));
    for (int64_t m = 0; m < M; ++m) {
        p->nl.n[m] = (int)f.levels[m].size();
        std::copy(f.levels[m].begin(), f.levels[m].end(), p->levels.begin() + m * MOM_LEVELS);
        for (int64_t b = 0; b < f.n_boxes; ++b)
            p->boxes[(size_t)(m * f.n_boxes + b)] = (unsigned)f.lo[m][(size_t)b] | ((unsigned)f.hi[m][(size_t)b] << 16);
    }
    *out = std::move(p);
    return 0;
}
// on g's stream; the handle keeps the plan (and with it the host copies the transfers read) once both are queued
static int mom_upload_plan(bohip_gp* g, const std::shared_ptr<MomPlan>& p, bool resident) {
    if (resident) return 0;
    g->mom_plan.reset();
    HIPCHK(g->mom_levels.reserve((size_t)(BOHIP_MOM_OBJ_MAX * MOM_LEVELS), g->stream));
    HIPCHK(g->mom_boxes.reserve(p->boxes.size(), g->stream, Grow::Half));
    HIPCHK(hipMemcpyAsync(g->mom_levels, p->levels.data(), p->levels.size() * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(g->mom_boxes, p->boxes.data(), p->boxes.size() * 4, hipMemcpyHostToDevice, g->stream));
    g->mom_plan = p;
    return 0;
}
// the EHVI and the record on g's stream (no synchronisation, no copies); b is ensure_con's block with C = M - 1
static int mom_ehvi_stage(bohip_gp* g, const MomPlan& p, const ConBufs& b, int64_t R, bool partials, bool jac, bool want_best) {
    const StageOuts o = stage_outs(g, b, R, partials, jac, want_best);
    const int W = mom_cand(o.grad_form);
    const int nb = (int)std::min<int64_t>(MO_GRID_MAX, (R + W - 1) / W);
    t_begin(g, "mom_ehvi");
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(64 * W), 0, g->stream, (const double*)g->mom_levels, p.nl, (const unsigned*)g->mom_boxes, p.nbox,
                           (const double*)b.mu, (const double*)b.var, R, R, b.value, o.pmu, o.pvar, o.jmu, o.jvar, o.jplane, g->d, o.grad, o.blocks);
    };
    if (o.grad_form) {
        if (p.M == 2) launch(k_ehvi_boxes<2, true>);
        else if (p.M == 3) launch(k_ehvi_boxes<3, true>);
        else launch(k_ehvi_boxes<4, true>);
    } else {
        if (p.M == 2) launch(k_ehvi_boxes<2, false>);
        else if (p.M == 3) launch(k_ehvi_boxes<3, false>);
        else launch(k_ehvi_boxes<4, false>);
    }
    return stage_end(g, b, nb, want_best);
}

int bohip_mom_ehvi_values(bohip_gp* g, int64_t M, const double* front, int64_t n_front, const double* ref, const double* mu,
                          const double* var, int64_t R, double* value, double* dmu, double* dvar, bohip_best* best) {
    if (!g) return fail(BOHIP_E_ARG, "mom_ehvi_values: null handle");
    if (R < 0 || (R > 0 && (!mu || !var || !value))) return fail(BOHIP_E_ARG, "mom_ehvi_values: bad arguments");
    if ((dmu == nullptr) != (dvar == nullptr)) return fail(BOHIP_E_ARG, "mom_ehvi_values: dmu and dvar are given together or not at all");
    std::shared_ptr<MomPlan> p;
    bool resident = false;
    CHK(mom_make_plan(g, "mom_ehvi_values", M, front, n_front, ref, &p, &resident));
    auto stage = [&](const ConBufs& b) -> int {
        CHK(mom_upload_plan(g, p, resident));
        return mom_ehvi_stage(g, *p, b, R, dmu != nullptr, false, best != nullptr);
    };
    return moments_to_values(g, M, mu, var, R, stage, value, nullptr, dmu, dvar, best);
}

int bohip_gp_score_mom(bohip_gp* const* objs, int64_t M, const double* front, int64_t n_front, const double* ref, const double* Xs,
                       int64_t R, double* score, double* grad, double* mu, double* var, bohip_best* best) {
    if (M < 2 || M > BOHIP_MOM_OBJ_MAX)
        return fail(BOHIP_E_ARG, "score_mom: M must be in [2, " + std::to_string(BOHIP_MOM_OBJ_MAX) + "], got " + std::to_string(M));
    if (!objs) return fail(BOHIP_E_ARG, "score_mom: objs is null");
    for (int64_t m = 0; m < M; ++m) {
        if (!objs[m]) return fail(BOHIP_E_ARG, "score_mom: handle " + std::to_string(m) + " is null");
        if (objs[m]->d != objs[0]->d) return fail(BOHIP_E_ARG, "score_mom: objective " + std::to_string(m) + " has another dimension");
        if (objs[m]->device != objs[0]->device) return fail(BOHIP_E_ARG, "score_mom: objective " + std::to_string(m) + " lives on another device");
    }
    if (R < 0 || (R > 0 && !Xs)) return fail(BOHIP_E_ARG, "score_mom: bad arguments");
    std::shared_ptr<MomPlan> p;
    bool resident = false;
    CHK(mom_make_plan(objs[0], "score_mom", M, front, n_front, ref, &p, &resident));
    for (int64_t m = 0; m < M; ++m)
        if (objs[m]->n == 0) return fail(BOHIP_E_STATE, "score_mom: objective " + std::to_string(m) + " has no observations");
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    bohip_gp* const owner = objs[0];
    HIPCHK(hipSetDevice(owner->device));
    const bool jac = grad != nullptr;
    ConBufs b{};
    CHK(ensure_con(owner, M - 1, R, jac, &b));
    CHK(mom_upload_plan(owner, p, resident));   // (on the owner's stream, ahead of its posterior)
    CHK(multi_posterior(owner, objs, M, false, Xs, R, jac, b));
    CHK(mom_ehvi_stage(owner, *p, b, R, false, jac, best != nullptr));
    return multi_download(owner, objs, M, b, R, score, grad, mu, var, best);
}

// ---- posterior sample paths (kernels_path.hip): pathwise conditioning with a random-feature prior ----------------
// The object owns copies of everything an evaluation reads (X, Omega, Cf, the hyper-parameters), so the model may change or be
// refitted afterwards; it borrows the handle's device and stream.
struct bohip_paths {
    bohip_gp* g = nullptr;
    int64_t S = 0, M = 0, N = 0, Npad = 0, ldc = 0;
    int d = 0, F = 0, mfma_min = 0;
    double amp = 0.0, beta = 0.0;
    KernelHyper hp;
    DBuf<double> dX, dOm, dCf;
    // evaluation scratch: one chunk of candidates, its S x chunk values, its tile records, the S running records, the gradient staging
    DBuf<double> dXs, dV, df, dg;
    DBuf<int64_t> dpath_of;
    DBuf<Best> dpart, dbest;
};
static constexpr int64_t PATHS_CHUNK = 32768;       // candidates per launch of an evaluation (a multiple of PM_ROWS and PR_CAND)
static constexpr int64_t PATHS_GRAD_CHUNK = 4096;   // points per launch of bohip_paths_eval_grad
static_assert(BOHIP_PATHS_S_MAX <= 65535 && PATHS_CHUNK % PM_ROWS == 0 && PATHS_CHUNK % PR_CAND == 0, "grid.y holds the path tiles");

static void paths_free(bohip_paths* p) { delete p; }   // (the members free themselves)
static PathArgs paths_args(const bohip_paths* p) {
    return PathArgs{p->dX, p->dOm, p->dCf, p->N, p->Npad, p->ldc, p->S, p->F, p->amp, p->beta};
}
static bool paths_use_mfma(const bohip_paths* p) { return p->S >= p->mfma_min; }
static int64_t paths_tile(bool mfma) { return mfma ? PM_ROWS : PR_CAND; }

// One launch over Rc candidates already on the device: values (nullable, leading dimension ldv) and, with dbest, the fold of the
// chunk's tile records onto dbest (carry: onto what the earlier chunks left there).
static int paths_eval_launch(bohip_paths* p, const double* dXs, int64_t Rc, int64_t j_off, double* dV, int64_t ldv, Best* dbest,
                             bool carry, bool feat_only, bool mfma) {
    hipStream_t st = p->g->stream;
    const PathArgs a = paths_args(p);
    const bool lo = fam_low(p->hp);
    const int ntiles = (int)((Rc + paths_tile(mfma) - 1) / paths_tile(mfma));
    Best* part = dbest ? p->dpart : nullptr;
    if (mfma) {
        const dim3 grid((unsigned)ntiles, (unsigned)((p->S + PM_PATHS - 1) / PM_PATHS));
        LAUNCH_FAM(lo, k_path_mfma<true>, k_path_mfma<false>, grid, dim3(256), path_mfma_lds_bytes(p->d), st, a, p->hp, dXs, Rc, j_off,
                   dV, ldv, part, ntiles, feat_only ? 1 : 0);
    } else if (p->S == 1) {
        LAUNCH_FAM(lo, (k_path_rows<1, true>), (k_path_rows<1, false>), dim3((unsigned)ntiles, 1), dim3(256), 0, st, a, p->hp, dXs, Rc,
                   j_off, dV, ldv, part, ntiles, feat_only ? 1 : 0);
    } else {
        LAUNCH_FAM(lo, (k_path_rows<4, true>), (k_path_rows<4, false>), dim3((unsigned)ntiles, (unsigned)((p->S + 3) / 4)), dim3(256), 0,
                   st, a, p->hp, dXs, Rc, j_off, dV, ldv, part, ntiles, feat_only ? 1 : 0);
    }
    if (dbest) hipLaunchKernelGGL(k_path_best, dim3((unsigned)p->S), dim3(64), 0, st, p->dpart, ntiles, dbest, carry ? 1 : 0);
    HIPCHK(hipGetLastError());
    return 0;
}

static int paths_draw_fill(bohip_paths* p, uint64_t seed) {
    bohip_gp* g = p->g;
    hipStream_t st = g->stream;
    const int64_t N = p->N, S = p->S, M = p->M;
    const int d = p->d;
    HIPCHK(p->dX.reserve((size_t)N * d, st));
    HIPCHK(p->dOm.reserve((size_t)p->F * d, st));
    HIPCHK(p->dCf.reserve((size_t)S * p->ldc, st));
    HIPCHK(p->dbest.reserve((size_t)S, st));
    // right-hand sides and the two triangular products: [S][ldr] twice (k_trimv_stream reads whole chunks of 256 columns, masked by index)
    const int64_t ldr = round_up(N, 256) + 256;
    DBuf<double> T0, T1;   // (freed when the function leaves, however it leaves)
    HIPCHK(T0.reserve((size_t)S * ldr, st));
    if (T1.reserve((size_t)S * ldr, st) != hipSuccess) return fail(BOHIP_E_HIP, "paths_draw: out of device memory");
    {
        HIPCHK(hipMemcpyAsync(p->dX, g->dX, (size_t)N * d * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(p->dCf, 0, (size_t)S * p->ldc * 8, st));
        HIPCHK(hipMemsetAsync(T0, 0, (size_t)S * ldr * 8, st));
        HIPCHK(hipMemsetAsync(T1, 0, (size_t)S * ldr * 8, st));
        t_begin(g, "path_basis");
        PathLen len;
        for (int k = 0; k < DMAX; ++k) len.inv[k] = k < d ? std::exp(-g->loglen[kern_iso(g->kern) ? 0 : k]) : 0.0;
        hipLaunchKernelGGL(k_path_omega, dim3((unsigned)((p->F + 255) / 256)), dim3(256), 0, st, seed, p->F, d, path_family_dof(p->hp.fam), len,
                           p->dOm);
        hipLaunchKernelGGL(k_path_w, dim3((unsigned)((M + 255) / 256), (unsigned)S), dim3(256), 0, st, seed, M, p->dCf, p->ldc, p->Npad);
        HIPCHK(hipGetLastError());
        t_end(g);
        // r_s = Phi(X) w_s at the observations: the evaluation kernel itself, prior term only.  ALWAYS the MFMA form, so that the
        // coefficients of path s do not depend on how many paths were drawn.
        t_begin(g, "path_prior_at_X");
        for (int64_t j0 = 0; j0 < N; j0 += PATHS_CHUNK) {
            const int64_t Rc = std::min<int64_t>(PATHS_CHUNK, N - j0);
            CHK(paths_eval_launch(p, p->dX + j0 * d, Rc, j0, T0 + j0, ldr, nullptr, false, true, true));
        }
        const double noise = std::exp(2.0 * g->lognoise) + std::numeric_limits<double>::epsilon() + g->jitter_last;
        hipLaunchKernelGGL(k_path_rhs, dim3((unsigned)((N + 255) / 256), (unsigned)S), dim3(256), 0, st, seed, M, N, g->dy, g->beta,
                           std::sqrt(noise), T0, ldr);
        HIPCHK(hipGetLastError());
        t_end(g);
        // u_s = W'(W rhs_s): the streaming triangular products, 16 right-hand sides per pass over W
        t_begin(g, "path_solve");
        const int64_t nblk = (N + 7) / 8;
        const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::max(device_cus(), 1), nblk));
        const dim3 tg(wgs, (unsigned)((S + 15) / 16));
        hipLaunchKernelGGL(k_trimv_stream<TRIMV_D>, tg, dim3(TRIMV_THREADS), trimv_lds_bytes(TRIMV_D), st, g->dW, g->ld, N, T0, ldr, (int)S,
                           T1, ldr, 0, (const unsigned*)nullptr);
        hipLaunchKernelGGL(k_trimv_stream<TRIMV_D>, tg, dim3(TRIMV_THREADS), trimv_lds_bytes(TRIMV_D), st, g->dWT, g->ld, N, T1, ldr, (int)S,
                           T0, ldr, 1, (const unsigned*)nullptr);
        hipLaunchKernelGGL(k_path_pack, dim3((unsigned)((N + 255) / 256), (unsigned)S), dim3(256), 0, st, T0, ldr, N, p->dCf, p->ldc);
        HIPCHK(hipGetLastError());
        t_end(g);
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

int bohip_gp_paths_draw(bohip_gp* g, int64_t S, int64_t M, uint64_t seed, bohip_paths** out) {
    auto done = [](int rc) { return rc; };
    if (!out) return fail(BOHIP_E_ARG, "paths_draw: null output pointer");
    *out = nullptr;
    if (!g) return done(fail(BOHIP_E_ARG, "paths_draw: null handle"));
    CHK(refuse_weighted(g, "bohip_gp_paths_draw"));
    if (S < 1) return done(fail(BOHIP_E_ARG, "paths_draw: S must be at least 1"));
    if (M < 2 || (M & 1) || M % 16 != 0) return done(fail(BOHIP_E_ARG, "paths_draw: M must be a positive multiple of 16"));
    if (S > BOHIP_PATHS_S_MAX) return done(fail(BOHIP_E_UNSUPPORTED, "paths_draw: at most " + std::to_string(BOHIP_PATHS_S_MAX) + " paths per object"));
    if (M > BOHIP_PATHS_M_MAX) return done(fail(BOHIP_E_UNSUPPORTED, "paths_draw: at most " + std::to_string(BOHIP_PATHS_M_MAX) + " features"));
    if (g->n < 1) return done(fail(BOHIP_E_STATE, "paths_draw: the model has no observations"));
    if (hipSetDevice(g->device) != hipSuccess) return done(fail(BOHIP_E_HIP, "paths_draw: hipSetDevice failed"));
    t_reset(g);
    int rc = one_time_kernel_setup();
    if (rc == 0) rc = ensure_fresh(g);
    if (rc != 0) return done(rc);
    bohip_paths* p = new bohip_paths;
    p->g = g;
    p->S = S; p->M = M; p->F = (int)(M / 2); p->N = g->n; p->d = g->d;
    p->Npad = round_up(p->N, KC);
    p->ldc = p->Npad + M;                         // a multiple of 16 doubles = 128 B ...
    if ((p->ldc / 16) % 2 == 0) p->ldc += 16;     // ... made an odd one (alloc_model's reason)
    p->hp = make_hyper(g);
    p->beta = g->beta;
    p->amp = std::sqrt(p->hp.sigma2 / (double)p->F);
    p->mfma_min = g_path_mfma_min;
    if (const char* e = getenv("BOHIP_PATH_MFMA_MIN")) p->mfma_min = std::max(1, atoi(e));
    rc = paths_draw_fill(p, seed);
    t_collect(g);
    if (rc != 0) { paths_free(p); return done(rc); }
    *out = p;
    return 0;
}

void bohip_paths_destroy(bohip_paths* p) {
    if (!p) return;
    hipSetDevice(p->g->device);
    hipStreamSynchronize(p->g->stream);
    paths_free(p);
}

int bohip_paths_dims(const bohip_paths* p, int64_t* S, int64_t* M, int64_t* N, int64_t* d) {
    if (!p) return fail(BOHIP_E_ARG, "paths_dims: null object");
    if (S) *S = p->S;
    if (M) *M = p->M;
    if (N) *N = p->N;
    if (d) *d = p->d;
    return 0;
}

int bohip_paths_coef(const bohip_paths* p, int64_t s, double* omega, double* w, double* u) {
    if (!p) return fail(BOHIP_E_ARG, "paths_coef: null object");
    if (s < 0 || s >= p->S) return fail(BOHIP_E_ARG, "paths_coef: no such path");
    HIPCHK(hipSetDevice(p->g->device));
    hipStream_t st = p->g->stream;
    if (omega) HIPCHK(hipMemcpyAsync(omega, p->dOm, (size_t)p->F * p->d * 8, hipMemcpyDeviceToHost, st));
    if (w) HIPCHK(hipMemcpyAsync(w, p->dCf + s * p->ldc + p->Npad, (size_t)p->M * 8, hipMemcpyDeviceToHost, st));
    if (u) HIPCHK(hipMemcpyAsync(u, p->dCf + s * p->ldc, (size_t)p->N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int bohip_paths_eval(bohip_paths* p, const double* Xs, int64_t R, double* values, bohip_best* best) {
    if (!p || !Xs) return fail(BOHIP_E_ARG, "paths_eval: null argument");
    if (R < 1) return fail(BOHIP_E_ARG, "paths_eval: R must be at least 1");
    bohip_gp* g = p->g;
    HIPCHK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    const bool mfma = paths_use_mfma(p);
    // with values the chunk also bounds the S x chunk staging block (128 MiB)
    int64_t chunk = PATHS_CHUNK;
    if (values) chunk = std::max<int64_t>(PM_ROWS, std::min<int64_t>(PATHS_CHUNK, ((int64_t)1 << 24) / p->S / PM_ROWS * PM_ROWS));
    chunk = std::min<int64_t>(chunk, round_up(R, PM_ROWS));
    HIPCHK(p->dXs.reserve((size_t)chunk * p->d, st));
    HIPCHK(p->dV.reserve(values ? (size_t)p->S * chunk : 0, st));
    HIPCHK(p->dpart.reserve(best ? (size_t)p->S * ((chunk + paths_tile(mfma) - 1) / paths_tile(mfma)) : 0, st));
    t_reset(g);
    t_begin(g, "path_eval");
    for (int64_t j0 = 0; j0 < R; j0 += chunk) {
        const int64_t Rc = std::min<int64_t>(chunk, R - j0);
        HIPCHK(hipMemcpyAsync(p->dXs, Xs + j0 * p->d, (size_t)Rc * p->d * 8, hipMemcpyHostToDevice, st));
        CHK(paths_eval_launch(p, p->dXs, Rc, j0, values ? p->dV : nullptr, chunk, best ? p->dbest : nullptr, j0 > 0, false, mfma));
        if (values)
            HIPCHK(hipMemcpy2DAsync(values + j0, (size_t)R * 8, p->dV, (size_t)chunk * 8, (size_t)Rc * 8, (size_t)p->S, hipMemcpyDeviceToHost, st));
    }
    t_end(g);
    if (best) HIPCHK(hipMemcpyAsync(best, p->dbest, (size_t)p->S * sizeof(Best), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    t_collect(g);
    return 0;
}

int bohip_paths_eval_grad(bohip_paths* p, const double* Xs, int64_t R, const int64_t* path_of, double* f, double* grad) {
    if (!p || !Xs || !f || !grad) return fail(BOHIP_E_ARG, "paths_eval_grad: null argument");
    if (R < 1) return fail(BOHIP_E_ARG, "paths_eval_grad: R must be at least 1");
    if (path_of)
        for (int64_t j = 0; j < R; ++j)
            if (path_of[j] < 0 || path_of[j] >= p->S) return fail(BOHIP_E_ARG, "paths_eval_grad: path_of[" + std::to_string(j) + "] names no path");
    bohip_gp* g = p->g;
    HIPCHK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    const int64_t chunk = std::min<int64_t>(PATHS_GRAD_CHUNK, R);
    HIPCHK(p->df.reserve((size_t)chunk, st));
    HIPCHK(p->dg.reserve((size_t)chunk * p->d, st));
    HIPCHK(p->dpath_of.reserve((size_t)chunk, st));
    HIPCHK(p->dXs.reserve((size_t)chunk * p->d, st));
    const PathArgs a = paths_args(p);
    const bool lo = fam_low(p->hp);
    t_reset(g);
    t_begin(g, "path_grad");
    for (int64_t j0 = 0; j0 < R; j0 += chunk) {
        const int64_t Rc = std::min<int64_t>(chunk, R - j0);
        HIPCHK(hipMemcpyAsync(p->dXs, Xs + j0 * p->d, (size_t)Rc * p->d * 8, hipMemcpyHostToDevice, st));
        if (path_of) HIPCHK(hipMemcpyAsync(p->dpath_of, path_of + j0, (size_t)Rc * 8, hipMemcpyHostToDevice, st));
        LAUNCH_FAM(lo, k_path_grad<true>, k_path_grad<false>, dim3((unsigned)Rc), dim3(256), 0, st, a, p->hp, p->dXs, Rc,
                   path_of ? p->dpath_of : (const int64_t*)nullptr, p->df, p->dg);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(f + j0, p->df, (size_t)Rc * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(grad + j0 * p->d, p->dg, (size_t)Rc * p->d * 8, hipMemcpyDeviceToHost, st));
    }
    t_end(g);
    HIPCHK(hipStreamSynchronize(st));
    t_collect(g);
    return 0;
}

int bohip_gp_score(bohip_gp* g, int acq_id, const double* acq_params, const double* Xs, int64_t R, double* score,
                   bohip_best* best) {
    if (!g || R < 0 || (R > 0 && !Xs)) return fail(BOHIP_E_ARG, "bad arguments");
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "unknown acq_id");
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    const double* xin = small_candidates_in_place(g, Xs, R);
    if (!xin) HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    if (R <= SMALL_R && g->hpin) {
        double* pscore = g->pin.score;
        Best* pbest = reinterpret_cast<Best*>(g->pin.rec);
        CHK(score_core(g, acq_id, acq_params, xin ? xin : g->dXs, R, nullptr, nullptr, score ? pscore : nullptr, best ? pbest : nullptr));
        HIPCHK(hipStreamSynchronize(g->stream));
        if (score) std::memcpy(score, pscore, (size_t)R * 8);
        if (best) std::memcpy(best, pbest, sizeof(Best));
        t_collect(g);
        return 0;
    }
    CHK(score_core(g, acq_id, acq_params, g->dXs, R, nullptr, nullptr, score ? g->dscore : nullptr,
                   best ? g->dbest : nullptr));
    if (score) HIPCHK(hipMemcpyAsync(score, g->dscore, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, g->dbest, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// ---- greedy batch selection (an extension: the reference proposes ONE point per iteration, src/BayesianOptimization.jl:185-196) ----
// q picks from one contraction: V' of all R candidates is kept (dBV), every further pick is k_batch_cond + k_batch_final
// (kernels_batch.hip).  All rounds are enqueued without a synchronisation; the model is not touched.
static constexpr size_t BATCH_VT_CAP_BYTES = (size_t)8 << 30;   // V' of one call (R = 32768 at N = 10^4: 2.7 GB)
struct BatchWs { double* U; BatchRec* rec; BatchScal* scal; Best* wg_best; int* picked; };
static int ensure_batch(bohip_gp* g, int64_t R, int64_t q, BatchWs* w) {
    const int64_t rows = round_up(R, TILE) + TILE;
    bool grew = false;   // (ld never changes under a live dBV: alloc_model releases it)
    HIPCHK(g->dBV.reserve((size_t)rows * g->ld, g->stream, Grow::Exact, &grew));
    if (grew) HIPCHK(hipMemsetAsync(g->dBV, 0, (size_t)rows * g->ld * 8, g->stream));   // padding columns (>= N) stay zero
    auto lay = [&](const void* base) { return layout::batch(base, (size_t)q, (size_t)rows, BATCH_WG_MAX, w); };
    HIPCHK(g->dbatch.reserve(lay(nullptr), g->stream));
    lay(g->dbatch);
    return 0;
}

int bohip_gp_select_batch(bohip_gp* g, int acq_id, const double* acq_params, const double* Xs, int64_t R, int64_t q, int fantasy,
                          double fantasy_value, int flags, int64_t* idx, double* val, double* mu, double* var) {
    if (!g || !Xs || !idx || !val || R < 1) return fail(BOHIP_E_ARG, "bad arguments");
    if (acq_id == BOHIP_ACQ_THOMPSON_DRAW) return fail(BOHIP_E_ARG, "select_batch: a posterior draw has no conditioned score");
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "unknown acq_id");
    AcqParams ap;
    CHK(make_acq(acq_id, acq_params, &ap));
    if (q < 1 || q > R) return fail(BOHIP_E_ARG, "select_batch: q must lie in 1..R (q = " + std::to_string(q) + ", R = " + std::to_string(R) + ")");
    if (fantasy != BOHIP_FANTASY_BELIEVER && fantasy != BOHIP_FANTASY_CONST)
        return fail(BOHIP_E_ARG, "select_batch: unknown fantasy " + std::to_string(fantasy));
    if (fantasy == BOHIP_FANTASY_CONST && !std::isfinite(fantasy_value)) return fail(BOHIP_E_ARG, "select_batch: fantasy_value is not finite");
    if (flags & ~BOHIP_BATCH_RAISE_TAU) return fail(BOHIP_E_ARG, "select_batch: unknown flags");
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    if (q == 1) {   // one pick is the plain arg-max: bohip_gp_score's record (and its pruned pass)
        bohip_best b{-INFINITY, -1};
        CHK(bohip_gp_score(g, acq_id, acq_params, Xs, R, nullptr, &b));
        idx[0] = b.idx; val[0] = b.val;
        double m = NAN, v = NAN;
        if ((mu || var) && b.idx >= 0) CHK(bohip_gp_predict(g, Xs + b.idx * g->d, 1, &m, &v));
        if (mu) mu[0] = m;
        if (var) var[0] = v;
        return 0;
    }
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_fresh(g));
    const int64_t rows = round_up(R, TILE) + TILE;
    if ((size_t)rows * (g->ld + q) * 8 > BATCH_VT_CAP_BYTES)   // V' [rows][ld] and the q rows of u_i
        return fail(BOHIP_E_UNSUPPORTED, "select_batch: V' of " + std::to_string(R) + " candidates needs " +
                                             std::to_string((size_t)rows * (g->ld + q) * 8) + " bytes, above the cap of " +
                                             std::to_string(BATCH_VT_CAP_BYTES) + " (at this model size R <= " +
                                             std::to_string((int64_t)(BATCH_VT_CAP_BYTES / ((size_t)(g->ld + q) * 8)) - 2 * TILE) + ")");
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    CHK(one_time_kernel_setup());
    BatchWs bw;
    CHK(ensure_batch(g, R, q, &bw));
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    // round 0 is the batched pass (K*' chunk -> k_trigemm_sq with V' stored), whatever R is: the other routes do not leave V' in this layout
    const PassPlan pl = choose_route(g, R, WHOLE_K_ONLY);
    const int64_t N = pl.dm.N, Rpad = pl.dm.Rpad, ld = pl.dm.ld;
    const KernelHyper hp = make_hyper(g);
    double* U = bw.U;
    BatchRec* rec = bw.rec;
    BatchScal* scal = bw.scal;
    Best* wg_best = bw.wg_best;
    int* picked = bw.picked;
    HIPCHK(hipMemsetAsync(picked, 0, (size_t)rows * sizeof(int), g->stream));
    const int64_t chunks = chunk_pass(g, pl, g->dXs, hp, ChunkV{g->dBV, ld}, false, FuseParams{}, no_finish);
    if (chunks < 0) return (int)chunks;
    g->score_launches = chunks;
    t_begin(g, "batch_rounds");
    const int nb = (int)((R + 255) / 256);
    hipLaunchKernelGGL(k_score, dim3(nb), dim3(256), 0, g->stream, g->dq, Rpad, pl.dq_tiles(), g->dmu_raw, R, hp.sigma2, g->beta, ap, g->dmu, g->dvar,
                       (double*)nullptr, g->dblock_best);
    BatchFinal bf{};
    bf.mu = g->dmu; bf.var = g->dvar; bf.picked = picked; bf.rec = rec; bf.scal = scal; bf.fantasy = fantasy;
    bf.fantasy_value = fantasy_value; bf.tau0 = ap.p0;
    bf.noise = std::exp(2.0 * g->lognoise) + std::numeric_limits<double>::epsilon() + g->jitter_last;   // as on cK's diagonal
    bf.raise_tau = (flags & BOHIP_BATCH_RAISE_TAU) && (acq_id == BOHIP_ACQ_EI || acq_id == BOHIP_ACQ_PI || acq_id == BOHIP_ACQ_LOGEI);
    bf.in = g->dblock_best; bf.n = nb; bf.t = 0;
    hipLaunchKernelGGL(k_batch_final, dim3(1), dim3(256), 0, g->stream, bf);
    BatchCond bc{};
    bc.VT = g->dBV; bc.ldv = ld; bc.N = N; bc.Xs = g->dXs; bc.R = R; bc.mu = g->dmu; bc.var = g->dvar; bc.U = U; bc.ldu = rows;
    bc.picked = picked; bc.rec = rec; bc.scal = scal; bc.ap = ap; bc.block_best = wg_best;
    const size_t lds = (size_t)(N / 2) * 16;
    bc.use_lds = lds <= (size_t)BATCH_LDS_MAX;
    const int nwg = (int)std::min<int64_t>((R + BATCH_WAVES - 1) / BATCH_WAVES, BATCH_WG_MAX);
    bf.in = wg_best; bf.n = nwg;
    for (int64_t t = 0; t + 1 < q; ++t) {
        bc.t = (int)t;
        LAUNCH_FAM(fam_low(hp), k_batch_cond<true>, k_batch_cond<false>, dim3(nwg), dim3(64 * BATCH_WAVES), bc.use_lds ? lds : 0, g->stream, bc, hp);
        bf.t = (int)t + 1;
        hipLaunchKernelGGL(k_batch_final, dim3(1), dim3(256), 0, g->stream, bf);
    }
    HIPCHK(hipGetLastError());
    t_end(g);
    std::vector<BatchRec> h((size_t)q);
    HIPCHK(hipMemcpyAsync(h.data(), rec, (size_t)q * sizeof(BatchRec), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    for (int64_t t = 0; t < q; ++t) {
        idx[t] = h[t].idx; val[t] = h[t].val;
        if (mu) mu[t] = h[t].mu;
        if (var) var[t] = h[t].var;
    }
    t_collect(g);
    return 0;
}

int bohip_gp_score_grad(bohip_gp* g, int acq_id, const double* acq_params, const double* Xs, int64_t R, double* score,
                        double* grad) {
    if (!g || R < 0 || (R > 0 && (!Xs || !score || !grad))) return fail(BOHIP_E_ARG, "bad arguments");
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "unknown acq_id");
    if (R == 0) return 0;
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_xs(g, R));
    HIPCHK(g->dgrad.reserve((size_t)R * g->d, g->stream));
    double* dgrad = g->dgrad;
    const double* xin = small_candidates_in_place(g, Xs, R);
    if (!xin) HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    int rc = ensure_score_scratch(g, R);
    if (rc == 0 && R <= SMALL_R && g->hpin) {
        double *pscore = g->pin.score, *pgrad = g->pin.grad;
        rc = score_grad_core(g, acq_id, acq_params, xin ? xin : g->dXs, R, pscore, pgrad);
        if (rc == 0) {
            const hipError_t e = hipStreamSynchronize(g->stream);
            if (e != hipSuccess) rc = fail(BOHIP_E_HIP, hipGetErrorString(e));
        }
        if (rc == 0) {
            std::memcpy(score, pscore, (size_t)R * 8);
            std::memcpy(grad, pgrad, (size_t)R * g->d * 8);
        }
        t_collect(g);
        return rc;
    }
    if (rc == 0) rc = score_grad_core(g, acq_id, acq_params, g->dXs, R, g->dscore, dgrad);
    if (rc == 0) {
        hipError_t e = hipMemcpyAsync(score, g->dscore, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(grad, dgrad, (size_t)R * g->d * 8, hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = fail(BOHIP_E_HIP, hipGetErrorString(e));
    }
    t_collect(g);
    return rc;
}

static int ensure_ascent(bohip_gp* g, int64_t R) {
    HIPCHK(g->asc_bounds.reserve((size_t)3 * DMAX, g->stream));
    HIPCHK(g->asc_best.reserve(1, g->stream));
    if (g->asc_rows >= R && g->asc_block && g->asc_ints && g->asc_hints) return 0;
    // the three blocks behind asc are laid out for `cap` starts (at least 32) and re-made together
    const size_t cap = (size_t)std::max<int64_t>(R, 32);
    AscentState& a = g->asc;
    g->asc_rows = 0;
    const size_t nd = layout::ascent_doubles(nullptr, cap, (size_t)g->d, ASC_M, &a), ni = layout::ascent_words(nullptr, cap, ASC_RING, &a),
                 nh = layout::ascent_pinned(nullptr, cap, ASC_RING, &a);
    HIPCHK(g->asc_block.reserve(nd, g->stream));
    HIPCHK(g->asc_ints.reserve(ni, g->stream));
    HIPCHK(g->asc_hints.reserve(nh, g->stream));
    HIPCHK(hipMemset(g->asc_ints, 0, ni));
    std::memset(g->asc_hints, 0, nh);
    layout::ascent_doubles(g->asc_block, cap, (size_t)g->d, ASC_M, &a);
    layout::ascent_words(g->asc_ints, cap, ASC_RING, &a);
    layout::ascent_pinned(g->asc_hints, cap, ASC_RING, &a);
    g->asc_rows = (int64_t)cap;
    return 0;
}

// acquire_max(acquisition, model, lb, ub, restarts) for the gradient-based methods (reference src/acquisition.jl:48-68 with
// nlopt_setup :23-35): lock-step projected L-BFGS ascent from R start columns, state resident in HBM.
// bohip_gp_acquire_max is a prologue (validation, scratch, the pinned [lb | ub | starts] block), ONE of three drivers, and an epilogue
// (ascent_read_result).  What the prologue made and the drivers share:
struct AscentCall {
    int acq_id, d;
    const double* acq_params;
    AcqParams ap;
    int64_t R, maxeval;
    double ftol_rel, xtol_abs, first_step;   // first_step: g_asc_first_step x the smallest box side
    double *dlb, *dub, *dstarts, *dbx;       // the [lb | ub | starts] block where it landed on the device; the winner's coordinates
    double* hout;                            // pinned: k_asc_final's packed result [best 2 | best_x d | f R | x R d | passes R]
};
// NLopt's maxtime (reference src/acquisition.jl:24-27 forwards it): checked once per iteration
static bool ascent_out_of_time(const bohip_gp* g, std::chrono::steady_clock::time_point t_start) {
    return g->asc_maxtime > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() >= g->asc_maxtime;
}
// The final arg-max, and the call's ONE synchronisation.  The packed result goes straight into the pinned host block (second half: the
// first holds the inputs): ~100 doubles written by one workgroup, no copy command behind the kernel (~10 us of a 0.2-0.4 ms call).
static int ascent_finish(bohip_gp* g, const AscentCall& c, const int* passes) {
    hipLaunchKernelGGL(k_asc_final, dim3(1), dim3(256), 0, g->stream, g->asc, c.d, (int)c.R, g->asc_best, c.dbx, c.hout, passes);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}
static void ascent_read_result(const AscentCall& c, const double* lb, bohip_best* best, double* best_x, double* f_out, double* x_out) {
    const double* hout = c.hout;
    const int64_t d = c.d, R = c.R;
    if (best) { best->val = hout[0]; best->idx = (long long)hout[1]; }
    if (best_x) for (int k = 0; k < d; ++k) best_x[k] = hout[1] >= 0.0 ? hout[2 + k] : lb[k];   // :56  maxx = lowerbounds when nothing beat -Inf
    if (f_out) std::memcpy(f_out, hout + 2 + d, (size_t)R * 8);
    if (x_out) std::memcpy(x_out, hout + 2 + d + R, (size_t)R * d * 8);
}

// small models: one workgroup per start point runs its whole ascent, ONE launch (kernels_ascent.hip k_ascent_wg)
static int ascent_one_launch(bohip_gp* g, const AscentCall& c, int64_t* evals) {
    const AscentState& st = g->asc;
    const int d = c.d; const int64_t R = c.R;
    AscWgParams pw{};
    pw.W = g->dW; pw.WT = g->dWT; pw.X = g->dX; pw.alpha = g->dalpha; pw.ld = g->ld; pw.N = g->n;
    pw.hp = make_hyper(g); pw.ap = c.ap;
    pw.beta = g->beta; pw.st = st; pw.starts = c.dstarts; pw.lb = c.dlb; pw.ub = c.dub; pw.R = (int)R;
    pw.maxeval = (int)std::min<int64_t>(c.maxeval, 1 << 30); pw.ftol_rel = c.ftol_rel; pw.xtol_abs = c.xtol_abs; pw.first_step_scale = c.first_step;
    pw.max_ticks = g->asc_maxtime > 0.0 ? (unsigned long long)(g->asc_maxtime * 1e8) : 0ull;
    pw.passes = st.accepted;
    t_begin(g, "ascent_wg");
    const bool lo = fam_low(pw.hp);
    if (d > 8 && pw.ap.acq == ACQ_LOGEI)   // (the instantiation of its own: kernels_ascent.hip k_ascent_wg_logei16)
        LAUNCH_FAM(lo, (k_ascent_wg_logei16<true>), (k_ascent_wg_logei16<false>), dim3((unsigned)R), dim3(AWG_THREADS), 0, g->stream, pw);
    else   // (this driver: d <= 16)
        dispatch_dt<16>(d, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            LAUNCH_FAM(lo, (k_ascent_wg<DT, true>), (k_ascent_wg<DT, false>), dim3((unsigned)R), dim3(AWG_THREADS), 0, g->stream, pw);
        });
    HIPCHK(hipGetLastError());
    t_end(g);
    CHK(ascent_finish(g, c, st.accepted));
    const double* passes = c.hout + 2 + d + R + (size_t)R * d;   // (>= 0, R >= 1)
    *evals = (int64_t)*std::max_element(passes, passes + R);
    return 0;
}

// FREE-RUNNING driver (k_asc_step): pass after pass is enqueued without waiting; how many start points are still active after pass e is read LAG
// passes later from pinned memory (long written by then: no stall), so at most LAG passes run beyond convergence.  The lock-step driver's trajectories.
static int ascent_free_running(bohip_gp* g, const AscentCall& c, int64_t* evals_out) {
    const AscentState& st = g->asc;
    const int d = c.d; const int64_t R = c.R; const unsigned nR = (unsigned)R;
    const int LAG = 1;   // (2 until round 4: with 17 passes per call instead of 228 a wasted pass is 5 % of it; one queued pass keeps the device fed)
    // (the counters of a pass clear themselves; this is for a call that was cut short -- queued before the start kernel, where the device
    // waits for the host's copy anyway)
    HIPCHK(hipMemsetAsync(st.nact, 0, (size_t)2 * ASC_RING * sizeof(unsigned), g->stream));
    for (int i = 0; i < ASC_RING; ++i) st.h_cnt[i] = 0;
    hipLaunchKernelGGL(k_asc_start, dim3(nR), dim3(64), 0, g->stream, st, d, c.dstarts, c.dlb, c.dub);
    bool first_folded = false;   // the start points' adoption and first direction ran in the gradient kernel's last workgroup (SmallFold, on = 2)
    SmallFold fold0{};
    fold0.on = 2; fold0.R = (int)R; fold0.ring_slot = ASC_RING - 1; fold0.st = st; fold0.lb = c.dlb; fold0.ub = c.dub; fold0.first_step_scale = c.first_step;
    CHK(score_grad_core(g, c.acq_id, c.acq_params, st.Xt, R, st.ft, st.Gt, AscPass{g_asc_fold ? &fold0 : nullptr, nullptr, &first_folded}));
    if (!first_folded) {
        // no synchronisation here: how many start points are active at all is counted by the adopt kernel into the ring slot the host reads
        // once the first pass is queued (below)
        hipLaunchKernelGGL(k_asc_adopt_count, dim3(nR), dim3(64), 0, g->stream, st, d, (int)R, ASC_RING - 1);
        HIPCHK(hipGetLastError());
    }
    int64_t evals = 1;
    const auto t_start = std::chrono::steady_clock::now();
    if (!first_folded) hipLaunchKernelGGL(k_asc_direction, dim3(nR), dim3(64), 0, g->stream, st, d, (int)R, 0, 0, c.dlb, c.dub, c.first_step);
    int64_t e = 0, converged_at = -1;
    bool none_active = false;
    auto read_count = [&](int64_t pass) -> int {   // active start points after `pass` (waits for it if need be)
        volatile int* w = st.h_cnt + (pass % ASC_RING);
        const auto t0 = std::chrono::steady_clock::now();
        int v;
        while ((v = *w) == 0) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 30.0) return -1;
        }
        *w = 0;
        return v - 1;
    };
    for (; evals < c.maxeval && !ascent_out_of_time(g, t_start); ++e) {
        SmallFold fold{};
        fold.on = 1; fold.R = (int)R; fold.ring_slot = (int)(e % ASC_RING); fold.st = st; fold.lb = c.dlb; fold.ub = c.dub; fold.ftol_rel = c.ftol_rel; fold.xtol_abs = c.xtol_abs;
        bool folded = false;
        CHK(score_grad_core(g, c.acq_id, c.acq_params, st.Xt, R, st.ft, st.Gt, AscPass{g_asc_fold ? &fold : nullptr, st.ticket, &folded}));
        ++evals;
        if (!folded)   // (more than 16 start points, d > 16, or the batch took another path: the step as a launch of its own)
            hipLaunchKernelGGL(k_asc_step, dim3(nR), dim3(64), 0, g->stream, st, d, (int)R, c.dlb, c.dub, c.first_step, c.ftol_rel, c.xtol_abs,
                               (int)(e % ASC_RING));
        HIPCHK(hipGetLastError());
        if (e == 0) {   // the adopt kernel's count (the device is busy with the first pass meanwhile)
            const int n0 = read_count(ASC_RING - 1);
            if (n0 < 0) return fail(BOHIP_E_HIP, "device ascent: the first evaluation did not report back within 30 s");
            if (n0 == 0) { none_active = true; ++e; break; }   // no start point with a finite value: the queued pass changes nothing
        }
        if (e >= LAG) {
            const int n = read_count(e - LAG);
            if (n < 0) return fail(BOHIP_E_HIP, "device ascent: an evaluation pass did not report back within 30 s");
            if (n == 0) { converged_at = e - LAG; ++e; break; }
        }
    }
    CHK(ascent_finish(g, c, nullptr));   // (queued behind the last pass at once; the counts of the last LAG passes are looked at after it)
    if (converged_at < 0)   // stopped by maxeval / maxtime, or converged within the last LAG passes
        for (int64_t p2 = std::max<int64_t>(0, e - LAG); p2 < e && converged_at < 0; ++p2)
            if (st.h_cnt[p2 % ASC_RING] == 1) converged_at = p2;
    if (converged_at >= 0) evals = 2 + converged_at;   // passes that were needed: the first one + passes 0 .. converged_at
    if (none_active) evals = 1;
    *evals_out = evals;
    return 0;
}

// LOCK-STEP driver (BOHIP_ASC_LOCKSTEP=1): five launches and a stream synchronisation per evaluation pass, the host decides between passes
static int ascent_lock_step(bohip_gp* g, const AscentCall& c, int64_t* evals_out) {
    const AscentState& st = g->asc;
    const int d = c.d; const int64_t R = c.R; const unsigned nR = (unsigned)R;
    auto any_of = [&](const int* v, int want) { return std::any_of(v, v + R, [&](int x) { return (x != 0) == (want != 0); }); };
    hipLaunchKernelGGL(k_asc_start, dim3(nR), dim3(64), 0, g->stream, st, d, c.dstarts, c.dlb, c.dub);
    CHK(score_grad_core(g, c.acq_id, c.acq_params, st.Xt, R, st.ft, st.Gt));
    hipLaunchKernelGGL(k_asc_adopt, dim3(nR), dim3(64), 0, g->stream, st, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g->stream));
    bool any_active = any_of(st.h_active, 1);
    int64_t evals = 1;
    int nh = 0, it = 0;
    const auto t_start = std::chrono::steady_clock::now();
    while (evals < c.maxeval && any_active && !ascent_out_of_time(g, t_start)) {
        hipLaunchKernelGGL(k_asc_direction, dim3(nR), dim3(64), 0, g->stream, st, d, (int)R, nh, (it + ASC_M - 1) % ASC_M, c.dlb, c.dub,
                           c.first_step);
        for (int bt = 0; bt < ASC_MAX_BT; ++bt) {   // backtracking Armijo, all start points per device pass
            CHK(score_grad_core(g, c.acq_id, c.acq_params, st.Xt, R, st.ft, st.Gt));
            ++evals;
            hipLaunchKernelGGL(k_asc_linesearch, dim3(nR), dim3(64), 0, g->stream, st, d, c.dlb, c.dub);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(g->stream));
            if (bt == 0 && it > 0) any_active = any_of(st.h_active, 1);   // written by the previous k_asc_update
            if (!any_of(st.h_accepted, 0) || evals >= c.maxeval || !any_active) break;
        }
        if (!any_active) { --evals; break; }   // the speculative evaluation of an already converged set is not counted
        hipLaunchKernelGGL(k_asc_update, dim3(nR), dim3(64), 0, g->stream, st, d, (int)R, it % ASC_M, c.ftol_rel, c.xtol_abs);
        nh = std::min(nh + 1, ASC_M);
        ++it;
    }
    CHK(ascent_finish(g, c, nullptr));
    *evals_out = evals;
    return 0;
}

int bohip_gp_acquire_max(bohip_gp* g, int acq_id, const double* acq_params, const double* lb, const double* ub,
                         const double* starts, int64_t R, int64_t maxeval, double ftol_rel, double xtol_abs, double* x_out,
                         double* f_out, bohip_best* best, double* best_x, int64_t* evals_out) {
    if (!g || !lb || !ub || R < 0 || (R > 0 && !starts)) return fail(BOHIP_E_ARG, "bad arguments");
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "unknown acq_id");
    AscentCall c{};
    c.acq_id = acq_id; c.acq_params = acq_params; c.R = R; c.maxeval = maxeval; c.ftol_rel = ftol_rel; c.xtol_abs = xtol_abs;
    CHK(make_acq(acq_id, acq_params, &c.ap));
    if (evals_out) *evals_out = 0;
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    const int d = c.d = g->d;
    for (int k = 0; k < d; ++k)
        if (!(lb[k] <= ub[k])) return fail(BOHIP_E_ARG, "lowerbounds must not exceed upperbounds");
    CHK(ensure_fresh(g));
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    CHK(ensure_ascent(g, R));
    AscentState& st = g->asc;
    st.ftol_abs = g->asc_ftol_abs; st.xtol_rel = g->asc_xtol_rel; st.stopval = g->asc_stopval;
    // one pinned block in ([lb | ub | starts]), one pinned block out (k_asc_final's packed result): seven pageable copies were ~0.1 ms
    // of a call that is 1.3 ms at N = 3000 since the search needs 17 passes instead of 228
    const size_t n_in = (size_t)(2 + R) * d, n_out = (size_t)2 + d + R + (size_t)R * d + R, n_io = std::max(n_in, n_out);
    if (n_io > g->asc_hio.capacity() || n_io > g->asc_dio.capacity()) {   // (room for twice the call that grows them)
        HIPCHK(g->asc_hio.reserve(n_io * 2, g->stream));
        HIPCHK(g->asc_dio.reserve(n_io * 2, g->stream));
    }
    std::memcpy(g->asc_hio, lb, (size_t)d * 8);
    std::memcpy(g->asc_hio + d, ub, (size_t)d * 8);
    std::memcpy(g->asc_hio + 2 * d, starts, (size_t)R * d * 8);
    HIPCHK(hipMemcpyAsync(g->asc_dio, g->asc_hio, n_in * 8, hipMemcpyHostToDevice, g->stream));
    c.dlb = g->asc_dio; c.dub = g->asc_dio + d; c.dstarts = g->asc_dio + 2 * d;   // (the kernels read the bounds and the starts where the block landed)
    c.dbx = g->asc_bounds + 2 * DMAX;
    c.hout = g->asc_hio + n_io;
    double span = INFINITY;
    for (int k = 0; k < d; ++k) span = std::min(span, ub[k] - lb[k] + 1e-300);
    c.first_step = g_asc_first_step * span;
    const bool use_wg = g_asc_wg_nmax > 0 && g->n <= std::min<int64_t>(g_asc_wg_nmax, AWG_NMAX - 1) && d <= 16 && !g_asc_lockstep;
    int64_t evals = 0;
    if (use_wg) CHK(ascent_one_launch(g, c, &evals));
    else if (!g_asc_lockstep) CHK(ascent_free_running(g, c, &evals));
    else CHK(ascent_lock_step(g, c, &evals));
    ascent_read_result(c, lb, best, best_x, f_out, x_out);
    if (evals_out) *evals_out = evals;
    t_collect(g);
    return 0;
}

double bohip_thompson_normal(uint64_t seed, int64_t s, int64_t j) { return thompson_normal(seed, s, j); }

// ---- :GN_DIRECT_L (reference src/acquisition.jl:7-9, :20-38): the dividing-rectangles search, bookkeeping in direct_l.h ----
struct bohip_direct { DirectL s; };

int bohip_direct_create(int64_t d, const double* lb, const double* ub, int64_t maxeval, double stopval, double maxtime,
                        bohip_direct** out) {
    if (d < 1 || !lb || !ub || !out) return fail(BOHIP_E_ARG, "bad arguments");
    for (int64_t i = 0; i < d; ++i)
        if (!(lb[i] <= ub[i])) return fail(BOHIP_E_ARG, "direct: lower bound above upper bound");
    try {
        *out = new bohip_direct{DirectL(d, lb, ub, maxeval, stopval, maxtime)};
    } catch (const std::exception& e) { return fail(BOHIP_E_ARG, e.what()); }
    return 0;
}
void bohip_direct_destroy(bohip_direct* s) { delete s; }
int bohip_direct_ask(bohip_direct* s, double* X, int64_t cap, int64_t* n) {
    if (!s || !n || cap < 0 || (cap > 0 && !X)) return fail(BOHIP_E_ARG, "bad arguments");
    if (cap == 0) {   // size query: plans the iteration, hands out nothing yet
        try { *n = s->s.plan_next(); } catch (const std::exception& e) { return fail(BOHIP_E_ARG, e.what()); }
        return 0;
    }
    int64_t m = 0;
    try { m = s->s.ask(X, cap); } catch (const std::exception& e) { return fail(BOHIP_E_ARG, e.what()); }
    if (m < 0) return fail(BOHIP_E_ARG, "direct: the buffer is smaller than this iteration's batch (maxeval columns always suffice)");
    *n = m;
    return 0;
}
int bohip_direct_tell(bohip_direct* s, const double* f, int64_t n) {
    if (!s || !f || n < 1) return fail(BOHIP_E_ARG, "bad arguments");
    try {
        if (!s->s.tell(f, n)) return fail(BOHIP_E_STATE, "direct: tell without a matching ask");
    } catch (const std::exception& e) { return fail(BOHIP_E_ARG, e.what()); }   // (nothing throws across the ABI: allocation failures end here)
    return 0;
}
int bohip_direct_best(const bohip_direct* s, double* best_f, double* best_x, int64_t* evaluations, int64_t* iterations) {
    if (!s) return fail(BOHIP_E_ARG, "bad arguments");
    const double f = s->s.best(best_x);
    if (best_f) *best_f = f;
    if (evaluations) *evaluations = s->s.evals;
    if (iterations) *iterations = s->s.iterations;
    return 0;
}

// The whole search in one call: ask -> ONE scoring call of the iteration's points -> tell, until DIRECT-L stops.
// acq_id = BOHIP_ACQ_THOMPSON_DRAW: the objective is x -> myrand(model, x) (src/acquisitionfunctions.jl:107-108), one posterior draw
// per evaluated point, mu + sigma z with z = bohip_thompson_normal(seed, 0, e) for the e-th evaluation of the search.
int bohip_gp_direct_max(bohip_gp* g, int acq_id, const double* acq_params, const double* lb, const double* ub, int64_t maxeval,
                        double stopval, double maxtime, uint64_t seed, double* best_f, double* best_x, int64_t* evaluations,
                        int64_t* device_calls) {
#pragma clang fp contract(off)
    if (!g || !lb || !ub) return fail(BOHIP_E_ARG, "bad arguments");
    if (!acq_id_scores(acq_id) && acq_id != BOHIP_ACQ_THOMPSON_DRAW) return fail(BOHIP_E_ARG, "unknown acq_id");
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    const int64_t d = g->d;
    for (int64_t i = 0; i < d; ++i)
        if (!(lb[i] <= ub[i])) return fail(BOHIP_E_ARG, "direct: lower bound above upper bound");
    try {
    DirectL s(d, lb, ub, maxeval, stopval, maxtime);
    std::vector<double> X, f, var;
    int64_t calls = 0, e = 0;
    for (;;) {
        const int64_t m = s.plan_next();       // (an iteration's batch is at most 2 d points per potentially optimal rectangle)
        if (m == 0) break;
        if ((int64_t)f.size() < m) { X.resize((size_t)m * d); f.resize(m); var.resize(m); }
        s.ask(X.data(), m);
        if (acq_id == BOHIP_ACQ_THOMPSON_DRAW) {
            CHK(bohip_gp_predict(g, X.data(), m, f.data(), var.data()));
            for (int64_t c = 0; c < m; ++c, ++e) {
                const double sd = std::sqrt(std::max(var[c], 0.0));
                const double t = sd * thompson_normal(seed, 0, e);
                f[c] = f[c] + t;
            }
        } else {
            CHK(bohip_gp_score(g, acq_id, acq_params, X.data(), m, f.data(), nullptr));
        }
        ++calls;
        s.tell(f.data(), m);
    }
    const double bf = s.best(best_x);
    if (best_f) *best_f = bf;
    if (evaluations) *evaluations = s.evals;
    if (device_calls) *device_calls = calls;
    } catch (const std::exception& e) { return fail(BOHIP_E_ARG, e.what()); }   // (nothing throws across the ABI)
    return 0;
}

// include/bohip_acq.h: the functors on their own (no model: the current device, the default stream, buffers of the call)
int bohip_acq_eval(int acq_id, const double* acq_params, int64_t n, const double* mu, const double* var, double* value,
                   double* dmu, double* dvar) {
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "unknown acq_id");
    AcqParams ap;
    CHK(make_acq(acq_id, acq_params, &ap));
    if (n < 0 || (n > 0 && (!mu || !var || !value)) || (!dmu != !dvar)) return fail(BOHIP_E_ARG, "bad arguments");
    if (n == 0) return 0;
    if (n > (int64_t)1 << 31) return fail(BOHIP_E_UNSUPPORTED, "acq_eval: more than 2^31 elements");
    if (bohip_device_count() <= 0) return fail(BOHIP_E_NODEVICE, "no HIP device visible; libbohip has no CPU fallback");
    const int nout = dmu ? 3 : 1;
    DBuf<double> buf;   // (freed when the call leaves)
    HIPCHK(buf.reserve((size_t)n * (2 + nout), (hipStream_t)0));
    double *d_mu = buf, *d_var = buf + n, *d_val = buf + 2 * n, *d_dmu = dmu ? buf + 3 * n : nullptr, *d_dvar = dmu ? buf + 4 * n : nullptr;
    hipError_t e = hipMemcpy(d_mu, mu, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_var, var, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_acq_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)0, ap, n, d_mu, d_var, d_val, d_dmu, d_dvar);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(value, d_val, (size_t)n * 8, hipMemcpyDeviceToHost);   // (blocking: waits for the kernel)
    if (e == hipSuccess && dmu) e = hipMemcpy(dmu, d_dmu, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dmu) e = hipMemcpy(dvar, d_dvar, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(BOHIP_E_HIP, std::string("acq_eval: ") + hipGetErrorString(e));
    return 0;
}

int bohip_gp_thompson(bohip_gp* g, const double* Xs, int64_t R, int64_t S, uint64_t seed, int64_t j0, bohip_best* best) {
    if (!g || R <= 0 || S <= 0 || !Xs || !best) return fail(BOHIP_E_ARG, "bad arguments");
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    CHK(score_core(g, BOHIP_ACQ_MAXMEAN, nullptr, g->dXs, R, g->dmu, g->dvar, nullptr, nullptr));
    CHK(ensure_thompson(g, S));
    Best* dout = g->dthompson;
    t_begin(g, "thompson");
    hipLaunchKernelGGL(k_thompson, dim3(S), dim3(256), 0, g->stream, g->dmu, g->dvar, R, seed, j0, dout, 0ll);
    t_end(g);
    hipError_t e = hipMemcpyAsync(best, dout, S * sizeof(Best), hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    if (e != hipSuccess) return fail(BOHIP_E_HIP, hipGetErrorString(e));
    t_collect(g);
    return 0;
}

int bohip_gp_set_stream(bohip_gp* g, void* stream) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(g->stream));
    g->stream = stream ? (hipStream_t)stream : g->own_stream;
    return 0;
}
int bohip_gp_synchronize(bohip_gp* g) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

int bohip_gp_get_factor(bohip_gp* g, double* L) {
    if (!g || !L) return fail(BOHIP_E_ARG, "null argument");
    HIPCHK(hipSetDevice(g->device));
    CHK(ensure_fresh(g));
    if (g->n == 0) return 0;
    HIPCHK(hipMemcpy2DAsync(L, g->n * 8, g->dL, g->ld * 8, g->n * 8, g->n, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}
int bohip_gp_get_alpha(bohip_gp* g, double* alpha) {
    if (!g || !alpha) return fail(BOHIP_E_ARG, "null argument");
    HIPCHK(hipSetDevice(g->device));
    CHK(ensure_fresh(g));
    if (g->n == 0) return 0;
    HIPCHK(hipMemcpyAsync(alpha, g->dalpha, g->n * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}
static int comm_nranks(const bohip_gp* g, int64_t* value);
static int comm_rccl_version(int64_t* value);
int bohip_gp_info(const bohip_gp* g, int what, int64_t* value) {
    if (!g || !value) return fail(BOHIP_E_ARG, "null argument");
    switch (what) {
        case BOHIP_INFO_PIVOT: *value = g->pivot; return 0;
        case BOHIP_INFO_CAPACITY: *value = g->cap; return 0;
        case BOHIP_INFO_REFITS: *value = g->refits; return 0;
        case BOHIP_INFO_APPENDS: *value = g->appends; return 0;
        case BOHIP_INFO_CHOL_FORM: *value = g->chol_form_last; return 0;
        case BOHIP_INFO_CHOL_FALLBACKS: *value = g->chol_fallbacks; return 0;
        case BOHIP_INFO_CHOL_ABORT_TILES: *value = g->chol_abort_T; return 0;
        case BOHIP_INFO_JITTER_STEPS: *value = g->jitter_steps_last; return 0;
        case BOHIP_INFO_SCORE_LAUNCHES: *value = g->score_launches; return 0;
        case BOHIP_INFO_SCORE_CHUNK: *value = g->score_chunk; return 0;
        case BOHIP_INFO_KERNEL_CLOCK_MHZ: {   // since the previous read; synchronises the handle's stream
            *value = 0;
            if (!g->dclk) return 0;
            unsigned long long c[2] = {0, 0};
            if (hipSetDevice(g->device) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess ||
                hipMemcpy(c, g->dclk, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess || hipMemset(g->dclk, 0, sizeof(c)) != hipSuccess)
                return fail(BOHIP_E_HIP, "reading the clock sample failed");
            if (c[1] > 0) *value = (int64_t)((double)c[0] / (double)c[1] * 100.0 + 0.5);   // wall_clock64 ticks at 100 MHz
            return 0;
        }
        case BOHIP_INFO_COMM_NRANKS: return comm_nranks(g, value);   // read back from the communicator (multigpu.hip)
        case BOHIP_INFO_COMM_EXCHANGES: *value = g->comm_exchanges; return 0;
        case BOHIP_INFO_COMM_RCCL_VERSION: return comm_rccl_version(value);
        case BOHIP_INFO_CHOL_LOCK_SKIPS: *value = g->chol_lock_skips; return 0;
        default: return fail(BOHIP_E_ARG, "unknown info id");
    }
}
int bohip_gp_set_batch_hint(bohip_gp* g, int64_t total_candidates) {
    if (!g || total_candidates < 0) return fail(BOHIP_E_ARG, "bad arguments");
    g->batch_hint = total_candidates;
    return 0;
}
int bohip_gp_set_jitter(bohip_gp* g, double rel, int max_tries) {
    if (!g || !(rel >= 0.0) || max_tries < 0 || max_tries > 32) return fail(BOHIP_E_ARG, "bad arguments");
    g->jitter_rel = rel;
    g->jitter_tries = rel > 0.0 ? max_tries : 0;
    return 0;
}
int bohip_gp_set_maxtime(bohip_gp* g, double seconds) {
    if (!g || !(seconds >= 0.0)) return fail(BOHIP_E_ARG, "bad arguments");
    g->asc_maxtime = seconds;
    return 0;
}
int bohip_gp_set_ascent_stop(bohip_gp* g, double ftol_abs, double xtol_rel, double stopval) {
    if (!g || !(ftol_abs >= 0.0) || !(xtol_rel >= 0.0) || stopval != stopval) return fail(BOHIP_E_ARG, "bad arguments");
    g->asc_ftol_abs = ftol_abs;
    g->asc_xtol_rel = xtol_rel;
    g->asc_stopval = stopval;
    return 0;
}
int bohip_gp_enable_timing(bohip_gp* g, int on) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    g->timing = on != 0;
    g->timing_dominant_only = on == 2 || on == 3;
    g->timing_accumulate = on == 3;
    g->tused = 0;
    g->tlabel.clear();
    return 0;
}
int bohip_gp_get_timing(bohip_gp* g, const char** names, double* ms, int cap) {
    if (!g) return 0;
    if (g->timing_accumulate) {   // everything recorded since enable_timing(3) / the previous read
        hipSetDevice(g->device);
        t_collect(g, true);
    }
    const int n = (int)std::min<size_t>(g->tnames.size(), cap > 0 ? cap : 0);
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = g->tnames[i].c_str();
        if (ms) ms[i] = g->tms[i];
    }
    return (int)g->tnames.size();
}

// ---- pending evaluations (include/bohip_pend.h; kernels_pend.hip) -----------------------------------------------------
// An extension: the reference evaluates one point at a time (src/BayesianOptimization.jl:185-196).  The set lives on the handle as the
// caller gave it; V_p', mu_p, Sigma_p and L_p are derived lazily and kept while the model and the set they were computed from stand.
using PendCallWs = layout::PendCall<Best>;
static bool pend_tau_acq(int acq_id) { return acq_id == BOHIP_ACQ_EI || acq_id == BOHIP_ACQ_PI || acq_id == BOHIP_ACQ_LOGEI; }
static double pend_noise(const bohip_gp* g) {   // as on cK's diagonal
    return std::exp(2.0 * g->lognoise) + std::numeric_limits<double>::epsilon() + g->jitter_last;
}
static bohip_gp::PendKey pend_key_now(const bohip_gp* g) {
    bohip_gp::PendKey k;
    k.n = g->n; k.ld = g->ld; k.refits = g->refits; k.appends = g->appends; k.hyper_gen = g->hyper_gen; k.pend_gen = g->pend_gen;
    k.jitter = g->jitter_last;
    return k;
}
static constexpr size_t PEND_G_TILE = (size_t)TILE * PEND_GLD;   // the one 128 x 64 tile k_gemm_nt writes for V_p'V_p
static size_t pend_state_layout(const bohip_gp* g, const void* base, layout::PendState* w) {
    return layout::pend_state(base, PEND_PMAX, (size_t)g->d, PEND_G_TILE, w);
}
// V' of the chunk buffer (dVT alone: no U' here), as ensure_grad_scratch sizes it
static int ensure_pend_vt(bohip_gp* g) {
    const size_t n = (size_t)g->kst_rows * g->ld;
    bool grew = false;
    HIPCHK(g->dVT.reserve(n, g->stream, Grow::Exact, &grew));
    if (grew) HIPCHK(hipMemsetAsync(g->dVT, 0, n * 8, g->stream));  // padding columns (>= N) must stay zero
    return 0;
}
// The derived state up to date (the model is fresh, the set is not empty): one posterior pass over Xp that keeps V_p', mu_p from its
// alpha row, V_p'V_p on the MFMA engine, Sigma_p and its factor in one workgroup.  A failed pivot: BOHIP_E_NOTPD, the state stays unset.
static int ensure_pending(bohip_gp* g, layout::PendState* out) {
    const int64_t p = g->pend_p;
    HIPCHK(g->pend_state.reserve(pend_state_layout(g, nullptr, out), g->stream));
    pend_state_layout(g, g->pend_state, out);
    const bohip_gp::PendKey now = pend_key_now(g);
    if (g->pend_key == now) return 0;
    g->pend_key = bohip_gp::PendKey{};
    CHK(ensure_score_scratch(g, p));
    CHK(one_time_kernel_setup());
    const int64_t rows = 2 * TILE;   // one tile of pending columns and a tile of head-room (tile-granular stores; the MFMA product reads 128 rows)
    HIPCHK(g->dPV.reserve((size_t)rows * g->ld, g->stream));
    HIPCHK(hipMemsetAsync(g->dPV, 0, (size_t)rows * g->ld * 8, g->stream));   // padding columns (>= N) and rows (>= p) start at zero
    HIPCHK(hipMemcpyAsync(out->Xp, g->hpend.data(), (size_t)p * g->d * 8, hipMemcpyHostToDevice, g->stream));
    const PassPlan pl = choose_route(g, p, WHOLE_K_ONLY);
    const KernelHyper hp = make_hyper(g);
    const int64_t chunks = chunk_pass(g, pl, out->Xp, hp, ChunkV{g->dPV, g->ld}, false, FuseParams{}, no_finish);   // (one chunk)
    if (chunks < 0) return (int)chunks;
    t_begin(g, "pend_state");
    AcqParams mm{BOHIP_ACQ_MAXMEAN, 0.0, 0.0};
    hipLaunchKernelGGL(k_score, dim3(1), dim3(256), 0, g->stream, g->dq, pl.dm.Rpad, pl.dq_tiles(), g->dmu_raw, p, hp.sigma2, g->beta, mm,
                       out->mu, (double*)nullptr, (double*)nullptr, (Best*)nullptr);
    GemmNTParams gp{};   // (V_p'V_p)[i][j] = sum_n V_p'[i][n] V_p'[j][n]: one 128 x 64 tile, of which the lower p x p corner is read
    gp.A = g->dPV; gp.lda = g->ld; gp.B = g->dPV; gp.ldb = g->ld; gp.C = out->G; gp.ldc = PEND_GLD;
    gp.mt = 1; gp.nt64 = 1; gp.kc = pl.dm.T * (TILE / KC); gp.alpha = 1.0; gp.beta = 0.0;
    CHK(launch_gemm_nt(g, gp));
    dispatch_dt(g->d, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        LAUNCH_FAM(fam_low(hp), (k_pend_state<DT, true>), (k_pend_state<DT, false>), dim3(1), dim3(256), 0, g->stream, out->Xp, (int)p, hp,
                   pend_noise(g), out->G, out->Sigma, out->L, out->info);
    });
    HIPCHK(hipGetLastError());
    t_end(g);
    int info = 0;
    HIPCHK(hipMemcpyAsync(&info, out->info, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (info != 0)
        return fail(BOHIP_E_NOTPD, "pending evaluations: the covariance of the " + std::to_string(p) + " pending points is not positive "
                                   "definite (pivot " + std::to_string(info) + "); no jitter is added here");
    g->pend_key = now;
    return 0;
}

int bohip_gp_pending_set(bohip_gp* g, const double* Xp, int64_t p) {
    if (!g) return fail(BOHIP_E_ARG, "pending_set: null handle");
    if (p < 0 || p > BOHIP_PEND_PMAX)
        return fail(BOHIP_E_ARG, "pending_set: p = " + std::to_string(p) + " does not lie in 0.." + std::to_string(BOHIP_PEND_PMAX) +
                                 " (BOHIP_PEND_PMAX)");
    if (p > 0 && !Xp) return fail(BOHIP_E_ARG, "pending_set: null Xp");
    for (int64_t e = 0; e < p * g->d; ++e)
        if (!std::isfinite(Xp[e])) return fail(BOHIP_E_ARG, "pending_set: coordinate " + std::to_string(e % g->d) + " of pending point " +
                                                                std::to_string(e / g->d) + " is not finite");
    if (p > 0) CHK(refuse_weighted(g, "bohip_gp_pending_set"));
    g->hpend.assign(Xp, Xp + p * g->d);
    g->pend_p = p;
    g->pend_gen++;
    return 0;
}

int bohip_gp_pending_info(bohip_gp* g, int64_t* p_out, double* Xp, double* mu_p, double* cov_p) {
    if (!g) return fail(BOHIP_E_ARG, "pending_info: null handle");
    const int64_t p = g->pend_p;
    if (p_out) *p_out = p;
    if (p == 0) return 0;
    if (Xp) std::memcpy(Xp, g->hpend.data(), (size_t)p * g->d * 8);
    if (!mu_p && !cov_p) return 0;
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(refuse_weighted(g, "bohip_gp_pending_info"));
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_fresh(g));
    layout::PendState st;
    CHK(ensure_pending(g, &st));
    if (mu_p) HIPCHK(hipMemcpyAsync(mu_p, st.mu, (size_t)p * 8, hipMemcpyDeviceToHost, g->stream));
    if (cov_p) HIPCHK(hipMemcpyAsync(cov_p, st.Sigma, (size_t)p * p * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

static int pend_check_acq(const char* who, int acq_id, const double* acq_params, int64_t S, int flags, AcqParams* ap) {
    if (acq_id == BOHIP_ACQ_THOMPSON_DRAW) return fail(BOHIP_E_ARG, std::string(who) + ": a posterior draw has no score under fantasies");
    if (!acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, std::string(who) + ": unknown acq_id");
    CHK(make_acq(acq_id, acq_params, ap));
    if (S < 0 || S > BOHIP_PEND_SMAX)
        return fail(BOHIP_E_ARG, std::string(who) + ": S = " + std::to_string(S) + " does not lie in 0.." + std::to_string(BOHIP_PEND_SMAX) +
                                 " (BOHIP_PEND_SMAX)");
    if (flags & ~BOHIP_PEND_RAISE_TAU) return fail(BOHIP_E_ARG, std::string(who) + ": unknown flags");
    return 0;
}
// the averaging stage and the record: k_pend_score over R candidates, k_argmax_final when a record is wanted
static int pend_blocks(int64_t R) { return (int)((R + PEND_SCORE_THREADS - 1) / PEND_SCORE_THREADS); }
static int pend_score_stage(bohip_gp* g, PendScore ps, Best* blk, Best* d_best) {
    const int nb = pend_blocks(ps.R);
    ps.block_best = d_best ? blk : nullptr;
    t_begin(g, "pend_score");
    hipLaunchKernelGGL(k_pend_score, dim3(nb), dim3(PEND_SCORE_THREADS), 0, g->stream, ps);
    if (d_best) hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, blk, nb, d_best, (long long)0);
    HIPCHK(hipGetLastError());
    t_end(g);
    return 0;
}

int bohip_gp_score_pending(bohip_gp* g, int acq_id, const double* acq_params, const double* Xs, int64_t R, int64_t S, uint64_t seed,
                           int flags, double* score, double* mu, double* var, bohip_best* best) {
    if (!g || R < 0 || (R > 0 && !Xs)) return fail(BOHIP_E_ARG, "score_pending: bad arguments");
    AcqParams ap;
    CHK(pend_check_acq("score_pending", acq_id, acq_params, S, flags, &ap));
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    const int64_t p = g->pend_p;
    if (p == 0) {   // no pending point: the call IS bohip_gp_score (and bohip_gp_predict for the moments)
        CHK(bohip_gp_score(g, acq_id, acq_params, Xs, R, score, best));
        if (R > 0 && (mu || var)) {
            std::vector<double> tmp((size_t)R);
            CHK(bohip_gp_predict(g, Xs, R, mu ? mu : tmp.data(), var ? var : tmp.data()));
        }
        return 0;
    }
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    CHK(refuse_weighted(g, "bohip_gp_score_pending"));
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_fresh(g));
    layout::PendState st;
    CHK(ensure_pending(g, &st));
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    CHK(one_time_kernel_setup());
    const PassPlan pl = choose_route(g, R, WHOLE_K_ONLY);   // the route that stores V'
    CHK(ensure_pend_vt(g));
    const int64_t S1 = std::max<int64_t>(S, 1), crows = round_up(std::min(R, pl.chunk), TILE);
    // V'V_p is 128 x 64 tiles over a contraction of Npad: a chunk of 4096 candidates is 32 workgroups.  The contraction is cut into
    // slices of kz 16-deep steps -- a function of the row tiles alone, so a candidate's value does not depend on the batch it is
    // scored in -- whose planes k_pend_cross adds in ascending order (measured: profiles/pending_ab.txt).
    const int kc_all = pl.dm.T * (TILE / KC), kz = std::max(8, (kc_all + 7) / 8), nsl = (kc_all + kz - 1) / kz;
    const int64_t plane = crows * PEND_GLD;
    const int nb = pend_blocks(R);
    PendCallWs w;
    auto lay = [&](const void* base) { return layout::pend_call(base, (size_t)(nsl * plane), (size_t)R, (size_t)p, (size_t)S1, 0, (size_t)nb, &w); };
    HIPCHK(g->pend_call.reserve(lay(nullptr), g->stream));
    lay(g->pend_call);
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    const bool tau_acq = pend_tau_acq(acq_id), raise = tau_acq && (flags & BOHIP_PEND_RAISE_TAU);
    t_begin(g, "pend_tables");
    hipLaunchKernelGGL(k_pend_tables, dim3((unsigned)((S1 + 63) / 64)), dim3(64), 0, g->stream, st.mu, st.L, (int)p, (int)S1, S == 0 ? 1 : 0,
                       (unsigned long long)seed, ap.p0, raise ? 1 : 0, w.Z, w.tau);
    HIPCHK(hipGetLastError());
    t_end(g);
    const KernelHyper hp = make_hyper(g);
    auto cross = [&](int64_t r0, int64_t r1) {   // per K*' chunk: C = V'V_p on the MFMA engine, then c, b = L_p^-1 c per candidate
        t_begin(g, "pend_cross");
        GemmNTParams gp{};
        gp.A = g->dVT; gp.lda = g->ld; gp.B = g->dPV; gp.ldb = g->ld; gp.C = w.C; gp.ldc = PEND_GLD;
        gp.mt = (int)((r1 - r0 + TILE - 1) / TILE); gp.nt64 = 1; gp.kc = kz; gp.alpha = 1.0; gp.beta = 0.0;
        gp.kz = kz; gp.ktot = kc_all; gp.zA = (int64_t)kz * KC; gp.zB = (int64_t)kz * KC; gp.zC = plane;
        CHK(launch_gemm_nt(g, gp, nsl));
        const unsigned blocks = (unsigned)((r1 - r0 + PEND_CROSS_THREADS - 1) / PEND_CROSS_THREADS);
        dispatch_dt(g->d, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            LAUNCH_FAM(fam_low(hp), (k_pend_cross<DT, true>), (k_pend_cross<DT, false>), dim3(blocks), dim3(PEND_CROSS_THREADS), 0, g->stream,
                       g->dXs.get(), r0, r1, hp, st.Xp, (int)p, st.L, w.C, nsl, plane, w.B);
        });
        HIPCHK(hipGetLastError());
        t_end(g);
        return 0;
    };
    const int64_t chunks = chunk_pass(g, pl, g->dXs, hp, ChunkV{g->dVT, 0}, false, FuseParams{}, cross);
    if (chunks < 0) return (int)chunks;
    g->score_launches = chunks;
    AcqParams mm{BOHIP_ACQ_MAXMEAN, 0.0, 0.0};
    hipLaunchKernelGGL(k_score, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, g->stream, g->dq, pl.dm.Rpad, pl.dq_tiles(), g->dmu_raw, R,
                       hp.sigma2, g->beta, mm, g->dmu.get(), g->dvar.get(), (double*)nullptr, (Best*)nullptr);
    PendScore ps{};
    ps.mu = g->dmu; ps.var = g->dvar; ps.B = w.B; ps.Z = w.Z; ps.tau = w.tau; ps.R = R; ps.p = (int)p; ps.S1 = (int)S1; ps.sub_bb = 1;
    ps.tau_acq = tau_acq ? 1 : 0; ps.ap = ap; ps.score_out = score ? g->dscore.get() : nullptr; ps.var_out = g->dvar;
    CHK(pend_score_stage(g, ps, w.blk, best ? w.best : nullptr));
    if (score) HIPCHK(hipMemcpyAsync(score, g->dscore, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (mu) HIPCHK(hipMemcpyAsync(mu, g->dmu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (var) HIPCHK(hipMemcpyAsync(var, g->dvar, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, w.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

int bohip_pend_values(bohip_gp* g, int acq_id, const double* acq_params, int64_t R, int64_t p, int64_t S, const double* mu,
                      const double* var, const double* B, const double* Z, const double* tau_s, double* score, bohip_best* best) {
    if (!g) return fail(BOHIP_E_ARG, "pend_values: null handle");
    AcqParams ap;
    CHK(pend_check_acq("pend_values", acq_id, acq_params, S, 0, &ap));
    if (S < 1) return fail(BOHIP_E_ARG, "pend_values: S = 0; the believer is one fantasy with z = 0 (1 <= S <= BOHIP_PEND_SMAX)");
    if (p < 1 || p > BOHIP_PEND_PMAX)
        return fail(BOHIP_E_ARG, "pend_values: p = " + std::to_string(p) + " does not lie in 1.." + std::to_string(BOHIP_PEND_PMAX) +
                                 " (BOHIP_PEND_PMAX)");
    if (R < 0 || !Z || (R > 0 && (!mu || !var || !B || !score))) return fail(BOHIP_E_ARG, "pend_values: bad arguments");
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    const int nb = pend_blocks(R);
    PendCallWs w;
    auto lay = [&](const void* base) { return layout::pend_call(base, 0, (size_t)R, (size_t)p, (size_t)S, (size_t)R, (size_t)nb, &w); };
    HIPCHK(g->pend_call.reserve(lay(nullptr), g->stream));
    lay(g->pend_call);
    HIPCHK(hipMemcpyAsync(w.mu, mu, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(w.var, var, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(w.B, B, (size_t)R * p * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(w.Z, Z, (size_t)S * p * 8, hipMemcpyHostToDevice, g->stream));
    if (tau_s) HIPCHK(hipMemcpyAsync(w.tau, tau_s, (size_t)S * 8, hipMemcpyHostToDevice, g->stream));
    PendScore ps{};
    ps.mu = w.mu; ps.var = w.var; ps.B = w.B; ps.Z = w.Z; ps.tau = tau_s ? w.tau : nullptr; ps.R = R; ps.p = (int)p; ps.S1 = (int)S;
    ps.sub_bb = 0; ps.tau_acq = pend_tau_acq(acq_id) ? 1 : 0; ps.ap = ap; ps.score_out = w.score; ps.var_out = nullptr;
    CHK(pend_score_stage(g, ps, w.blk, best ? w.best : nullptr));
    HIPCHK(hipMemcpyAsync(score, w.score, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, w.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    return 0;
}

// ---- noisy expected improvement (include/bohip_nei.h; kernels_nei.hip) -----------------------------------------------
// An extension.  The noise-free model of the same sites is a bohip_gp of its own, owned by the caller's handle: the refit plan, the
// incremental append and the posterior pass (small, split-K, whole-K) are the model's, not copies of them.  It runs on the owner's
// stream, is made at the first call of this header and is kept in step lazily; the fantasies live in one block on the owner.
using NeiCallWs = layout::NeiCall<Best>;
static int nei_kernel_setup() {
    static bool done[64] = {false};
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    return once_per_device(done, dev, [] {
        HIPCHK(hipFuncSetAttribute((const void*)k_nei_means, hipFuncAttributeMaxDynamicSharedMemorySize, glds3_lds_bytes<4>()));
        return 0;
    });
}
static int nei_check(const char* who, int acq_id, int64_t S, double jitter_rel, bool want_acq) {
    if (want_acq && !pend_tau_acq(acq_id))
        return fail(BOHIP_E_ARG, std::string(who) + ": noisy expected improvement averages an acquisition with an incumbent (EI, PI, LogEI)");
    if (S < 0 || S > BOHIP_NEI_SMAX)
        return fail(BOHIP_E_ARG, std::string(who) + ": S = " + std::to_string(S) + " does not lie in 0.." + std::to_string(BOHIP_NEI_SMAX) +
                                 " (BOHIP_NEI_SMAX)");
    if (!(jitter_rel > 0.0) || !std::isfinite(jitter_rel)) return fail(BOHIP_E_ARG, std::string(who) + ": jitter_rel must be positive and finite");
    return 0;
}
// the companion's stage times behind the owner's (the owner's were collected)
static void nei_merge_timing(bohip_gp* g) {
    bohip_gp* c = g->nei;
    if (!g->timing || g->timing_accumulate || !c) return;
    g->tnames.insert(g->tnames.end(), c->tnames.begin(), c->tnames.end());   // (what an append of the companion collected itself)
    g->tms.insert(g->tms.end(), c->tms.begin(), c->tms.end());
    t_collect(c);
    g->tnames.insert(g->tnames.end(), c->tnames.begin(), c->tnames.end());
    g->tms.insert(g->tms.end(), c->tms.begin(), c->tms.end());
    c->tnames.clear();
    c->tms.clear();
}
// The companion up to date with the owner's X and kernel parameters at delta = jitter_rel sigma_f^2 (the owner is fresh).  New rows go
// through append_rows: up to 32 of them onto a fresh factor are ONE incremental append, anything else a refit.  A failed pivot tries
// delta x 10, up to three times.
static int nei_companion_sync(bohip_gp* g, double jitter_rel) {
    if (!g->nei) {
        bohip_gp* c = nullptr;
        CHK(bohip_gp_create(g->d, std::max<int64_t>(g->cap, 1), g->kern, g->device, &c));
        c->jitter_rel = 0.0; c->jitter_tries = 0;   // (the steps here are the header's, not BOHIP_JITTER's)
        g->nei = c;
        g->nei_jrel = -1.0;
        g->nei_key = bohip_gp::NeiKey{};
    }
    bohip_gp* c = g->nei;
    c->stream = g->stream;
    c->batch_hint = g->batch_hint;
    c->timing = g->timing; c->timing_dominant_only = g->timing_dominant_only; c->timing_accumulate = false;
    t_reset(c);
    bool same = jitter_rel == g->nei_jrel && c->logsig == g->logsig;
    for (int k = 0; k < g->d; ++k) same = same && c->loglen[k] == g->loglen[k];
    const double eps = std::numeric_limits<double>::epsilon();
    int rc = 0;
    for (int step = same ? g->nei_steps : 0; step <= 3; ++step) {
        if (!same || step != g->nei_steps) {
            const double delta = jitter_rel * std::exp(2.0 * g->logsig) * std::pow(10.0, step);
            for (int k = 0; k < DMAX; ++k) c->loglen[k] = g->loglen[k];
            c->logsig = g->logsig;
            c->lognoise = delta > 2.0 * eps ? 0.5 * std::log(delta - eps) : -400.0;
            c->stale = true;
            g->nei_jrel = jitter_rel;
            g->nei_steps = step;
            g->nei_delta = std::exp(2.0 * c->lognoise) + eps;
        }
        c->beta = g->beta;
        if (c->n < g->n) {
            const int64_t n0 = c->n;
            rc = append_rows(c, g->hX.data() + n0 * g->d, g->hy.data() + n0, nullptr, nullptr, g->n - n0);
        } else {
            rc = ensure_fresh(c);
        }
        if (rc != BOHIP_E_NOTPD) return rc;
        same = false;
    }
    return rc;
}
static bohip_gp::NeiKey nei_key_now(const bohip_gp* g, int64_t S, uint64_t seed) {
    bohip_gp::NeiKey k;
    k.n = g->n; k.ld = g->ld; k.refits = g->refits; k.appends = g->appends; k.c_refits = g->nei->refits; k.c_appends = g->nei->appends;
    k.S = S; k.hyper_gen = g->hyper_gen; k.data_version = g->data_version; k.seed = seed; k.jitter = g->jitter_last; k.delta = g->nei_delta;
    return k;
}
// out[s][i] = sum_j in[s][j] B[i][j] for the rows of the fantasy matrices and the Npad rows of a resident factor B (both K-major).
// The factors are triangular by TILES only where their readers are (the other tiles of dW, dWT are never read by the model's passes
// and hold whatever the factorisation parked there), so the products take the same limits: a lower factor (L, W: j <= i) is the A
// operand with khi_from_m and the result leaves transposed; an upper one (W': j >= i) is the B operand with klo_from_n.
static int nei_product(bohip_gp* g, const double* in, const double* B, int64_t ldb, bool lower, double* out, int64_t rows, int64_t ld,
                       int64_t Npad) {
    GemmNTParams p{};
    p.kc = (int)(Npad / KC); p.alpha = 1.0; p.beta = 0.0;
    if (lower) {
        p.A = B; p.lda = ldb; p.B = in; p.ldb = ld; p.C = nullptr; p.CT = out; p.ldct = ld;
        p.mt = (int)(Npad / TILE); p.nt64 = (int)(rows / CTILE); p.khi_from_m = 1;
    } else {
        p.A = in; p.lda = ld; p.B = B; p.ldb = ldb; p.C = out; p.ldc = ld;
        p.mt = (int)(rows / TILE); p.nt64 = (int)(Npad / CTILE); p.klo_from_n = 1;
    }
    return launch_gemm_nt(g, p);
}
// The fantasies and alpha_s up to date (the owner and the companion are fresh): five N x N x S products on the MFMA engine between
// the element-wise stages of kernels_nei.hip.
static int ensure_nei_fantasies(bohip_gp* g, int64_t S, uint64_t seed, layout::NeiState* st) {
    bohip_gp* c = g->nei;
    const int64_t S1 = std::max<int64_t>(S, 1), rows = round_up(S1, TILE), N = g->n, Npad = (int64_t)row_tiles(g) * TILE;
    const bohip_gp::NeiKey now = nei_key_now(g, S, seed);
    if (g->nei_key == now && g->nei_ws) {
        layout::nei_state(g->nei_ws, (size_t)rows, (size_t)g->nei_ld, (size_t)S1, st);
        return 0;
    }
    g->nei_key = bohip_gp::NeiKey{};
    const int64_t ld = g->ld;
    const size_t bytes = layout::nei_state(nullptr, (size_t)rows, (size_t)ld, (size_t)S1, st);
    HIPCHK(g->nei_ws.reserve(bytes + 128, g->stream));
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(g->nei_ws.get()) + 127) / 128 * 128);   // (hipMalloc aligns to more; the layout wants 128)
    layout::nei_state(base, (size_t)rows, (size_t)ld, (size_t)S1, st);
    g->nei_ld = ld;
    CHK(one_time_kernel_setup());
    t_begin(g, "nei_fantasies");
    HIPCHK(hipMemsetAsync(base, 0, bytes, g->stream));   // rows >= S1 and columns >= N start at zero (and stay: the stages write i < N)
    const dim3 grid_n((unsigned)((N + 255) / 256), (unsigned)S1), grid_pad((unsigned)((Npad + 255) / 256), (unsigned)S1);
    const dim3 grid_mask((unsigned)((Npad - N + 255) / 256), (unsigned)rows);
    const double nu = pend_noise(g);
    const double* invr = g->weighted ? g->dinvr.get() : nullptr;
    const int zero = S == 0 ? 1 : 0;
    double *Z = st->w0, *G = st->w1, *RH = st->w2, *T = st->w3, *Q = st->w0, *P = st->w1, *T2 = st->w3;
    if (S > 0) {
        hipLaunchKernelGGL(k_nei_normals, grid_n, dim3(256), 0, g->stream, Z, ld, N, (int)S, (unsigned long long)seed);
        CHK(nei_product(g, Z, c->dL, c->ld, true, G, rows, ld, Npad));                          // g_s = L_d z_s
    }
    hipLaunchKernelGGL(k_nei_resid, grid_n, dim3(256), 0, g->stream, g->dy.get(), g->beta, G, ld, N, zero, (unsigned long long)seed, nu, invr, RH);
    CHK(nei_product(g, RH, g->dW, g->ld, true, T, rows, ld, Npad));                             // W r_s
    hipLaunchKernelGGL(k_nei_mask, grid_mask, dim3(256), 0, g->stream, T, ld, N, Npad);   // (row N of W holds alpha)
    CHK(nei_product(g, T, g->dWT, g->ld, false, Q, rows, ld, Npad));                             // A^-1 r_s = W'(W r_s)
    hipLaunchKernelGGL(k_nei_fant, grid_n, dim3(256), 0, g->stream, G, Q, ld, N, g->beta, nu, invr, RH, st->F);
    hipLaunchKernelGGL(k_nei_tau, dim3((unsigned)S1), dim3(256), 0, g->stream, st->F, ld, N, st->tau);
    CHK(nei_product(g, RH, c->dW, c->ld, true, P, rows, ld, Npad));                             // W_d h_s
    hipLaunchKernelGGL(k_nei_t2, grid_pad, dim3(256), 0, g->stream, P, ld, N, Npad, zero, (unsigned long long)seed, T2);
    CHK(nei_product(g, T2, c->dWT, c->ld, false, st->alpha, rows, ld, Npad));                    // alpha_s = W_d'(z_s + W_d h_s)
    hipLaunchKernelGGL(k_nei_mask, grid_mask, dim3(256), 0, g->stream, st->alpha, ld, N, Npad);
    HIPCHK(hipGetLastError());
    t_end(g);
    g->nei_key = now;
    g->nei_rebuilds++;
    return 0;
}
// everything a call of the header needs, in order; *st: the fantasies
static int nei_ready(bohip_gp* g, double jitter_rel, int64_t S, uint64_t seed, layout::NeiState* st) {
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    CHK(ensure_fresh(g));
    CHK(nei_companion_sync(g, jitter_rel));
    return ensure_nei_fantasies(g, S, seed, st);
}

int bohip_gp_nei_prepare(bohip_gp* g, double jitter_rel, int64_t S, uint64_t seed) {
    return bohip_gp_nei_fantasies(g, jitter_rel, S, seed, nullptr, nullptr);
}

int bohip_gp_nei_fantasies(bohip_gp* g, double jitter_rel, int64_t S, uint64_t seed, double* F, double* tau) {
    if (!g) return fail(BOHIP_E_ARG, "nei_fantasies: null handle");
    CHK(nei_check("nei_fantasies", 0, S, jitter_rel, false));
    layout::NeiState st;
    CHK(nei_ready(g, jitter_rel, S, seed, &st));
    const int64_t S1 = std::max<int64_t>(S, 1);
    if (F) HIPCHK(hipMemcpy2DAsync(F, (size_t)g->n * 8, st.F, (size_t)g->nei_ld * 8, (size_t)g->n * 8, (size_t)S1, hipMemcpyDeviceToHost, g->stream));
    if (tau) HIPCHK(hipMemcpyAsync(tau, st.tau, (size_t)S1 * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    nei_merge_timing(g);
    return 0;
}

// the averaging stage of the candidates [r0, r1) whose means sit in w.MT (column 0 = r0), and -- last -- the record
static int nei_reduce_stage(bohip_gp* g, const NeiCallWs& w, const double* var, const double* tau, int64_t ldm, int nsl, int64_t plane,
                            int64_t r0, int64_t r1, int64_t S1, int acq_id, bool want_best) {
    NeiReduce nr{};
    nr.MT = w.MT; nr.var = var; nr.tau = tau; nr.ldm = ldm; nr.nsl = nsl; nr.plane = plane; nr.r0 = r0; nr.r1 = r1; nr.S1 = (int)S1;
    nr.ap = AcqParams{acq_id, 0.0, 0.0};
    nr.score_out = w.score; nr.mu_out = w.mu; nr.block_best = want_best ? w.blk : nullptr;
    t_begin(g, "nei_reduce");
    hipLaunchKernelGGL(k_nei_reduce, dim3((unsigned)((r1 - r0 + NEI_RED_THREADS - 1) / NEI_RED_THREADS)), dim3(NEI_RED_THREADS), 0, g->stream, nr);
    HIPCHK(hipGetLastError());
    t_end(g);
    return 0;
}
static int nei_blocks(int64_t R) { return (int)((R + NEI_RED_THREADS - 1) / NEI_RED_THREADS); }
static int nei_record_stage(bohip_gp* g, const NeiCallWs& w, int64_t R) {
    hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, w.blk, nei_blocks(R), w.best, (long long)0);
    HIPCHK(hipGetLastError());
    return 0;
}

int bohip_gp_score_nei(bohip_gp* g, int acq_id, const double* acq_params, const double* Xs, int64_t R, int64_t S, uint64_t seed,
                       double jitter_rel, double* score, double* mu, double* var, bohip_best* best) {
    (void)acq_params;   // (tau is the fantasy's own)
    if (!g || R < 0 || (R > 0 && !Xs)) return fail(BOHIP_E_ARG, "score_nei: bad arguments");
    CHK(nei_check("score_nei", acq_id, S, jitter_rel, true));
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    layout::NeiState st;
    CHK(nei_ready(g, jitter_rel, S, seed, &st));
    bohip_gp* c = g->nei;
    CHK(ensure_xs(c, R));
    CHK(ensure_score_scratch(c, R));
    CHK(one_time_kernel_setup());
    CHK(nei_kernel_setup());
    const PassPlan pl = choose_route(c, R, RouteWants{true, true, Prune::No});   // the companion's ordinary pass: the existing plan
    const int64_t S1 = std::max<int64_t>(S, 1), Sp = round_up(S1, CTILE);
    const int64_t crows = round_up(pl.route == Route::WholeK ? std::min(R, pl.chunk) : R, TILE);
    // The means' contraction is cut into slices of kz 16-deep steps -- a function of the row tiles alone, so a candidate's value does
    // not depend on the batch it is scored in -- whose planes k_nei_reduce adds in ascending order (32 workgroups over the whole
    // contraction at R = 4096, S = 64 took 0.21 ms: profiles/nei_ab.txt).  The planes of one launch stay below 256 MB: a chunk is
    // taken mrows candidates at a time (which changes no bit).
    const int kc_all = (int)(pl.dm.Npad / KC), kz = std::max(8, (kc_all + 7) / 8), nsl = (kc_all + kz - 1) / kz;
    const int64_t mrows = std::min(crows, std::max<int64_t>(TILE, ((int64_t)256 << 20) / (8 * nsl * Sp) / TILE * TILE));
    const int64_t plane = Sp * mrows;
    NeiCallWs w;
    auto lay = [&](const void* base) { return layout::nei_call(base, (size_t)(nsl * plane), (size_t)R, 0, 0, (size_t)nei_blocks(R), &w); };
    HIPCHK(g->nei_call.reserve(lay(nullptr) + 128, g->stream));
    lay(reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(g->nei_call.get()) + 127) / 128 * 128));
    HIPCHK(hipMemcpyAsync(c->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    const KernelHyper hp = make_hyper(c);
    const AcqParams mm{BOHIP_ACQ_MAXMEAN, 0.0, 0.0};
    // per K*' chunk (rows 0 .. r1 - r0 of the companion's chunk buffer, the one its variance contraction read): the means of every
    // fantasy on the MFMA engine, then the average over the fantasies
    auto finish = [&](int64_t r0, int64_t r1) {
        for (int64_t b0 = r0; b0 < r1; b0 += mrows) {
            const int64_t b1 = std::min(r1, b0 + mrows);
            NeiMeans nm{};
            nm.A = c->dKsT + (b0 - r0) * c->ld; nm.lda = c->ld; nm.B = st.alpha; nm.ldb = g->nei_ld; nm.MT = w.MT; nm.ldm = mrows; nm.plane = plane;
            nm.mt = (int)((b1 - b0 + TILE - 1) / TILE); nm.nt = (int)(Sp / CTILE); nm.kc = kc_all; nm.kz = kz; nm.beta = g->beta;
            t_begin(c, "nei_means");
            hipLaunchKernelGGL(k_nei_means, dim3((unsigned)(nm.mt * nm.nt), (unsigned)nsl), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), g->stream, nm);
            HIPCHK(hipGetLastError());
            t_end(c);
            CHK(nei_reduce_stage(c, w, c->dvar, st.tau, mrows, nsl, plane, b0, b1, S1, acq_id, best != nullptr));
        }
        return 0;
    };
    if (pl.route == Route::Small) {
        CHK(small_pass_mfma(c, c->dXs, R, mm, c->dmu, c->dvar, nullptr, nullptr, 0, nullptr));
        t_begin(c, "kstar");
        CHK(launch_kstar_any(c, c->dXs, 0, R, pl.dm.Npad, hp));   // (the small pass builds its K* in registers: the means need it in memory)
        t_end(c);
        CHK(finish(0, R));
    } else if (pl.route == Route::Split) {
        CHK(split_posterior(c, c->dXs, pl, false));
        hipLaunchKernelGGL(k_score, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, g->stream, c->dq.get(), pl.dm.Rpad, pl.dq_tiles(),
                           c->dmu_raw.get(), R, hp.sigma2, c->beta, mm, c->dmu.get(), c->dvar.get(), (double*)nullptr, (Best*)nullptr);
        HIPCHK(hipGetLastError());
        CHK(finish(0, R));
    } else {
        auto chunk_finish = [&](int64_t r0, int64_t r1) {
            hipLaunchKernelGGL(k_score, dim3((unsigned)((r1 - r0 + 255) / 256)), dim3(256), 0, g->stream, c->dq.get() + r0, pl.dm.Rpad,
                               pl.dq_tiles(), c->dmu_raw.get() + r0, r1 - r0, hp.sigma2, c->beta, mm, c->dmu.get() + r0, c->dvar.get() + r0,
                               (double*)nullptr, (Best*)nullptr);
            HIPCHK(hipGetLastError());
            return finish(r0, r1);
        };
        const int64_t chunks = chunk_pass(c, pl, c->dXs, hp, ChunkV{}, false, FuseParams{}, chunk_finish);
        if (chunks < 0) return (int)chunks;
        c->score_launches = chunks;
    }
    if (best) CHK(nei_record_stage(g, w, R));
    if (score) HIPCHK(hipMemcpyAsync(score, w.score, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (mu) HIPCHK(hipMemcpyAsync(mu, w.mu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (var) HIPCHK(hipMemcpyAsync(var, c->dvar, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, w.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    t_collect(g);
    nei_merge_timing(g);
    return 0;
}

int bohip_nei_values(bohip_gp* g, int acq_id, int64_t R, int64_t S, const double* mu_s, const double* var, const double* tau_s,
                     double* score, double* mu_mean, bohip_best* best) {
    if (!g) return fail(BOHIP_E_ARG, "nei_values: null handle");
    CHK(nei_check("nei_values", acq_id, S, 1.0, true));
    if (S < 1) return fail(BOHIP_E_ARG, "nei_values: S = 0; the plug-in form is one fantasy (1 <= S <= BOHIP_NEI_SMAX)");
    if (R < 0 || !tau_s || (R > 0 && (!mu_s || !var || !score))) return fail(BOHIP_E_ARG, "nei_values: bad arguments");
    if (R == 0) {
        if (best) { best->val = -INFINITY; best->idx = -1; }
        return 0;
    }
    HIPCHK(hipSetDevice(g->device));
    t_reset(g);
    NeiCallWs w;
    auto lay = [&](const void* base) { return layout::nei_call(base, (size_t)(S * R), (size_t)R, (size_t)R, (size_t)S, (size_t)nei_blocks(R), &w); };
    HIPCHK(g->nei_call.reserve(lay(nullptr) + 128, g->stream));
    lay(reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(g->nei_call.get()) + 127) / 128 * 128));
    std::vector<double> mt((size_t)(S * R));   // fantasy-major, as k_nei_means leaves the means
    for (int64_t r = 0; r < R; ++r)
        for (int64_t s = 0; s < S; ++s) mt[(size_t)(s * R + r)] = mu_s[r * S + s];
    HIPCHK(hipMemcpyAsync(w.MT, mt.data(), (size_t)(S * R) * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(w.var, var, (size_t)R * 8, hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(w.tau, tau_s, (size_t)S * 8, hipMemcpyHostToDevice, g->stream));
    CHK(nei_reduce_stage(g, w, w.var, w.tau, R, 1, 0, 0, R, S, acq_id, best != nullptr));
    if (best) CHK(nei_record_stage(g, w, R));
    HIPCHK(hipMemcpyAsync(score, w.score, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (mu_mean) HIPCHK(hipMemcpyAsync(mu_mean, w.mu, (size_t)R * 8, hipMemcpyDeviceToHost, g->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, w.best, sizeof(Best), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));   // (mt lives until here)
    t_collect(g);
    return 0;
}

int bohip_gp_nei_info(const bohip_gp* g, int what, double* value) {
    if (!g || !value) return fail(BOHIP_E_ARG, "null argument");
    const bohip_gp* c = g->nei;
    switch (what) {
        case BOHIP_NEI_INFO_REFITS: *value = c ? (double)c->refits : 0.0; return 0;
        case BOHIP_NEI_INFO_APPENDS: *value = c ? (double)c->appends : 0.0; return 0;
        case BOHIP_NEI_INFO_REBUILDS: *value = (double)g->nei_rebuilds; return 0;
        case BOHIP_NEI_INFO_JITTER_STEPS: *value = c ? (double)g->nei_steps : 0.0; return 0;
        case BOHIP_NEI_INFO_DELTA: *value = c ? g->nei_delta : 0.0; return 0;
        case BOHIP_NEI_INFO_BYTES: {
            size_t b = g->nei_ws.capacity() + g->nei_call.capacity();
            if (c) b += 8 * (c->dL.capacity() + c->dW.capacity() + c->dWT.capacity() + c->dS.capacity() + c->dApp.capacity() + c->dKsT.capacity());
            *value = (double)b;
            return 0;
        }
        default: return fail(BOHIP_E_ARG, "unknown info id");
    }
}

int bohip_gp_nei_release(bohip_gp* g) {
    if (!g) return fail(BOHIP_E_ARG, "null handle");
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipStreamSynchronize(g->stream));
    delete g->nei;
    g->nei = nullptr;
    g->nei_ws.release();
    g->nei_call.release();
    g->nei_key = bohip_gp::NeiKey{};
    g->nei_jrel = -1.0; g->nei_delta = 0.0; g->nei_steps = 0; g->nei_rebuilds = 0;
    return 0;
}

}  // extern "C"
#include "multigpu.hip"
extern "C" {
// tools only: the resident W = L^-1 (which = 0) or W' (which = 1), n x n row-major
int bohip_debug_read_w(bohip_gp* g, int which, double* out) {
    if (!g || !out) return BOHIP_E_ARG;
    hipSetDevice(g->device);
    hipStreamSynchronize(g->stream);
    const double* src = which ? g->dWT : g->dW;
    return hipMemcpy2D(out, (size_t)g->n * 8, src, (size_t)g->ld * 8, (size_t)g->n * 8, (size_t)g->n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : BOHIP_E_HIP;
}
// test hook (tests/test_exec_tasks.py): the executor's task records for T row tiles with the three matrices at the fake
// addresses base_L/S/W (bytes) and flag word 0 at index 0 -- the CPU test replays them against a model of the chain.
// out: n x 16 uint64 words (the 128-byte records); returns the number of records, qbeg[0..EX_NQ] (EX_NQ + 1 = 7 ints) the queue boundaries,
// layout[0..9] the word offsets of panel, solved, crit, rest, col, farall, fol, colall, colr, xp inside the flag area;
// layout[10] the number of solve-follower workgroups of the chain kernel (CH_NSF).
int64_t bohip_debug_exec_tasks(int T, int64_t ld, uint64_t base_L, uint64_t base_S, uint64_t base_W, uint64_t base_WT, int inv_g, uint64_t* out,
                               int64_t cap, int* qbeg, int64_t* layout) {
    std::vector<bohip::ExTask> all;
    int qb[bohip::EX_NQ + 1];
    unsigned* fb = reinterpret_cast<unsigned*>(uintptr_t(1) << 40);
    // the follower count the records are built for = the one reported in layout[10]: the env knob is read HERE (the library's
    // one-time setup may not have run yet), and the process-wide setting is left alone
    const int nsf = g_chol_nsf;
    int grp_min = g_chol_inv_grp_min;
    if (const char* e = getenv("BOHIP_CHOL_INV_GRP_MIN")) grp_min = std::max(0, atoi(e));
    exec_task_list(reinterpret_cast<double*>(base_L), reinterpret_cast<double*>(base_S), reinterpret_cast<double*>(base_W),
                   reinterpret_cast<double*>(base_WT), fb, ld, T, nsf, inv_g, all, qb, grp_min);
    for (int i = 0; i <= bohip::EX_NQ; ++i) qbeg[i] = qb[i];
    const bohip::CholFlags fl = chol_flags_layout_at(fb, nullptr, T);
    const unsigned* ptrs[10] = {fl.panel, fl.solved, fl.crit, fl.rest, fl.col, fl.farall, fl.fol, fl.colall, fl.colr, fl.xp};
    for (int i = 0; i < 10; ++i) layout[i] = ptrs[i] - fb;
    layout[10] = nsf;
    layout[11] = (int64_t)chol_inv_word(T);
    layout[12] = (int64_t)chol_xp3_word(T);
    layout[13] = exec_bulk_stride_ok(all, qb, 4) ? 2 : 1;   // bulk tiles per claim the library may use at this T
    if ((int64_t)all.size() <= cap && out) std::memcpy(out, all.data(), all.size() * sizeof(bohip::ExTask));
    return (int64_t)all.size();
}
// tools only (tools/trace_trigemm.py): the row pieces k_trigemm_sq runs for T row tiles with the alpha row at alpha_row, in issue order
// (piece = rt | mode << 16, see kernels_score.hip); returns their number
// tests: the bytes the process's buffers hold (devbuf.h), kind 0 device memory, 1 pinned host memory
int bohip_debug_live_bytes(int kind, int64_t* out) {
    if ((kind != devbuf::DEVICE && kind != devbuf::PINNED) || !out) return fail(BOHIP_E_ARG, "bad arguments");
    *out = devbuf::g_live_bytes[kind].load();
    return 0;
}
int bohip_debug_trigemm_pieces(int T, int64_t alpha_row, int* out, int cap) {
    one_time_kernel_setup();
    std::vector<int> ps;
    trigemm_pieces(T, alpha_row, ps);
    for (int i = 0; i < (int)ps.size() && i < cap; ++i) out[i] = ps[i];
    return (int)ps.size();
}
// tools and bench.py: switch the executor's inverse queues at run time (returns the previous chunk size; 0 = off: the factorisation
// alone can then be timed against its own flop count)
// tests only (tests/test_prune_gpu.py): the pruned pass's upper bounds of the scores of R host candidates (layout of bohip_gp_score);
// BOHIP_E_UNSUPPORTED where a value-only call of this size would not prune
int bohip_debug_prune_bounds(bohip_gp* g, int acq_id, const double* acq_params, const double* Xs, int64_t R, double* ub) {
    if (!g || R <= 0 || !Xs || !ub || !acq_id_scores(acq_id)) return fail(BOHIP_E_ARG, "bad arguments");
    HIPCHK(hipSetDevice(g->device));
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(ensure_fresh(g));
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    static const double no_params[2] = {0.0, 0.0};   // (a null acq_params is taken as zeros here)
    AcqParams ap;
    CHK(make_acq(acq_id, acq_params ? acq_params : no_params, &ap));
    const PassPlan pl = choose_route(g, R, RouteWants{true, true, Prune::Probe});
    if (pl.route != Route::Pruned) return fail(BOHIP_E_UNSUPPORTED, "no pruning at this size");
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    return pruned_pass(g, g->dXs, pl, ap, nullptr, 0, ub);
}
// tests only (tests/test_prune_rows_gpu.py): the partial sums q[2T][R] and mu_raw[R] of R host candidates from the full pass's
// k_trigemm_sq (path 0) or from k_trigemm_rows over every row tile, the candidates listed in reverse order (path 1; path 2: the
// same with ONE column group in the grid, every further group from the kernel's loop).  Path 3: the phase-A launch exactly as
// pruned_pass enqueues it (phase_a_jobs, launch_phase_a, m from prune_tiles): q rows 2 t + h for t < m, every other row and mu zero;
// BOHIP_E_UNSUPPORTED where no T-tile model prunes.
int bohip_debug_trigemm_partials(bohip_gp* g, const double* Xs, int64_t R, int path, double* q_out, double* mu_out) {
    if (!g || R <= 0 || !Xs || !q_out || !mu_out || path < 0 || path > 3) return fail(BOHIP_E_ARG, "bad arguments");
    HIPCHK(hipSetDevice(g->device));
    if (g->n == 0) return fail(BOHIP_E_STATE, "model has no observations");
    CHK(ensure_fresh(g));
    CHK(ensure_xs(g, R));
    CHK(ensure_score_scratch(g, R));
    if (R > chunk_rows(g, R)) return fail(BOHIP_E_UNSUPPORTED, "more than one K*' chunk");
    CHK(one_time_kernel_setup());
    const PassDims dm = pass_dims(g, R);
    const int64_t N = dm.N, Npad = dm.Npad, Rpad = round_up(R, TILE);   // (this tool's rows of q are dense: no head-room tile, unlike dm.Rpad)
    const int T = dm.T;
    CHK(ensure_pieces(g, T, N));
    const std::vector<int> hv = rows_halves(g->hpieces);
    HIPCHK(hipMemcpyAsync(g->dXs, Xs, (size_t)R * g->d * 8, hipMemcpyHostToDevice, g->stream));
    CHK(launch_kstar_any(g, g->dXs, 0, R, Npad, make_hyper(g)));
    std::vector<double> q((size_t)2 * T * Rpad), mu((size_t)Rpad);
    if (path == 0) {
        CHK(launch_trigemm_on(g, g->dKsT, g->dpieces, g->n_pieces, (int)((R + CTILE - 1) / CTILE), g->dq, Rpad, g->dmu_raw, FuseParams{}));
        HIPCHK(hipMemcpyAsync(q.data(), g->dq, q.size() * 8, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipMemcpyAsync(mu.data(), g->dmu_raw, mu.size() * 8, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        for (int t = 0; t < 2 * T; ++t) std::memcpy(q_out + (size_t)t * R, q.data() + (size_t)t * Rpad, (size_t)R * 8);
        std::memcpy(mu_out, mu.data(), (size_t)R * 8);
        return 0;
    }
    if (path == 3) {
        const int m = prune_tiles(T);
        if (m <= 0 || m >= T) return fail(BOHIP_E_UNSUPPORTED, "no pruning at this size");
        const std::vector<int> ph = phase_a_jobs(g->hpieces, m);
        int* dj = nullptr;
        HIPCHK(hipMalloc(&dj, ph.size() * sizeof(int)));
        hipMemcpyAsync(dj, ph.data(), ph.size() * sizeof(int), hipMemcpyHostToDevice, g->stream);
        hipMemsetAsync(g->dq, 0, q.size() * 8, g->stream);
        const int rc = launch_phase_a(g, g->dKsT, dj, (int)ph.size(), (int)((R + CTILE - 1) / CTILE), g->dq, Rpad);
        hipMemcpyAsync(q.data(), g->dq, q.size() * 8, hipMemcpyDeviceToHost, g->stream);
        const hipError_t e = hipStreamSynchronize(g->stream);
        hipFree(dj);
        if (rc != 0) return rc;
        if (e != hipSuccess) return fail(BOHIP_E_HIP, hipGetErrorString(e));
        for (int t = 0; t < 2 * T; ++t) std::memcpy(q_out + (size_t)t * R, q.data() + (size_t)t * Rpad, (size_t)R * 8);
        std::memset(mu_out, 0, (size_t)R * 8);
        return 0;
    }
    std::vector<int> list((size_t)R);
    for (int64_t i = 0; i < R; ++i) list[i] = (int)(R - 1 - i);
    const unsigned n = (unsigned)R;
    char* d = nullptr;
    const size_t o_q = 0, o_mu = o_q + q.size() * 8, o_l = o_mu + mu.size() * 8, o_h = o_l + list.size() * 4, o_c = o_h + hv.size() * 4;
    HIPCHK(hipMalloc(&d, o_c + 16));
    int rc = 0;
    hipMemcpyAsync(d + o_l, list.data(), list.size() * 4, hipMemcpyHostToDevice, g->stream);
    hipMemcpyAsync(d + o_h, hv.data(), hv.size() * 4, hipMemcpyHostToDevice, g->stream);
    hipMemcpyAsync(d + o_c, &n, 4, hipMemcpyHostToDevice, g->stream);
    rc = launch_trigemm_rows(g, g->dKsT, (const int*)(d + o_h), (int)hv.size(), (const int*)(d + o_l), (const unsigned*)(d + o_c), (int)R,
                             (double*)(d + o_q), Rpad, (double*)(d + o_mu), path == 2 ? 1 : 0);
    hipMemcpyAsync(q.data(), d + o_q, q.size() * 8, hipMemcpyDeviceToHost, g->stream);
    hipMemcpyAsync(mu.data(), d + o_mu, mu.size() * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e = hipStreamSynchronize(g->stream);
    hipFree(d);
    if (rc != 0) return rc;
    if (e != hipSuccess) return fail(BOHIP_E_HIP, hipGetErrorString(e));
    for (int t = 0; t < 2 * T; ++t)
        for (int64_t i = 0; i < R; ++i) q_out[(size_t)t * R + list[i]] = q[(size_t)t * Rpad + i];
    for (int64_t i = 0; i < R; ++i) mu_out[list[i]] = mu[i];
    return 0;
}
// tests only: round 2's list length of the handle's last pruned call (the pinned word prune_wanted reads; 0 after a backoff), -1: none yet
int64_t bohip_debug_prune_stat(bohip_gp* g) {
    if (!g || !g->hprune_stat) return -1;
    return (int64_t)__atomic_load_n(g->hprune_stat.get(), __ATOMIC_RELAXED);
}
// tests only: round 2's form in the handle's pruned calls -- -1 the library's rule, 0 the steady form (one launch), 1 the long form
int bohip_debug_prune_round2_form(bohip_gp* g, int form) {
    if (!g || form < -1 || form > 1) return fail(BOHIP_E_ARG, "bad arguments");
    g->prune_r2_form = form;
    return 0;
}
// tests only (tests/test_prune_poison_gpu.py): the handle's K*' buffer and the pruned pass's packed rows set to all-ones bytes
// (NaNs), so that a value-only call which reads an element that none of its own launches wrote cannot give the right record
int bohip_debug_kstar_poison(bohip_gp* g) {
    if (!g) return fail(BOHIP_E_ARG, "bad arguments");
    HIPCHK(hipSetDevice(g->device));
    if (g->dKsT) HIPCHK(hipMemsetAsync(g->dKsT, 0xff, (size_t)(g->kst_rows + TILE) * g->ld * 8, g->stream));
    if (g->dpr && g->pr_ks_len) HIPCHK(hipMemsetAsync(g->dpr, 0xff, std::min(g->pr_ks_len, g->dpr.capacity()), g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}
int bohip_debug_set_chol_inv_g(int g_new) {
    return g_chol_inv_g.exchange(std::min(64, std::max(0, g_new)));   // (atomic; a refit in flight on another thread may see either value)
}
// tools only (tools/exec_throughput.py): how fast does the executor kernel get through its task list when NOTHING has to be waited for?
// The records of the queues in `qmask` run with their counters removed (every task runnable at once, no chain kernel beside them), on
// whatever the matrices hold: the time is the floor under any schedule of the same records.  hot = 1: every operand address of the bulk
// and wave records points at the first panel of the scratch matrix (L2-resident) -- the same instruction stream without its fabric-side
// traffic.  The model's factor and inverse are garbage afterwards (the handle is marked stale: the next use refits).
int bohip_debug_exec_throughput(bohip_gp* g, unsigned qmask, int hot, int wgs, double* ms_out, double* gflop_out) {
    if (!g || !ms_out || g->n == 0) return BOHIP_E_ARG;
    hipSetDevice(g->device);
    CHK(one_time_kernel_setup());
    const int T = row_tiles(g);
    if (T <= 3) return BOHIP_E_UNSUPPORTED;
    std::vector<ExTask> all, run;
    int qb[EX_NQ + 1], qb2[EX_NQ + 1];
    exec_task_list(g->dL, g->dS, g->dW, g->dWT, g->dchol_flags, g->ld, T, g_chol_nsf, g_chol_inv_g, all, qb);
    double fl = 0.0;
    qb2[0] = 0;
    for (int qi = 0; qi < EX_NQ; ++qi) {
        if ((qmask >> qi) & 1u)
            for (int i = qb[qi]; i < qb[qi + 1]; ++i) {
                ExTask t = all[i];
                for (int d = 0; d < EX_NDEP; ++d) { t.dep_idx[d] = EX_NONE; t.dep_want[d] = 0; }
                t.sig_idx[0] = t.sig_idx[1] = EX_NONE;
                t.kc_split = 0; t.dep2_idx[0] = t.dep2_idx[1] = EX_NONE;
                if (hot && (qi == EX_QBULK || qi == EX_QWAVE)) { t.A = g->dS; t.B = g->dS + (int64_t)TILE * g->ld; }
                fl += 2.0 * TILE * CTILE * KC * t.kc;
                run.push_back(t);
            }
        qb2[qi + 1] = (int)run.size();
    }
    if (run.empty()) return BOHIP_E_ARG;
    ExTask* dt = nullptr;
    HIPCHK(hipMalloc(&dt, run.size() * sizeof(ExTask)));
    HIPCHK(hipMemcpy(dt, run.data(), run.size() * sizeof(ExTask), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(g->dchol_flags, 0, chol_flag_words(T) * sizeof(unsigned), g->stream));
    ExQueues q{};
    q.tasks = dt;
    for (int i = 0; i <= EX_NQ; ++i) q.qbeg[i] = qb2[i];
    q.flags = g->dchol_flags;
    q.abort = g->dchol_flags + chol_abort_word(T);
    q.heads = q.abort + 1;
    q.ld = g->ld;
    q.spin_ticks = g_chol_spin_ticks;
    const int exec_wgs = wgs > 0 ? wgs : std::max(2, std::min(g_chol_exec_wgs > 0 ? g_chol_exec_wgs : 1 << 20, 2 * std::max(1, device_cus() - (9 + g_chol_nsf + 6))));
    q.nurgent = std::max(1, std::min(exec_wgs / 8, g_chol_exec_urgent > 0 ? g_chol_exec_urgent : (T >= 56 ? 16 : 32)));
    const int pairs_ = g_chol_exec_pairs == 0 ? 0 : 1;
        q.stride[0] = 1; q.stride[1] = 1; q.stride[2] = pairs_ ? 2 : 1; q.stride[EX_QBULK] = pairs_ >= 2 ? 2 * std::min(pairs_, 4) : (pairs_ ? 2 : 1);
    q.stride[EX_QROWS] = q.stride[EX_QWAVE] = g_chol_exec_inv_pairs ? 2 : 1;
    q.fill_inv = g_chol_exec_fill_inv;
    q.patience_ticks = (unsigned)g_chol_exec_patience_us * 100u;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, g->stream));
    hipLaunchKernelGGL(k_chol_exec, dim3(exec_wgs), dim3(GEMM_THREADS_8), glds3_lds_bytes<4>(), g->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, g->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(dt);
    *ms_out = ms;
    if (gflop_out) *gflop_out = fl * 1e-9;
    g->stale = true;
    g->w_done = false;
    return 0;
}
#if BOHIP_CHOL_TRACE
int bohip_debug_chol_trace_read(unsigned long long* out, int64_t n_words) {   // tools only
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bohip::g_chol_trace), (size_t)n_words * 8) == hipSuccess ? 0 : -3;
}
int bohip_debug_exec_trace_read(unsigned long long* out, int64_t n_words) {   // tools only
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bohip::g_ex_trace), (size_t)n_words * 8) == hipSuccess ? 0 : -3;
}
#endif
#if BOHIP_TRACE
int bohip_debug_trace_read(unsigned long long* out, int64_t n_words) {   // tools only
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bohip::g_trace), (size_t)n_words * 8) == hipSuccess ? 0 : -3;
}
int bohip_debug_phase_read(unsigned long long* out, int64_t n_words) {   // tools only
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bohip::g_phase), (size_t)n_words * 8) == hipSuccess ? 0 : -3;
}
#endif
}  // extern "C"
