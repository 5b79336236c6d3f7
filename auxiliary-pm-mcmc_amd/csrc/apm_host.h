// What the host orchestration units share: the context, the cross-stream edges, error and
// profiling plumbing, and the functions one unit calls in another. The kernel launchers are in
// apm_internal.h; the C-ABI (include/apm.h) is implemented in capi.cpp.
//   host_ctx.cpp      context allocation, environment knobs, stream skew, profiling, read-back,
//                     per-call uploads, fp64 factors of wide slots
//   host_chol64.cpp   update-list caches, the fp64 two-level Cholesky schedule (two forms)
//   host_newton.cpp   fp32 Newton factorisation with its lookahead, the Newton loop, fp64 rerun
//   host_theta.cpp    the theta-call: concurrent chol(K), posterior factor, guard, ICM check
//   host_laplace.cpp  apm_laplace's fit and covariance, the predictive and gradient paths
//   host_ep.cpp       the sweep loop of parallel expectation propagation (ep.hip)
//   host_predict_joint.cpp  the joint Laplace / EP predictive's tail: covariance, factor, draws
//   host_is_predict.cpp  the importance-sampling predictive's tail after an IS theta-call
//   host_is_diag.cpp  block estimates and weight diagnostics of the IS estimate over replicates
//   host_is_loo.cpp   leave-one-out predictive densities from the IS samples of a cached u-call
//   host_is_psis.cpp  their Pareto-smoothed form and the Pareto k-hat of the ratios' tails
// Everything shared has hidden visibility: the library exports the apm_* functions only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/apm.h"
#include "apm_internal.h"

#define HIPC(x)                                                                              \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess)                                                                \
            throw HipError{std::string(#x) + ": " + hipGetErrorString(e_)};                  \
    } while (0)

namespace apm_host __attribute__((visibility("hidden"))) {

struct ProfRec {
    hipEvent_t a, b;
    int kind;
    double work;
};

// per chain: the trace(C) below which the reference's route to chol(C) is checked (icm_check):
// C's mean diagonal below APM_ICM_Q^-1 of K's largest diagonal entry, i.e. K - V^T V cancels
// ~log10(APM_ICM_Q) digits or more (1e-7 of K_ii at the golden ICM theta icm_a, 1e-5 at icm_b;
// ~1/4 at configs[2]'s sigma = e^18.5, and no chain of the bench's stationary states: unchecked)
#define APM_ICM_Q 1.0e3

// The cross-stream edges of a theta-call, one event each (DESIGN.md §11 names the producer and
// the consumer of every one). No event is recorded again before the wait that names its previous
// record has been enqueued: the per-panel edges are indexed by panel; the Newton lookahead's
// per-panel pair is recorded once per factorisation, and a factorisation starts only after the
// previous one's last far update was joined into the main stream.
struct Edges {
    hipEvent_t gram_k = nullptr;       // main -> s2: the Gram wrote K (and BL's first panel)
    hipEvent_t cholk_done = nullptr;   // s2 -> main: L_K final in BL, its log-det in ldet + nb
    hipEvent_t y2 = nullptr;           // main -> s2: L_K J formed in BL (k_form_y2_rev)
    hipEvent_t bottom_done = nullptr;  // s2 -> main: the fp32 bottom block (S32) final
    std::vector<hipEvent_t> cholk_rel; // main -> s2, per chol(K) panel: its release (no data)
    std::vector<hipEvent_t> lp_panel;  // main -> s2, per panel of L': tiles and inverses final
    std::vector<hipEvent_t> df;        // main -> s3, per Newton panel: its columns + planes final
    std::vector<hipEvent_t> far;       // s3 -> main, per Newton panel: its far update done
    std::vector<hipEvent_t*> all() {
        std::vector<hipEvent_t*> v{&gram_k, &cholk_done, &y2, &bottom_done};
        for (auto* w : {&cholk_rel, &lp_panel, &df, &far})
            for (hipEvent_t& e : *w) v.push_back(&e);
        return v;
    }
};

// a device-resident update list (tile, super-tile or quad-tile order) and its length
typedef std::pair<unsigned*, int> DevList;
typedef std::map<std::tuple<int, int, int, int, int, int>, DevList> ListCache;

// The pinned staging buffers, every field max_batch (B) entries long. The per-call uploads are
// single copies that rely on a field's neighbours, on the host as on the device:
//   hpin: [slots | ubufs] int64 (-> d_slots | d_ubufs), [h3ok | h3post | invok] int (-> h3ok ..),
//         one int of padding per chain, [icm thresholds] double (-> icm_thr)
//   hblk: the 7 B words of the d_i3 block (apm_u_normal / apm_u_combine), fields of StageBlk
//   hx:   the read-back buffer, sized for a theta-call's [logf double | status | n_iter | wide]
struct StagePin {
    int64_t B;
    size_t slots() const { return 0; }
    size_t ubufs() const { return slots() + sizeof(int64_t) * B; }
    size_t h3ok() const { return ubufs() + sizeof(int64_t) * B; }
    size_t h3post() const { return h3ok() + sizeof(int) * B; }
    size_t invok() const { return h3post() + sizeof(int) * B; }
    size_t icm() const { return invok() + 2 * sizeof(int) * B; }
    size_t bytes() const { return icm() + sizeof(double) * B; }
};
enum StageBlk {  // word offsets, in units of B: ubufs / dst share the first field
    BLK_I3 = 0, BLK_A = 1, BLK_B = 2, BLK_CA = 3, BLK_CB = 4, BLK_SEEDS = 5, BLK_CTRS = 6,
    BLK_FIELDS = 7
};
inline size_t read_back_bytes(int64_t B) { return (sizeof(double) + 3 * sizeof(int)) * B; }

}  // namespace apm_host

struct __attribute__((visibility("hidden"))) apm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int kind = 0, n = 0, d = 0, np = 0, nb = 0, P = 0, S = 0, sp = 0;
    int max_batch = 0, n_slots = 0, n_ubufs = 0;
    // tiles per outer panel of the fp64 factorisations and of the Newton matrix (<= 14: the
    // dataflow panel's progress word packs the column step in 4 bits, 15 = failed;
    // rhs_row_update32 covers a depth of 16 tiles; the explicit-inverse panels need 8)
    static constexpr int outer = 8, outer32 = 8;
    static constexpr int symv_tpw = 2;  // K x: lower tiles per workgroup (launch_symv)
    std::vector<int> slot_refs;  // owners of each cache slot (apm_cache_*; 0 = free)
    std::vector<int> slot_wide;  // host mirror of Sl.wide (read back with each theta-call)
    // the last theta-call into the slot failed (its status != 0): the slot was not written, or its
    // value is withheld - apm_u_eval_diag / apm_is_spread report NaN for it
    std::vector<int> slot_failed;
    // fp64 factors of the wide slots: one np x np buffer attached per wide slot (Sl.L64 is the
    // device copy of l64_h), returned to l64_free when its slot is rewritten narrow
    std::vector<double*> l64_h, l64_free;
    double** l64_d = nullptr;
    double eps = 1e-8, tol = 1e-4;
    int lik = APM_LIK_PROBIT;  // apm_set_likelihood: p(y|f) of every later call on the context
    int64_t max_iters = 1000;
    std::string err;
    // device data
    double *X = nullptr, *y = nullptr, *theta = nullptr;
    MatB K{}, A{};
    double *Dinv = nullptr, *ldet = nullptr, *out = nullptr, *partial = nullptr;
    int64_t dstride = 0, lstride = 0, pstride = 0;
    NewtonVecs v{};
    double* vecbase = nullptr;
    double* rvec = nullptr;   // 3 refinement vectors per chain (mixed-precision Newton)
    double* sympart = nullptr;  // symmetric K x partials: nb*nb*64 per chain (launch_symv)
    int64_t sstride = 0;
    bool mixed = true;        // APM_MIXED=0: fp64 Newton factorisation (development knob)
    int n_refine = 3;         // maximum refinement steps per solve
    double refine_tol = 1e-3; // acceptance of a refinement step (k_refine_check)
    int *active = nullptr, *status = nullptr, *n_iter = nullptr;
    int* refining = nullptr;  // chains still refining their Newton solve
    double* refine_prev = nullptr;  // max|d| of the previous refinement step per chain
    int64_t n_refine_steps = 0, n_fp64_rerun = 0;  // statistics (apm_prof_read APM_PROF_STATS)
    int64_t n_icm_check = 0;  // chains whose C was formed the reference's way (icm_check)
    int64_t n_guard = 0;      // chains failed by the guard (APM_STATUS_GUARD)
    // APM_ICM_Q: the threshold of the check of the reference's chol(C) (icm_check; test knob: a
    // huge value checks every chain, 0 checks none)
    double icm_q = APM_ICM_Q;
    int64_t *d_slots = nullptr, *d_ubufs = nullptr, *d_i3 = nullptr;  // d_ubufs = d_slots + B
    // pinned host staging of the per-call uploads (one H2D of slots + ubufs; the per-chain
    // flags and icm thresholds): layout StagePin
    char* hpin = nullptr;
    int64_t* hblk = nullptr;  // pinned mirror of the d_i3 .. d_ctrs block (StageBlk)
    double* hth = nullptr;    // pinned theta staging (B x P)
    // read-back buffer: mapped, coherent pinned host memory (read_back_bytes) written by k_export,
    // dx its device address
    unsigned* hx = nullptr;
    unsigned* dx = nullptr;
    double *d_ca = nullptr, *d_cb = nullptr;
    uint64_t *d_seeds = nullptr, *d_ctrs = nullptr;
    double* U64 = nullptr;
    SlotSet Sl{};
    UPool Up{};
    std::vector<void*> allocs;
    // K's upper triangle holds valid data (host-uploaded K); otherwise every K x product uses the
    // symmetric lower-tile kernel (launch_symv)
    bool k_full = false;
    // profiling
    int prof = 0;  // apm_prof_enable level
    std::vector<hipEvent_t> evpool;
    size_t evnext = 0;
    std::vector<apm_host::ProfRec> recs;
    // update lists per launch shape, built once, kept on the device (cached_list): 64x64 tiles
    // and 128x128 super-tiles keyed by (i0, R, j0, jend, gap lo, gap hi), the super-tiles with a
    // row tile of its own (solo) apart, the lookahead's extended lists keyed by (i0, R, j0, jend,
    // rhs, jext), the 256x256 quad tiles by (i0, R, j0, jend)
    apm_host::ListCache tile_lists, super_lists, super_lists_solo, super_lists_ext;
    std::map<std::tuple<int, int, int, int>, apm_host::DevList> quad_lists;
    bool h3 = true;       // APM_H3=0: fp32 operands in the fp32 factorisations' outer updates
    bool h3_now = false;  // some chain of the current theta-call may use fp16x3 updates
    bool h3_all = false;  // ... and every chain may (the quad-tile far updates need that)
    bool h3post_all = false;  // every chain takes fp16x3 operands in the posterior bottom block
    int* h3ok = nullptr;  // per chain: fp16x3 allowed (range check on theta_0, chol32_update.hip)
    int* h3post = nullptr;  // the same for the posterior factor's fp32 bottom block (h3ok + B)
    // per chain: explicit-inverse Newton panels allowed (h3ok + 2B): their fp16x3 operands are
    // Schur-complement entries of B, bounded by max B_ii <= 1 + K_ii (not by sqrt(B_ii) as the
    // walk's solved entries are), so the range check is on 1 + K_ii itself (chol32_panel.hip)
    int* invok = nullptr;
    bool inv_any = false, inv_all = false;
    double* icm_thr = nullptr;  // per chain: SlotSet::icm_thr
    // the bottom block of the posterior factor [[J M J],[L_K J]] (the TRSM that yields chol(C) J)
    // in fp32 panel by panel beside the fp64 factorisation of J M J (postcov.hip); chains whose
    // trace(C) exceeds Sl.post_q are recomputed in fp64 (n_post64 counts them)
    int* hmask = nullptr;  // pinned: the chains of such a recomputation
    int64_t n_post64 = 0;
    // the Newton factorisation's dataflow launches also write the panel's fp16x3 operand planes
    // (Planes16), which the trailing updates stage with LDS-DMA. plane_bufs buffers of max_batch
    // chains each, one behind the other: one per outer panel for the left-looking far updates
    // (far_left: panel q's far tiles take panels 0 .. q-2 in one launch, chol_range32), or two by
    // panel parity for the right-looking ones (the lookahead's far update reads panel K's while
    // the dataflow launch of K + 1 writes its own): APM_FAR_LEFT=0, or the allocation failed
    unsigned short* planes = nullptr;
    int64_t plane_cs = 0;  // halves per chain and buffer
    int plane_bufs = 2;
    bool far_left = false;
    // explicit-inverse panels (chol32_panel.hip k_zinv_* / k_panel_inv_gemm32): the dataflow launch
    // walks the diagonal block and the right-hand-side row only; Z = inv(L_D) per chain (fp32
    // scratch zt: Z, Z^T, T^T; fp16x3 planes zplanes) and one GEMM per row tile below
    float* zt = nullptr;
    unsigned short* zplanes = nullptr;
    // per (chain, row tile) progress words, then [dataflow timeouts][TRSV timeouts][ticket]
    unsigned long long* dfprog = nullptr;
    unsigned long long df_fact = 0;        // factorisations so far (the words' monotonic base)
    // the arrival-ticket counter of the main stream's hand-over kernels (SpinCtl): reset at the
    // start of every theta-call, ticket_base = the tickets the call's launches have drawn so far
    unsigned long long ticket_base = 0;
    int spin_df = 1 << 22, spin_trsv = 1 << 20;  // poll bounds (APM_SPIN_LIMIT: tests only)
    // chains whose work the roofline accounting credits (Newton: the unconverged ones after the
    // previous convergence read; update_flops x live_n instead of x count)
    int live_n = 0;
    // chol(K) of the mixed-precision IS theta-call on a low-priority second stream, concurrent
    // with the Newton iterations, and the fp32 bottom block of the posterior factor on the same
    // stream; the far part of each Newton trailing update on stream3 beside the next panel's
    // dataflow launch (one-panel lookahead, chol_range32)
    hipStream_t stream2 = nullptr;
    hipStream_t stream3 = nullptr;
    // pacing of the concurrent chol(K) (feed_chol_k): panels it may still release in this Newton
    // iteration, from the previous theta-call's iteration count (newton_last; 0: no pacing)
    int cholk_quota = 1 << 30, newton_last = 0;
    apm_host::Edges ev;  // one event per cross-stream edge
    int skew = 0;  // APM_SKEW (tests only): delay kernels in front of launches (skew_point), bit 2
                   // drops the bottom_done wait
    // per-chain guard data (k_guard_*): [1/2 log|B| of the last Newton factor][1/2 log|K|]
    // [residuals r1 .. r4 of the last theta-call]
    double* guard = nullptr;
    double* guard_rows = nullptr;  // the slot writer's row residuals of C_chol g = f_post (B x np)
    int *active2 = nullptr, *status2 = nullptr;
    // chol(K) is enqueued one outer panel at a time, each released when the main stream enters a
    // single-workgroup-per-chain TRSV (3/4 of the CUs idle) - see feed_chol_k
    int cholk_next = -1, cholk_count = 0;
    // the Gram wrote only the first outer panel's tile columns into chol(K)'s working copy: the
    // first trailing update then reads its old tiles from K (out of place, k_chol_update_t128 S)
    bool cholk_partial = false;
    // the predictive path (apm_predict), allocated at its first call: one block of test inputs
    // (np x d), the mu* partials (max_batch x nb x np), the three outputs (max_batch x np each) and
    // behind them, as the host computes them (max_batch each): the chains' s = exp(theta_0) (psig,
    // the cross-covariance's), their prior variance k** = s + beta (pkss: s itself without the
    // constant term) and beta = exp(theta_{P-1}) (pbet: 0 without it). A kind with the linear term
    // (DESIGN.md §25): lambda = exp(theta_{P-1}) in plam (beta is then theta_{P-2}'s) and the
    // staged test rows' squared norms in pxn (np), k** = pkss[b] + plam[b] pxn[r]; both stay
    // null for every other kind, and no kernel launched for one reads them
    double *pxs = nullptr, *ppart = nullptr, *pmean = nullptr, *pvar = nullptr, *pprob = nullptr;
    double *psig = nullptr, *pkss = nullptr, *pbet = nullptr, *plam = nullptr, *pxn = nullptr;
    // max_i |x_i|^2 and sum_i |x_i|^2 of the training inputs (apm_create; the range flags of a
    // kind with the linear term: K_ii = s + beta + lambda |x_i|^2 + eps differs by row)
    double x2max = 0.0, x2sum = 0.0;
    // the gradient path (apm_laplace_grad), allocated at its first call: six vectors per chain
    // (dS, g, s2, t = K s2, u = -R t, q; max_batch x np each), the super-tile partials
    // (max_batch x ns (ns + 1) / 2 x P) and the gradients (max_batch x P)
    double *gvec = nullptr, *gpart = nullptr, *gout = nullptr;
    // expectation propagation (apm_ep_eval / apm_ep_predict / apm_ep): the settings of apm_set_ep
    // and the site and scratch vectors (EpVecs), allocated at the first EP call
    double ep_damping = 0.8, ep_tol = 1e-8;
    int64_t ep_max_sweeps = 100;
    // apm_set_ep_quadrature: the tilted moments by the rule of ep_quad.h (k_ep_sites_q) for
    // either likelihood, which opens EP to the logit; 0 keeps the closed-form probit kernel and
    // every refusal of a logit context
    int ep_quad = 0;
    EpVecs ep{};
    // the importance-sampling predictive (apm_is_predict), allocated at its first call: the
    // reversed transpose of each chain's U buffer (max_batch x sp x np), the weights (max_batch x
    // sp) and ess (max_batch), v* and c per test row (max_batch x np each), a vector of ones
    // (max_batch x np: k_gram_cross's Ws) and the sample-tile partials (max_batch x 3 x np x sp/64)
    double *is_ut = nullptr, *is_w = nullptr, *is_ess = nullptr, *is_vstar = nullptr;
    double *is_c = nullptr, *is_ones = nullptr, *is_part = nullptr;
    // the block diagnostics (apm_u_eval_diag / apm_is_spread), allocated at their first call: the
    // staging array (3 x max_batch x APM_SPREAD_MAX_BLOCKS) and the replicates' Philox keys
    // ([seeds: max_batch][counters: APM_SPREAD_MAX_BLOCKS x max_batch])
    double* sd_out = nullptr;
    uint64_t* sd_keys = nullptr;
    // the leave-one-out densities (apm_is_loo), allocated at its first call: log wbar (max_batch x
    // sp) and ess (max_batch), the sample-tile partials (max_batch x 5 x np x sp/64) and the four
    // row outputs (4 x max_batch x np)
    double *loo_w = nullptr, *loo_ess = nullptr, *loo_part = nullptr, *loo_out = nullptr;
    // the Pareto-smoothed densities (apm_is_loo_psis), one allocation at its first call (psis_t is
    // its base and the sign that it exists): the log ratios (max_batch x np x sp), log wbar
    // (max_batch x sp) and k_is_logw's ess (max_batch), and the outputs (loo_psis and khat:
    // 2 x max_batch x np; khat_w: max_batch)
    double *psis_w = nullptr, *psis_t = nullptr, *psis_out = nullptr;
    // the joint predictive (apm_predict_joint), allocated at its first call that draws: the labels
    // (np) and the chains' Philox keys ([seeds | counters], max_batch each); and, grown to the
    // largest number of draws asked for so far (jn_cap rows, a multiple of 64), the normals Xi^T
    // (max_batch x jn_cap x np), the tile partials of the draws' log-likelihoods (max_batch x nb x
    // jn_cap) and, at the first call that wants them back, the draws (max_batch x jn_cap x np)
    double *jn_ys = nullptr, *jn_xi = nullptr, *jn_part = nullptr, *jn_draws = nullptr;
    uint64_t* jn_keys = nullptr;
    int64_t jn_cap = 0;
};

namespace apm_host __attribute__((visibility("hidden"))) {

template <class T>
T* dalloc(apm_ctx* c, size_t count) {  // (at least one element)
    void* p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess)
        throw HipError{"hipMalloc(" + std::to_string(count * sizeof(T)) +
                       " bytes): " + hipGetErrorString(e)};
    c->allocs.push_back(p);
    return static_cast<T*>(p);
}

// ---- host_ctx.cpp ---------------------------------------------------------------------------
void init_ctx(apm_ctx* c, int device, int kind, const double* X, int64_t n, int64_t d,
              int64_t ldx, const double* y, double eps, int64_t S, int64_t max_batch,
              int64_t n_slots, int64_t n_ubufs);
void free_ctx(apm_ctx* c);
// the cached PRECOMPUTED context of a stand-alone call's shape (apm_laplace_lik, apm_ep), created
// at the first call (c null) and given the call's labels
void standalone_ctx(apm_ctx*& c, int device, int64_t n, const double* y);

struct SkewState {  // APM_SKEW (tests only): the calling thread's skew_point setting
    int mode = 0;
    hipStream_t main = nullptr, s2 = nullptr, s3 = nullptr;
};
struct SkewScope {  // an API entry point's launches belong to context c
    SkewState prev;
    explicit SkewScope(const apm_ctx* c);
    ~SkewScope();
};

hipEvent_t next_event(apm_ctx* c);  // from the context's pool (apm_prof_read's reset returns them)
struct ProfScope {  // times what is enqueued on s (default: the main stream) during its lifetime
    apm_ctx* c;
    int kind;
    double work;
    hipStream_t s;
    hipEvent_t a{}, b{};
    bool on = false;
    ProfScope(apm_ctx* c_, int k, double w, hipStream_t s_ = nullptr)
        : c(c_), kind(k), work(w), s(s_ ? s_ : c_->stream) {
        // the all-updates kinds time every in-panel launch: detailed level (2) only
        const bool all_upd = kind == APM_PROF_CHOL_UPDATE || kind == APM_PROF_CHOL_UPDATE32;
        if (kind >= 0 && c->prof >= (all_upd ? 2 : 1)) {
            on = true;
            a = next_event(c);
            b = next_event(c);
            HIPC(hipEventRecord(a, s));
        }
    }
    ~ProfScope() {
        if (on && hipEventRecord(b, s) == hipSuccess)
            c->recs.push_back(ProfRec{a, b, kind, work});
    }
};

inline void sync(apm_ctx* c) { HIPC(hipStreamSynchronize(c->stream)); }

// Read back up to four small per-chain device arrays (after the work enqueued so far on the
// main stream) and wait: one k_export launch into the mapped host buffer, a stream
// synchronisation, host copies.
struct RB {
    const void* src;
    int bytes;
    void* host;
};
void read_back(apm_ctx* c, std::initializer_list<RB> l);

// the fields of hpin (StagePin)
inline StagePin pin_of(const apm_ctx* c) { return StagePin{c->max_batch}; }
inline int64_t* pin_slots(apm_ctx* c) {
    return reinterpret_cast<int64_t*>(c->hpin + pin_of(c).slots());
}
inline int64_t* pin_ubufs(apm_ctx* c) {
    return reinterpret_cast<int64_t*>(c->hpin + pin_of(c).ubufs());
}
inline int* pin_h3(apm_ctx* c) { return reinterpret_cast<int*>(c->hpin + pin_of(c).h3ok()); }
inline int* pin_h3post(apm_ctx* c) { return reinterpret_cast<int*>(c->hpin + pin_of(c).h3post()); }
inline int* pin_inv(apm_ctx* c) { return reinterpret_cast<int*>(c->hpin + pin_of(c).invok()); }
inline double* pin_icm(apm_ctx* c) { return reinterpret_cast<double*>(c->hpin + pin_of(c).icm()); }
inline int64_t* blk_field(apm_ctx* c, StageBlk f) { return c->hblk + (int64_t)f * c->max_batch; }

void upload_idx(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs);
void upload_h3(apm_ctx* c, int count);
// the thetas of a call (count x P, row stride ldt) -> pinned staging -> device; returns the
// staged copy
const double* upload_thetas(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt);
// beta = exp(theta_{P-1}) of a biased kind's theta (P entries), 0 for every other kind: with it
// K_ii = exp(theta_0) + beta + eps and k** = exp(theta_0) + beta
inline double cov_beta(int kind, int P, const double* theta) {
    const KernelKind kk = kernel_kind_of(kind);
    return kk.bias ? std::exp(theta[P - 1 - kk.linear]) : 0.0;
}
// lambda = exp(theta_{P-1}) of a kind with the linear term (beta is then theta_{P-2}'s), 0 for
// every other kind: K_ii = exp(theta_0) + beta + lambda |x_i|^2 + eps
inline double cov_lambda(int kind, int P, const double* theta) {
    return kernel_kind_of(kind).linear ? std::exp(theta[P - 1]) : 0.0;
}
// the identity-padded copy of a host K (n x n, row stride ldk) -> chain 0's K, both triangles
// (k_full), staged in Kp, which the caller keeps until its next sync; returns max |K_ii|
double upload_padded_K(apm_ctx* c, const double* K, int64_t ldk, std::vector<double>& Kp);
void attach_l64(apm_ctx* c, int64_t slot);
void detach_l64(apm_ctx* c, int64_t slot);
void upload_l64(apm_ctx* c);

inline Live live_of(apm_ctx* c) { return Live{c->active, c->status}; }

// ---- host_chol64.cpp ------------------------------------------------------------------------
// Where a factorisation runs: stream, liveness, diagonal-inverse / log-det arrays. The main path
// uses the context stream; chol(K) of the IS theta-call runs concurrently on the low-priority
// second stream with its own liveness and the upper halves of Dinv / ldet (theta_eval_impl).
struct Exec {
    hipStream_t s;
    Live lv;
    double* Dinv;
    double* ldet;
    int live_n;  // chains credited by the roofline accounting
};
inline Exec main_exec(apm_ctx* c) {
    return Exec{c->stream, live_of(c), c->Dinv, c->ldet, c->live_n};
}

// Row tiles [lo, hi) known to be zero in panel column k (skipped by panel and update).
struct Gap {
    int lo, hi;
};
typedef Gap (*GapFn)(int k, int nb);
inline Gap no_gap(int, int) { return Gap{0, 0}; }
// [[J M J],[L_K J]] factorisation (postcov.hip): row tile nb+I of L_K J is zero in every column
// tile k < nb-1-I, so at column k only bottom rows >= 2nb-1-k are nonzero.
inline Gap y_gap(int k, int nb) { return Gap{nb, std::max(nb, 2 * nb - 1 - k)}; }

double update_flops(int i0, int R, int j0, int jend, int kc, Gap g, bool syrk_lower = false);
DevList tile_list(apm_ctx* c, int i0, int R, int j0, int jend, Gap g);
DevList super_list(apm_ctx* c, int i0, int R, int j0, int jend, Gap g, int solo = -1);
DevList super_list_ext(apm_ctx* c, int i0, int R, int j0, int jend, int rhs, int jext);
DevList quad_list(apm_ctx* c, int i0, int R, int j0, int jend);
void tracked_update(apm_ctx* c, MatB M, int k0, int kc, int i0, int R, int j0, int jend, Gap g,
                    int plus, int count, int fuse_k = -1, int fail_code = 0,
                    const Exec* ex = nullptr, const MatB* src = nullptr);

// what the two forms of the fp64 schedule rarely need; a call site names what it sets
struct SolveOpts {
    const Exec* ex = nullptr;  // where it runs (default: main_exec)
    GapFn gap = no_gap;        // row tiles known to be zero per panel column
};
struct FactorOpts : SolveOpts {
    // the first outer update reads its old tiles from here (out of place) instead of from M
    const MatB* first_src = nullptr;
    // after_panel(K, Kend): called (host side) once the panel's columns are final, before its
    // outer update is enqueued (the posterior factor's fp32 bottom block follows the panels)
    std::function<void(int, int)> after_panel;
};
void chol_factor(apm_ctx* c, MatB M, int k0, int k1, int R, int Cb, int fail_code, int count,
                 const FactorOpts& o = FactorOpts());
void chol_solve_rows(apm_ctx* c, MatB M, int k1, int row_start, int R, int Cb, int count,
                     const SolveOpts& o = SolveOpts());

// ---- host_newton.cpp ------------------------------------------------------------------------
unsigned long long* spin_words(apm_ctx* c);  // [dataflow timeouts][TRSV timeouts][ticket]
void reset_tickets(apm_ctx* c);
void newton(apm_ctx* c, int count, std::vector<int>& st_h, bool mixed, int live0);
void newton_is(apm_ctx* c, int count, std::vector<int>& st_h);

// ---- host_theta.cpp -------------------------------------------------------------------------
void feed_chol_k(apm_ctx* c);
void drain_chol_k(apm_ctx* c);
void u_eval_device(apm_ctx* c, int count, bool wide);
// The frame of a cached u-call (apm_u_eval, the diagnostics, the two LOO calls), whose arguments
// the caller has checked. The opening stages the call's slots and U buffers, clears the device
// statuses and, unless eval is false (apm_is_spread redraws the buffers first), enqueues
// u_eval_device: k_ugemm leaves the per-sample sums in c->partial, k_lme log f in c->out. It
// returns whether a slot of the call is wide (the host mirror), for the f64 twins of later
// launches. A new cached u-call supplies its kernels between the two and names its outputs.
bool u_call_open(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs,
                 bool eval = true);
// The closing copies each row output (count rows of `width` doubles from dev, row stride dev_ld,
// to host, row stride ld) and per-chain scalar (count doubles) whose host pointer is not null,
// then the statuses, synchronises once and writes NaN over the rows and scalars of every chain
// with status != 0 or whose slot's last theta-call failed. A row output without dev is one the
// caller has enqueued the copy of itself: it is only NaN-filled.
struct URows {
    double* host;
    int64_t ld;
    const double* dev;
    int64_t dev_ld, width;
};
struct UScalar {
    double* host;
    const double* dev;
};
void u_call_close(apm_ctx* c, int count, const int64_t* slots, std::initializer_list<URows> rows,
                  std::initializer_list<UScalar> scalars, int* status);
void theta_eval_impl(apm_ctx* c, int est, int count, bool gram, double* out_logf, int* status,
                     int64_t* nops);

// ---- host_laplace.cpp -----------------------------------------------------------------------
void augmented(apm_ctx* c, int count);
// C = K - V^T V of chain 0's last factor (augmented(): the bottom-right of A, lower) -> both
// triangles of C_out (n x n, ldc)
void covariance_out(apm_ctx* c, double* C_out, int64_t ldc);
// apm_laplace's fit of a host K (n x n, ldk) on a stand-alone context whose settings are made:
// the mode into f_out and, where asked for (non-null), the covariance and the LML; nothing but
// status and n_iter_out for a fit that failed
void laplace_on_K(apm_ctx* c, const double* K, int64_t ldk, double* f_out, double* C_out,
                  int64_t ldc, double* lml_out, int64_t* n_iter_out, int* status);
// a Laplace theta-call (Gram, fp64 Newton, LML into lml: count doubles) whose OK chains are then
// made live again (they left the Newton loop with active = 0) for the passes that reuse the last
// Newton factor; returns their number
int laplace_then_live(apm_ctx* c, int count, double* lml, int* status, int64_t* n_iter);
void predict_buffers(apm_ctx* c);
void predict_block(apm_ctx* c, int count, int ms, bool with_cov = false);
// One call's test inputs Xs (m x d, row stride ldxs), a block of at most np rows at a time: the
// constructor uploads the chains' s = exp(theta_0), s + beta and beta to psig / pkss / pbet
// (predict_buffers() first; cov_beta) and, for a kind with the linear term, lambda to plam; upload()
// packs rows [r0, r0 + ms) and sends them to pxs (returns ms; with the linear term their squared
// norms, features in order, go to pxn: once per block, the same for every chain), rows_back() enqueues the copy of
// the block's pmean / pvar / pprob rows to the caller's arrays (count x m, row stride ldo, any of
// them null). The two users copy back differently on purpose: the Laplace / EP predictive every
// row with one 2-D copy per output (only_ok null; rows of failed chains hold stale values, which
// the C-ABI overwrites), the IS predictive the rows of the chains that are OK in only_ok, because
// it leaves the caller's other rows untouched. The object stays alive until the sync after the
// last block.
struct TestInputs {
    apm_ctx* c;
    int count;
    const double* Xs;
    int64_t m, ldxs;
    std::vector<double> xs, sig;
    TestInputs(apm_ctx* c, int count, const double* thetas, int64_t ldt, const double* Xs,
               int64_t m, int64_t ldxs);
    int upload(int64_t r0);
    void rows_back(int64_t r0, int ms, const int* only_ok, double* mean, double* var, double* prob,
                   int64_t ldo);
};
// the predictive distribution of the live chains' state (S^1/2 or W^1/2 in v.Ws, a, the factor in
// A) at the m test inputs, in blocks of the free rows of A; outputs count x m, row stride ldo
void predict_all(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, const double* Xs,
                 int64_t m, int64_t ldxs, double* mean, double* var, double* prob, int64_t ldo);
void grad_buffers(apm_ctx* c);
void grad_block(apm_ctx* c, int count);
// grad_block's second pass for the chains left live by ep_fit: d log Z_EP / d theta into c->gout
void ep_grad_block(apm_ctx* c, int count);

// ---- host_predict_joint.cpp -----------------------------------------------------------------
// The joint predictive's tail for the chains left live by a Laplace theta-call or
// an EP fit (st_h their statuses) at the m <= np test inputs: mean (count x m, row stride ldo),
// cov (count blocks of m rows, row stride ldc, both triangles), n_draws draws of the latent
// function (count x n_draws x m) from the streams (seeds[i], counters[i]) and the joint log
// predictive density of the labels ys under them (count); any output may be null, the last two
// need n_draws > 0. A chain whose chol(Sigma + eps I) fails gets APM_STATUS_CHOL_C in st_h. Rows
// of a chain that is not OK hold stale values, which the C-ABI overwrites.
void predict_joint_tail(apm_ctx* c, int count, const double* thetas, int64_t ldt, int* st_h,
                        const double* Xs, int64_t m, int64_t ldxs, double* mean, int64_t ldo,
                        double* cov, int64_t ldc, int64_t n_draws, const uint64_t* seeds,
                        const uint64_t* counters, double* draws, const double* ys,
                        double* joint_lpd);

// ---- host_is_predict.cpp --------------------------------------------------------------------
// The predictive tail after an APM_EST_IS / APM_EST_IS_EP theta-call on the same context (its
// thetas, slots and ubufs still on the device; st_h the call's statuses) at the m test inputs:
// prob / mean / var (count x m, row stride ldo) and ess (count), any of them null. Rows of a
// chain that is not OK are left untouched. A factorisation that fails in the tail (none can for
// a chain whose theta-call succeeded in exact arithmetic) is reported in st_h.
void is_predict_tail(apm_ctx* c, int count, const double* thetas, int64_t ldt, int* st_h,
                     const double* Xs, int64_t m, int64_t ldxs, double* prob, double* mean,
                     double* var, int64_t ldo, double* ess);

// ---- host_is_diag.cpp -----------------------------------------------------------------------
// The u-path on the call's slots and U buffers and the block reduction (k_lme_blocks) of its
// per-sample sums, n_rep times; before replicate r the U buffers are redrawn from (seeds[i],
// counters[i] + r) when seeds is given (apm_is_spread), else n_rep = 1 and the buffers are read as
// they are (apm_u_eval_diag). Arguments are checked by the caller; logf / ess / wmax (count x
// n_rep nblk, row stride ldo) may be null, NaN for a chain whose slot's theta-call failed.
void is_diag_run(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs,
                 const uint64_t* seeds, const uint64_t* counters, int64_t n_rep, int64_t block,
                 double* logf, double* ess, double* wmax, int64_t ldo, int* status);

// ---- host_is_loo.cpp ------------------------------------------------------------------------
// apm_u_eval's launches on the call's slots and U buffers, then the log-weights, the product with
// the row-wise epilogue and the finish (is_loo.hip). Arguments are checked by the caller; every
// output but status may be null: out_logf and ess (count), loo / lpd / ess_loo / gauss (count x n,
// row stride ldo), NaN for a chain whose slot's theta-call failed.
void is_loo_run(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs,
                double* out_logf, double* loo, double* lpd, double* ess_loo, double* gauss,
                int64_t ldo, double* ess, int* status);

// ---- host_is_psis.cpp -----------------------------------------------------------------------
// apm_u_eval's launches on the call's slots and U buffers, then the log-weights, the product with
// the storing epilogue and the row fits (is_psis.hip). Arguments are checked by the caller; every
// output but status may be null: out_logf and khat_w (count), loo_psis / khat (count x n, row
// stride ldo), logratio (count x n n_imp, row stride ldr), NaN for a chain whose slot's theta-call
// failed.
void is_psis_run(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs,
                 double* out_logf, double* loo_psis, double* khat, int64_t ldo, double* khat_w,
                 double* logratio, int64_t ldr, int* status);

// ---- host_ep.cpp ----------------------------------------------------------------------------
void ep_buffers(apm_ctx* c);
// Parallel EP on K as it stands in c->K (k_full says which triangles) for chains
// [0, count): sets the liveness arrays, runs the sweeps and leaves each converged chain's state
// of its last sweep in place (sites, var and logz in c->ep; S^1/2 in v.Ws, a in v.a, mu in v.f,
// the factor in A / Dinv / ldet); host status per chain in st_h, sweeps in c->n_iter. The OK
// chains are live again on return (active = 1), as after laplace_then_live; returns their number
int ep_fit(apm_ctx* c, int count, std::vector<int>& st_h);
// ep_fit with the copy of the sweep counts enqueued behind it: f.sweeps holds them after the
// caller's next synchronisation of the main stream, until which f stays alive
struct EpFit {
    std::vector<int> st, sweeps;
    int ok = 0;  // chains left OK (and live)
};
void ep_fit_counted(apm_ctx* c, int count, EpFit& f);
// the Gram of the call's thetas (K's lower tiles, as a Laplace theta-call), then ep_fit_counted
void ep_gram_fit(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, EpFit& f);
// count x n device vectors (row stride src_ld) -> host rows (row stride ldo), if asked for
void ep_fetch(apm_ctx* c, double* dst, int64_t ldo, const double* src, int64_t src_ld,
              int64_t count);

}  // namespace apm_host
