// Host orchestration of the theta-call / u-call pipelines.
//
// theta-call (ApproxPosteriorIS, gpdemo/estimators.py:203-241), per batch of chains, one stream:
//   Gram -> Newton loop { prep, K b, form B|rhs, chol(B) (+ forward solve), L^T solve, a, K a,
//   check } -> augmented chol [[B,.],[K W^1/2, K],[0, f_post^T]] -> slot -> L.U + likelihood -> LME
// The only host syncs are one per Newton iteration (convergence flags) and one at the end.
#include <limits>

#include "apm_host.h"

// the guard's bounds (k_guard_check): r1 nats of 1/2 log-determinant between the
// last Newton factor (fp32 with fp16x3 updates) and the fp64 posterior factor, r2 relative, r3
// nats between the fp32 slot's log-diagonal and the fp64 log-determinants, r4 max |C_chol g -
// f_post| over the rows relative to max(1, max |f_post|); measured maxima in
// DESIGN.md §11 (tests/test_gpu_errors.py::test_guard_residuals_are_rounding_sized)
#define GUARD_T1 1.0
#define GUARD_T2 1.0e-6
#define GUARD_T3 5.0e-2
#define GUARD_T4 1.0e-4

namespace apm_host {

// wide: some slot of the call may be wide (theta-calls: unknown until the read-back; u-calls:
// the host mirror) - the f64 MFMA twin is launched as well
void u_eval_device(apm_ctx* c, int count, bool wide) {
    {
        ProfScope ps(c, APM_PROF_UGEMM, (double)c->n * (c->n + 1) * c->S * count);
        launch_ugemm(c->lik, c->Sl, c->d_slots, c->Up, c->d_ubufs, c->y, c->n, c->np,
                     c->partial, c->pstride, c->status, count, wide, c->stream);
    }
    launch_lme(c->partial, c->pstride, c->nb, c->S, c->sp, c->Sl, c->d_slots, c->out, c->status,
               count, c->stream);
}

bool u_call_open(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs, bool eval) {
    upload_idx(c, count, slots, ubufs);
    HIPC(hipMemsetAsync(c->status, 0, sizeof(int) * count, c->stream));
    bool wide = false;
    for (int b = 0; b < count; ++b) wide |= c->slot_wide[slots[b]] != 0;
    if (eval) u_eval_device(c, count, wide);
    return wide;
}

void u_call_close(apm_ctx* c, int count, const int64_t* slots, std::initializer_list<URows> rows,
                  std::initializer_list<UScalar> scalars, int* status) {
    hipStream_t s = c->stream;
    for (const URows& r : rows)
        if (r.host && r.dev)
            HIPC(hipMemcpy2DAsync(r.host, sizeof(double) * r.ld, r.dev, sizeof(double) * r.dev_ld,
                                  sizeof(double) * r.width, count, hipMemcpyDeviceToHost, s));
    for (const UScalar& q : scalars)
        if (q.host)
            HIPC(hipMemcpyAsync(q.host, q.dev, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(status, c->status, sizeof(int) * count, hipMemcpyDeviceToHost, s));
    sync(c);
    // a slot whose last theta-call failed was never written: its values mean nothing
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int b = 0; b < count; ++b)
        if (status[b] != 0 || c->slot_failed[slots[b]]) {
            for (const URows& r : rows)
                if (r.host) std::fill(r.host + b * r.ld, r.host + b * r.ld + r.width, nan);
            for (const UScalar& q : scalars)
                if (q.host) q.host[b] = nan;
        }
}

namespace {

// Posterior-covariance factor through chol(K) (postcov.hip): 4N^3/3 flops instead of the
// augmented 7N^3/3. Leaves chol(C) J in rows [np, 2np) x cols [0, np) of A, g in v.Kb and
// log|B| = log|M| in ldet[0..nb).
MatB bl_of(apm_ctx* c) { return MatB{c->A.base + (int64_t)c->np * c->A.ld, c->A.ld, c->A.cstride}; }

// chol(K) into the bottom-left block BL of the work matrix for the concurrent path: own stream
// (ex.s), liveness (active2 / status2, so that Newton convergence does not mask it) and the upper
// halves of Dinv / ldet (the Newton factorisation uses the lower halves and the top rows of A).
// chol_k_begin copies K and factors the first outer panel; each feed_chol_k call releases the
// next outer panel (panel + its trailing update) behind an event of the main stream, at most
// cholk_quota per Newton iteration (newton(): the panels left spread over the iterations the
// previous call took).
Exec k_exec(apm_ctx* c, hipStream_t s) {
    return Exec{s, Live{c->active2, c->status2}, c->Dinv + (int64_t)c->nb * 4096, c->ldet + c->nb,
                c->cholk_count};
}
void chol_k_panel(apm_ctx* c, const Exec& ex) {
    const int K = c->cholk_next;
    if (K < 0 || K >= c->nb) return;
    FactorOpts o;
    o.ex = &ex;
    // first panel after a partial Gram copy: the trailing update reads K's tiles (out of place)
    if (K == 0 && c->cholk_partial) o.first_src = &c->K;
    chol_factor(c, bl_of(c), K, std::min(K + c->outer, c->nb), c->nb, c->nb, APM_STATUS_CHOL_K,
                c->cholk_count, o);
    c->cholk_next = K + c->outer;
}
void chol_k_begin(apm_ctx* c, int count, const Exec& ex, bool copy = true, bool partial = false) {
    HIPC(hipMemsetD32Async(c->active2, 1, count, ex.s));
    HIPC(hipMemsetAsync(c->status2, 0, sizeof(int) * count, ex.s));
    if (copy)  // (else the Gram wrote K's lower tiles into BL as well, or those of the first
               // outer panel's tile columns: partial)
        launch_copy_lower(c->K, bl_of(c), c->np, ex.lv, count, ex.s);
    c->cholk_partial = !copy && partial;
    c->cholk_next = 0;
    c->cholk_count = count;
    chol_k_panel(c, ex);
}
// all of chol(K) on one stream (the rerun after an fp64 Newton fallback)
void chol_k_into_bl(apm_ctx* c, int count, const Exec& ex) {
    chol_k_begin(c, count, ex);
    while (c->cholk_next >= 0 && c->cholk_next < c->nb) chol_k_panel(c, ex);
    c->cholk_next = -1;
}

}  // namespace

// edge cholk_rel[p] (main -> s2) carries no data: chol(K) works in BL, ldet + nb and the upper
// half of Dinv, which nothing on the main stream touches while it runs (the fp64 Newton rerun,
// which writes BL's first row block, drains it first); it only releases the panel behind the
// main stream's TRSVs, whose single-workgroup-per-chain launches leave most CUs idle
void feed_chol_k(apm_ctx* c) {
    if (c->cholk_next < 0 || c->cholk_next >= c->nb) return;
    if (c->cholk_quota <= 0) return;
    --c->cholk_quota;
    hipEvent_t e = c->ev.cholk_rel[c->cholk_next / c->outer];
    HIPC(hipEventRecord(e, c->stream));
    HIPC(hipStreamWaitEvent(c->stream2, e, 0));
    chol_k_panel(c, k_exec(c, c->stream2));
}

// enqueue what is left of the concurrent chol(K) and order the main stream behind it (edge
// cholk_done, s2 -> main: L_K in BL, the log-dets in ldet + nb, status2)
void drain_chol_k(apm_ctx* c) {
    if (c->cholk_next < 0) return;
    while (c->cholk_next < c->nb) chol_k_panel(c, k_exec(c, c->stream2));
    c->cholk_next = -1;
    HIPC(hipEventRecord(c->ev.cholk_done, c->stream2));
    HIPC(hipStreamWaitEvent(c->stream, c->ev.cholk_done, 0));
}

namespace {

// The bottom block of [[J M J],[L_K J]] after the fp64 factorisation of J M J = L' L'^T: the TRSM
// (L_K J) L'^-T = chol(C) J as a blocked right-looking solve in fp32 on a working copy S32 in
// the free right half of A (postcov.hip): per outer panel of L', the rows' left-looking walks over
// the panel's columns (the dataflow kernel's no-wait twin, k_chol_panel_df32<true>, against the
// fp32 inverses of L''s diagonal tiles), then the rank-64*outer update of the rows' remaining
// columns on the 128x128 super-tile kernel (fp16x3 operands where h3post allows). Row tile nb + I
// of L_K J is zero before tile column nb - 1 - I (chol(C) J keeps that pattern), so a panel
// touches only the rows whose first nonzero tile lies in or before it. The fp64 route costs N^3/3
// flops per chain on the f64 MFMA; chol(C) enters the estimate only through the fp32 slot and
// L.U, and moves log f by ~1e-9 x trace(C) in fp32 (tools/postcov_precision_study.py), so chains
// with trace(C) > Sl.post_q are recomputed in fp64 after the slot write (bottom64_rerun).
MatF s32_of(apm_ctx* c) {
    return MatF{reinterpret_cast<float*>(c->A.base + c->np), 2 * c->A.ld, 2 * c->A.cstride};
}
float* d32post_of(apm_ctx* c) { return reinterpret_cast<float*>(c->Dinv + (int64_t)c->nb * 4096); }
// fp16x3 operand planes of the bottom block's trailing updates: the Newton planes' memory (free
// once the Newton loop is done: both parity buffers of a chain hold the 2 np rows of [top;
// bottom]), written per outer panel by the conversion (the top's rows below the diagonal block)
// and the bottom rows' walks, read by the quad-tile update on the same stream (stream2), so one
// buffer serves every panel. Only when every chain of the call takes fp16x3 operands there.
Planes16 post_planes_of(apm_ctx* c) {
    if (!c->planes || !c->h3post_all) return Planes16{nullptr, 0, 0, 0};
    return Planes16{c->planes, 2 * c->plane_cs, c->plane_cs, 2 * c->np};
}

// one outer panel [K, Kend) of the bottom block on stream s: the rows' walks, then the update of
// their remaining columns
void post_bottom32_steps(apm_ctx* c, int count, int K, int Kend, hipStream_t s) {
    const Live lv = live_of(c);
    const int nb = c->nb;
    MatF S = s32_of(c);
    const int64_t ds32 = 2 * c->dstride;
    const int hlim = c->h3 ? 2 * nb : 0;
    const int row0 = std::max(nb, 2 * nb - Kend);  // rows with a nonzero tile in the panel
    const Planes16 pl = Kend < nb ? post_planes_of(c) : Planes16{nullptr, 0, 0, 0};
    launch_chol_panel_bulk32(S, K, Kend - K, row0, 2 * nb, 2 * nb,
                             FusedDiag<float>{0, d32post_of(c), ds32, nullptr, 0, 0}, lv, count,
                             hlim, c->h3post, s, pl);
    if (Kend >= nb) return;
    const double fl =
        c->prof ? update_flops(row0, 2 * nb, Kend, nb, Kend - K, Gap{0, 0}) * c->live_n : 0.0;
    ProfScope ps(c, APM_PROF_POST32_OUTER, fl, s);
    if (pl.base) {  // 256x256 quad tiles from the planes (bitwise the split-while-staged kernel)
        const auto ql = quad_list(c, row0, 2 * nb, Kend, nb);
        launch_chol_update32_q256(S, K, Kend - K, ql.first, ql.second, lv, count, s, c->h3post,
                                  pl, UPD32_POST);
    } else {
        const auto sl = super_list(c, row0, 2 * nb, Kend, nb, Gap{0, 0});
        launch_chol_update32_t128(S, K, Kend - K, sl.first, sl.second, lv, count, s,
                                  FusedDiag<float>{0, nullptr, 0, nullptr, 0, 0}, hlim, c->h3post,
                                  -1, UPD32_POST);
    }
}

// The bottom block's copy once L_K J is formed, then each outer panel of the bottom on the
// low-priority stream2 as soon as the fp64 factorisation has finished that panel of L'
// (post_bottom32_panel, chol_factor's after_panel): the bottom's fp32 work fills the CUs the fp64
// in-panel steps leave idle instead of following the factorisation. Edge y2 (main -> s2): L_K J
// in BL's fp64 rows, the chains' liveness (active reset by post_cov_lk).
void post_bottom32_begin(apm_ctx* c, int count) {
    HIPC(hipEventRecord(c->ev.y2, c->stream));
    HIPC(hipStreamWaitEvent(c->stream2, c->ev.y2, 0));
    launch_post32_convert(c->A, s32_of(c), c->Dinv, c->dstride, d32post_of(c), 2 * c->dstride,
                          c->nb, c->outer, 0, 0, true, live_of(c), count, c->stream2);
}
// edge lp_panel[p] (main -> s2): the columns [K, Kend) of L' (rows K .. nb) and their diagonal
// inverses (Dinv, first half) are final; the main stream's trailing update that follows writes
// only columns >= Kend and Dinv[Kend]
void post_bottom32_panel(apm_ctx* c, int count, int K, int Kend) {
    hipEvent_t e = c->ev.lp_panel[K / c->outer];
    HIPC(hipEventRecord(e, c->stream));
    HIPC(hipStreamWaitEvent(c->stream2, e, 0));
    launch_post32_convert(c->A, s32_of(c), c->Dinv, c->dstride, d32post_of(c), 2 * c->dstride,
                          c->nb, c->outer, K, Kend, false, live_of(c), count, c->stream2,
                          Kend < c->nb ? post_planes_of(c) : Planes16{nullptr, 0, 0, 0});
    post_bottom32_steps(c, count, K, Kend, c->stream2);
}

// the guard (newton.hip k_guard_check) of the chains `lv` admits, after their slot write
void guard_check(apm_ctx* c, Live lv, int count) {
    launch_guard_check(c->ldet, c->lstride, c->nb, c->v.Kb, c->v.vstride, c->Sl, c->d_slots,
                       c->guard, c->max_batch, GUARD_T1, GUARD_T2, GUARD_T3, GUARD_T4,
                       c->guard_rows, c->v.f, APM_STATUS_GUARD, lv, count, c->stream);
}

// The fp64 bottom block for the chains flagged by the slot writer (bit 1 of Sl.chain_wide):
// (L_K J) L'^-T on the still intact fp64 rows [np, 2np) of A and L' (chol_solve_rows on those
// rows, the chains masked through active2), then their slots again in mode 2 and the u-path of
// the call again (the other chains' values are recomputed unchanged).
void bottom64_rerun(apm_ctx* c, int count, const std::vector<int>& redo) {
    const int nb = c->nb;
    for (int b = 0; b < count; ++b) c->hmask[b] = 0;
    for (int b : redo) c->hmask[b] = 1;
    HIPC(hipMemcpyAsync(c->active2, c->hmask, sizeof(int) * count, hipMemcpyHostToDevice,
                        c->stream));
    const Live lr{c->active2, c->status};
    const Exec ex{c->stream, lr, c->Dinv, c->ldet, (int)redo.size()};
    SolveOpts o;
    o.ex = &ex;
    o.gap = y_gap;
    chol_solve_rows(c, c->A, nb, /*row_start=*/nb, /*R=*/2 * nb, /*Cb=*/nb, count, o);
    launch_slot_write(c->A, c->v, c->ldet, c->lstride, nb, c->Sl, c->d_slots, 2, c->n, c->np, lr,
                      count, c->stream, MatF{nullptr, 0, 0}, c->guard_rows);
    guard_check(c, lr, count);  // (the fp64 bottom's rows now: r3, r4 were skipped before)
    c->n_post64 += (int64_t)redo.size();
}

// The reference's own route to chol(C) (estimators.py:206-215, lpa.py:107-112) for the chains
// whose C is small against K (bit 3 of Sl.chain_wide, APM_ICM_Q): C = K - V^T V with
// V = L^-1 W^1/2 K and L = chol(B) of the last Newton iteration, all fp64, as the bottom-right
// block of the factorisation of the augmented matrix [[B, .], [K W^1/2, K]] (k_form_B +
// k_form_aug, then one blocked Cholesky of 2N columns). The push-through factor the estimate uses
// cannot fail (M is SPD for any W >= 0); the reference's explicitly formed C can be numerically
// indefinite (a property of the route: it fails under 1-ulp perturbations of B at the golden ICM
// thetas and passes under them at configs[2]'s sigma = e^18.5, tools/icm_route_study.py). A chain
// whose C fails here gets APM_STATUS_CHOL_C, raised as InvalidCovarianceMatrixError (masked in
// batched calls) as the reference does. Only flagged chains pay (8N^3/3 flops each); A is free
// by now. (At the golden ICM thetas the device's chol(K) fails first: K's definiteness there is
// below its rounding)
void icm_check(apm_ctx* c, int count, const std::vector<int>& chk) {
    const int nb = c->nb;
    for (int b = 0; b < count; ++b) c->hmask[b] = 0;
    for (int b : chk) c->hmask[b] = 1;
    HIPC(hipMemcpyAsync(c->active2, c->hmask, sizeof(int) * count, hipMemcpyHostToDevice,
                        c->stream));
    const Live lr{c->active2, c->status};
    launch_form_B(c->K, c->A, c->v, c->np, lr, count, c->stream);
    launch_form_aug(c->K, c->A, c->v, c->np, lr, count, c->stream, !c->k_full);
    const Exec ex{c->stream, lr, c->Dinv, c->ldet, (int)chk.size()};
    FactorOpts o;
    o.ex = &ex;
    chol_factor(c, c->A, 0, 2 * nb, 2 * nb, 2 * nb, APM_STATUS_CHOL_C, count, o);
    c->n_icm_check += (int64_t)chk.size();
}

// L_K ready in BL (chol_k_into_bl); h = L_K^-1 f_post = L_K^T a because f_post = K a
void post_cov_lk(apm_ctx* c, int count, bool have_lk = false) {
    const Live lv = live_of(c);
    hipStream_t s = c->stream;
    HIPC(hipMemsetD32Async(c->active, 1, count, s));
    const int nb = c->nb, np = c->np;
    const int64_t vs = c->v.vstride;
    MatB TL = c->A;
    MatB BL = bl_of(c);
    if (have_lk) {
        launch_trmv_tiles(false, BL, c->v.a, c->v.z, vs, np, c->sympart, c->sstride, lv, count,
                          s);                                                 // h = L_K^T a -> z
    } else {
        launch_copy_lower(c->K, BL, np, lv, count, s);
        launch_set_rhs(c->A, 2 * (int64_t)np, np, c->v.f, vs, lv, count, s);  // f_post under K
        chol_factor(c, BL, 0, nb, nb + 1, nb, APM_STATUS_CHOL_K, count);      // L_K, h = L_K^-1 f
        launch_get_row(c->A, 2 * (int64_t)np, np, c->v.z, vs, lv, count, s);  // h -> z
        // (1/2 log|K| before M's factorisation overwrites ldet[0, nb))
        launch_guard_save(c->ldet, c->lstride, 0, nb, c->guard, c->max_batch, 1, lv, count, s);
    }
    // J M J = I + Y2 Y2^T: on the 128x128 super-tile path one launch writes it without reading TL
    // (tile column j takes Y2's column blocks k <= j); otherwise TL starts as I and receives
    // panel-wide updates (Y2 lower: j >= K suffices)
    const bool syrk1 = nb >= 2;
    launch_form_y2_rev(BL, TL, np, c->v.Ws, vs, np, lv, count, s, !syrk1);  // Y2, Y = L_K J
    // the bottom block's fp32 copy of L_K J (stream2, HBM-bound) beside the SYRK (MFMA-bound)
    // rather than beside the first panel's latency-bound in-panel steps (-1.4 ms per stationary
    // theta-call, profiles/r05_conv_early_ab.txt)
    post_bottom32_begin(c, count);
    if (syrk1) {
        tracked_update(c, TL, nb, nb, 0, nb, 0, nb, Gap{0, 0}, 2, count);
    } else {
        launch_identity_lower(TL, np, lv, count, s);
        for (int K = 0; K < nb; K += c->outer) {
            const int Kend = std::min(K + c->outer, nb);
            tracked_update(c, TL, nb + K, Kend - K, K, nb, K, nb, Gap{0, 0}, 1, count);
        }
    }
    // J M J alone in fp64 (its log-determinant is log|B|), the fp32 bottom block following its
    // panels on stream2
    FactorOpts o;
    o.after_panel = [c, count](int K, int Kend) { post_bottom32_panel(c, count, K, Kend); };
    chol_factor(c, TL, 0, nb, nb, nb, APM_STATUS_CHOL_C, count, o);
    launch_trmv_tiles(true, TL, c->v.z, c->v.Kb, vs, np, c->sympart, c->sstride, lv, count,
                      s);                                                     // g = J L'^T J h
    // edge bottom_done (s2 -> main): the slot writer reads the bottom block (S32). APM_SKEW bit 2
    // (tests only) drops this one wait, so that the skew test can show a missing edge being caught
    HIPC(hipEventRecord(c->ev.bottom_done, c->stream2));
    if (!(c->skew & 4)) HIPC(hipStreamWaitEvent(c->stream, c->ev.bottom_done, 0));
}

}  // namespace

void theta_eval_impl(apm_ctx* c, int est, int count, bool gram, double* out_logf, int* status,
                     int64_t* nops) {
    const Live lv = live_of(c);
    c->live_n = count;
    HIPC(hipMemsetD32Async(c->active, 1, count, c->stream));
    HIPC(hipMemsetAsync(c->status, 0, sizeof(int) * count, c->stream));
    HIPC(hipMemsetAsync(c->n_iter, 0, sizeof(int) * count, c->stream));
    reset_tickets(c);
    // IS: chol(K) runs on the second stream while the Newton iterations run on the main one
    const bool ov = est == APM_EST_IS && c->mixed;
    // the matrix a factorisation of K starts from (chol(K)'s working copy BL, or PriorMC's A):
    // the Gram writes K's lower tiles there too instead of a later copy pass
    MatB k2{nullptr, 0, 0};
    int k2cols = 1 << 30;
    if (gram) {
        if (est == APM_EST_PRIORMC) {
            k2 = c->A;
        } else if (ov) {
            k2 = bl_of(c);
            // chol(K)'s first trailing update can read its old tiles from K (out of place): the
            // Gram then copies only the first outer panel's tile columns (~1/4 of the lower tiles
            // at N = 4096 instead of all of them)
            if (c->outer >= 2 && c->nb - c->outer >= 2) k2cols = c->outer;
        }
    }
    if (gram) {
        // every consumer on this path reads K's lower tiles: the Gram writes N(N+1)/2 entries
        // 
        c->k_full = false;
        const double nk = 0.5 * (double)c->n * (c->n + 1);
        ProfScope ps(c, APM_PROF_GRAM, 8.0 * ((double)c->n * c->d + nk) * count + 8.0 * c->P);
        launch_gram(c->K, c->X, c->d, c->n, c->d, c->theta, c->P, c->kind, c->eps, c->np, lv,
                    count, c->stream, /*both=*/false, k2, k2cols);
    }
    std::vector<int> st_h(count, 0), it_h(count, 0);
    if (est == APM_EST_PRIORMC) {
        if (!k2.base) launch_copy_lower(c->K, c->A, c->np, lv, count, c->stream);
        chol_factor(c, c->A, 0, c->nb, c->nb, c->nb, APM_STATUS_CHOL_K, count);
        launch_slot_write(c->A, c->v, c->ldet, c->lstride, c->nb, c->Sl, c->d_slots, 1, c->n,
                          c->np, lv, count, c->stream);
        u_eval_device(c, count, true);
    } else if (est == APM_EST_IS_EP) {
        // the IS estimator around the EP fit: f_post = mu, W = tau~, z = nu~.
        // No concurrent chol(K): the sweeps keep the rows of V^T in BL, where it would factor, so
        // K is factored after the fit on the main stream (post_cov_lk without L_K). Chains whose
        // fit failed carry their status and drop out of everything below through Live.
        ep_fit(c, count, st_h);
        launch_ep_handoff(c->v, c->n, c->np, lv, count, c->stream);
        // the guard's 1/2 log|B| of the stop sweep's factor (fp64 here)
        launch_guard_save(c->ldet, c->lstride, 0, c->nb, c->guard, c->max_batch, 0, lv, count,
                          c->stream);
        post_cov_lk(c, count, false);
        launch_slot_write(c->A, c->v, c->ldet, c->lstride, c->nb, c->Sl, c->d_slots, 3, c->n,
                          c->np, lv, count, c->stream, s32_of(c), c->guard_rows);
        guard_check(c, lv, count);
        u_eval_device(c, count, true);
    } else {
        if (ov) {
            // edge gram_k (main -> s2): K and BL's first outer panel written by the Gram, the
            // chains' theta (the statuses chol(K) keeps apart: status2 / active2)
            HIPC(hipEventRecord(c->ev.gram_k, c->stream));
            HIPC(hipStreamWaitEvent(c->stream2, c->ev.gram_k, 0));
            chol_k_begin(c, count, k_exec(c, c->stream2), /*copy=*/k2.base == nullptr,
                         /*partial=*/k2cols < c->nb);
        }
        const int64_t reruns = c->n_fp64_rerun;
        if (est == APM_EST_LAPLACE) {  // log|B| of the Newton factor itself: fp64 (lpa.py:116)
            newton(c, count, st_h, false, count);
        } else {
            newton_is(c, count, st_h);
            // the guard's 1/2 log|B| of the last Newton factor (k_guard_check)
            launch_guard_save(c->ldet, c->lstride, 0, c->nb, c->guard, c->max_batch, 0, lv,
                              count, c->stream);
        }
        c->live_n = 0;
        for (int b = 0; b < count; ++b) c->live_n += st_h[b] == 0;
        if (ov) {
            drain_chol_k(c);  // what the TRSVs did not take (a no-op after an fp64 rerun)
            if (c->n_fp64_rerun != reruns)  // the fp64 Newton rerun used rows of BL: redo L_K
                chol_k_into_bl(c, count, k_exec(c, c->stream));
            // a chain whose blocked chol(K) failed is factored once more unblocked, in another
            // rounding order (chol.hip k_chol_unblocked, n <= 512: nothing is launched above
            // that) before LinAlgError is raised: at the reference's
            // InvalidCovarianceMatrixError thetas K's definiteness is decided by the rounding
            // order
            launch_chol_unblocked(c->K, bl_of(c), c->np, c->status2, APM_STATUS_CHOL_K,
                                  c->ldet + c->nb, c->lstride, count, c->stream);
            launch_merge_status(c->status, c->status2, APM_STATUS_CHOL_K, count, c->stream);
            launch_guard_save(c->ldet, c->lstride, c->nb, c->nb, c->guard, c->max_batch, 1, lv,
                              count, c->stream);  // 1/2 log|K| (chol(K) on stream2: ldet + nb)
        }
        if (est == APM_EST_LAPLACE) {
            launch_laplace_lml(c->lik, c->v, c->y, c->n, c->ldet, c->lstride, c->nb, c->out, lv,
                               count, c->stream);
        } else {
            post_cov_lk(c, count, ov);
            launch_slot_write(c->A, c->v, c->ldet, c->lstride, c->nb, c->Sl, c->d_slots,
                              3, c->n, c->np, lv, count, c->stream, s32_of(c), c->guard_rows);
            guard_check(c, lv, count);
            u_eval_device(c, count, true);
        }
    }
    std::vector<int> wide_h(count, 0);
    if (est == APM_EST_LAPLACE) {
        read_back(c, {RB{c->out, (int)sizeof(double) * count, out_logf},
                      RB{c->status, (int)sizeof(int) * count, st_h.data()},
                      RB{c->n_iter, (int)sizeof(int) * count, it_h.data()}});
    } else {
        read_back(c, {RB{c->out, (int)sizeof(double) * count, out_logf},
                      RB{c->status, (int)sizeof(int) * count, st_h.data()},
                      RB{c->n_iter, (int)sizeof(int) * count, it_h.data()},
                      RB{c->Sl.chain_wide, (int)sizeof(int) * count, wide_h.data()}});
        const int64_t* hs = pin_slots(c);  // the call's slots
        // (the follow-ups of the Laplace proposal's estimator apply to the EP proposal's alike)
        const bool is_like = est == APM_EST_IS || est == APM_EST_IS_EP;
        std::vector<int> chk;  // bit 3: the reference's route to chol(C) is checked (icm_check)
        for (int b = 0; b < count; ++b)
            if (st_h[b] == 0 && (wide_h[b] & 8) && is_like) chk.push_back(b);
        std::vector<int> redo, rewrite;  // fp32 bottom blocks above the trace bound (bit 1);
        bool attached = false;           // wide slots whose fp64 factor was not written (bit 2)
        for (int b = 0; b < count; ++b) {  // (a guard-failed chain's slot was written too)
            if (st_h[b] != 0 && st_h[b] != APM_STATUS_GUARD) continue;
            const bool rd = (wide_h[b] & 2) && is_like && st_h[b] == 0;
            if (rd) redo.push_back(b);
            if ((wide_h[b] & 4) && !c->l64_h[hs[b]]) {
                attach_l64(c, hs[b]);
                attached = true;
                if (!rd) rewrite.push_back(b);
            }
        }
        if (attached) upload_l64(c);
        if (!redo.empty()) bottom64_rerun(c, count, redo);  // (writes the wide ones' fp64 factor)
        if (!rewrite.empty()) {
            if (!redo.empty()) sync(c);  // (hmask feeds bottom64_rerun's pending copy)
            for (int b = 0; b < count; ++b) c->hmask[b] = 0;
            for (int b : rewrite) c->hmask[b] = 1;
            HIPC(hipMemcpyAsync(c->active2, c->hmask, sizeof(int) * count, hipMemcpyHostToDevice,
                                c->stream));
            launch_slot_write_L64(c->A, c->Sl, c->d_slots, est == APM_EST_PRIORMC ? 1 : 2, c->np,
                                  Live{c->active2, c->status}, count, c->stream);
        }
        if (!redo.empty() || !rewrite.empty()) {
            u_eval_device(c, count, true);
            read_back(c, {RB{c->out, (int)sizeof(double) * count, out_logf},
                          RB{c->status, (int)sizeof(int) * count, st_h.data()},
                          RB{c->Sl.chain_wide, (int)sizeof(int) * count, wide_h.data()}});
        }
        // the slots as the slot writer left them: the host mirror (slot_wide, the fp64 factor
        // attachments) follows every slot written this call, also of a chain the reference-route
        // check fails below (its slot holds a complete state that no caller reads)
        const std::vector<int> st_slot = st_h;
        if (!chk.empty()) {  // (after everything that reads A)
            icm_check(c, count, chk);
            read_back(c, {RB{c->status, (int)sizeof(int) * count, st_h.data()}});
        }
        for (int b = 0; b < count; ++b) c->n_guard += st_h[b] == APM_STATUS_GUARD;
        bool detached = false;
        for (int b = 0; b < count; ++b) {
            if (st_slot[b] != 0 && st_slot[b] != APM_STATUS_GUARD) continue;
            c->slot_wide[hs[b]] = wide_h[b] & 1;
            if (!(wide_h[b] & 1) && c->l64_h[hs[b]]) {
                detach_l64(c, hs[b]);
                detached = true;
            }
        }
        if (detached) upload_l64(c);
    }
    if (est != APM_EST_LAPLACE)  // (host bookkeeping for the block diagnostics, host_is_diag.cpp)
        for (int b = 0; b < count; ++b) c->slot_failed[pin_slots(c)[b]] = st_h[b] != 0;
    for (int b = 0; b < count; ++b) {
        status[b] = st_h[b];
        // no kernel writes c->out[b] for a failed chain: what was read back is an earlier call's
        // value at that position, which depends on the batches that ran before
        if (st_h[b] != 0) out_logf[b] = std::numeric_limits<double>::quiet_NaN();
        if (nops) {
            if (est == APM_EST_PRIORMC) nops[b] = 1;                   // estimators.py:322
            else if (est == APM_EST_LAPLACE) nops[b] = it_h[b];        // lpa.py:441-443 (i)
            else if (est == APM_EST_IS_EP) nops[b] = 2 * (int64_t)it_h[b] + 1 + 2;  // §16 + IS
            else nops[b] = (int64_t)it_h[b] + 1 + 2;                   // estimators.py:217
        }
    }
}

}  // namespace apm_host
