// The Newton loop of laplace_approximation: the fp32 factorisation of the Newton matrix
// (chol32_panel.hip, chol32_update.hip) in the memory of the work matrix with its one-panel lookahead, the solve with
// fp64 iterative refinement, the loop itself and the IS estimator's fp64 rerun.
#include "apm_host.h"

namespace apm_host {

unsigned long long* spin_words(apm_ctx* c) {
    return c->dfprog + (size_t)c->max_batch * (c->nb + 1);
}
void reset_tickets(apm_ctx* c) {
    HIPC(hipMemsetAsync(spin_words(c) + 2, 0, sizeof(unsigned long long), c->stream));
    c->ticket_base = 0;
}

namespace {

MatF b32_of(apm_ctx* c) {
    return MatF{reinterpret_cast<float*>(c->A.base), c->np, 2 * c->A.cstride};
}
SpinCtl spin_ctl(apm_ctx* c, bool trsv) {
    unsigned long long* w = spin_words(c);
    return SpinCtl{w + 2, c->ticket_base, trsv ? w + 1 : w, trsv ? c->spin_trsv : c->spin_df};
}
void trsv32(apm_ctx* c, bool fwd, MatF F, const float* D, int64_t ds, const double* r,
            double* out, Live lv, int count) {
    c->ticket_base += (unsigned long long)launch_trsv32_mw(
        fwd, F, c->nb, D, ds, r, out, c->v.vstride, lv, count, APM_STATUS_CHOL_B,
        spin_ctl(c, true), c->stream);
}
// entries between the planes of two outer panels (apm_ctx::plane_bufs buffers: one per panel, or
// two by panel parity)
int64_t plane_step(apm_ctx* c) { return (int64_t)c->max_batch * c->plane_cs; }
Planes16 planes_of(apm_ctx* c, int K) {
    if (!c->planes || !c->h3_now) return Planes16{nullptr, 0, 0, 0};
    return Planes16{c->planes + plane_step(c) * ((K / c->outer32) % c->plane_bufs), c->plane_cs,
                    c->plane_cs / 2, c->np};
}
float* dinv32_of(apm_ctx* c) { return reinterpret_cast<float*>(c->Dinv); }

void tracked_update32(apm_ctx* c, MatF M, int k0, int kc, int i0, int R, int j0, int jend,
                      int count, int fuse_k = -1, int fail_code = 0, hipStream_t st = nullptr,
                      Planes16 pl = Planes16{nullptr, 0, 0, 0}, int jext = -1) {
    if (!st) st = c->stream;
    if (i0 < j0) i0 = j0;
    if (update_tile_count(i0, R, j0, jend) <= 0) return;
    const auto tl = tile_list(c, i0, R, j0, jend, Gap{0, 0});
    if (tl.second <= 0) return;
    FusedDiag<float> fd{0, nullptr, 0, nullptr, 0, 0};
    if (fuse_k >= 0)
        fd = FusedDiag<float>{1, dinv32_of(c), 2 * c->dstride, c->ldet, c->lstride, fail_code};
    const bool outer = kc >= 2 && jend - j0 >= 2 && (fuse_k < 0 || (i0 == fuse_k && j0 == fuse_k));
    // the Newton matrix's appended right-hand-side row tile (nb, rows < R) is updated as a row
    // vector (rhs_row_update32); with the quad tiles that row is a launch of its own
    // (k_rhs_row_update32, outside the profiled scope: the roofline's launches are the quad and
    // 128-row GEMMs)
    const int rhs = R > c->nb || jext > 0 ? c->nb : -1;
    const bool quad =
        outer && pl.base && fuse_k < 0 && c->h3_all && i0 < c->nb && jext <= 0;
    {
        const int Rg = quad ? std::min(R, c->nb) : R;
        const double fl = c->prof ? update_flops(i0, Rg, j0, jend, kc, Gap{0, 0}) * c->live_n : 0.0;
        ProfScope ps(c, APM_PROF_CHOL_UPDATE32, fl, st);
        ProfScope ps_outer(c, outer ? APM_PROF_CHOL_UPDATE32_OUTER : -1, fl, st);
        if (quad) {
            const auto ql = quad_list(c, i0, Rg, j0, jend);
            launch_chol_update32_q256(M, k0, kc, ql.first, ql.second, live_of(c), count, st,
                                      c->h3ok, pl);
        } else if (outer) {
            // jext > jend: also the right-hand-side row's columns [jend, jext)
            const auto sl = jext > jend ? super_list_ext(c, i0, R, j0, jend, rhs, jext)
                                                    : super_list(c, i0, R, j0, jend, Gap{0, 0}, rhs);
            launch_chol_update32_t128(M, k0, kc, sl.first, sl.second, live_of(c), count, st, fd,
                                      c->h3_now ? c->nb : 0, c->h3ok, rhs,
                                      pl.base ? UPD32_NEWTON_PLANES : UPD32_NEWTON, pl);
        } else {
            launch_chol_update32(M, k0, kc, tl.first, tl.second, live_of(c), count, st, fd,
                                 c->h3_now ? c->nb : 0, c->h3ok);
        }
    }
    if (quad && R > c->nb) {
        const auto sl = super_list(c, c->nb, R, j0, jend, Gap{0, 0}, rhs);
        launch_rhs_row_update32(M, k0, kc, sl.first, sl.second, live_of(c), count, st);
    }
}

// The left-looking far update of chol_range32 on stream3: the tiles of the outer panel's columns
// [j0, jend) from their diagonal down to the right-hand-side row take the contributions of the
// outer panels 0 .. p in one quad-tile launch of depth 64 * outer32 * (p + 1): one load and one
// store of each tile where the right-looking schedule has p + 1 of each. A panel one tile wide
// (the last one) takes panel p from the 64x64 kernel behind the others' quad launch, as in the
// right-looking schedule, whose far update of that column alone is too narrow for the outer
// kernels: that kernel adds the old tile last, so its tile is not the quad kernel's bit for bit.
void far_update_left32(apm_ctx* c, MatF M, int p, int j0, int jend, int fail_code, int count) {
    const int kc = c->outer32, nb = c->nb;
    const int npan = jend - j0 >= 2 ? p + 1 : p;
    if (npan > 0) {
        const auto ql = quad_list(c, j0, nb, j0, jend);
        const double fl =
            c->prof ? update_flops(j0, nb, j0, jend, kc * npan, Gap{0, 0}) * c->live_n : 0.0;
        ProfScope ps(c, APM_PROF_CHOL_UPDATE32, fl, c->stream3);
        ProfScope ps_outer(c, APM_PROF_CHOL_UPDATE32_OUTER, fl, c->stream3);
        launch_chol_update32_q256(M, 0, kc, ql.first, ql.second, live_of(c), count, c->stream3,
                                  c->h3ok, planes_of(c, 0), UPD32_NEWTON, npan, plane_step(c));
    }
    if (npan <= p)
        tracked_update32(c, M, p * kc, kc, j0, nb, j0, jend, count, -1, fail_code, c->stream3,
                         planes_of(c, p * kc));
}

// chol_factor's twin for the fp32 Newton matrix: one dataflow launch per outer panel
// (k_chol_panel_df32: the in-panel steps, fused diagonal tiles), the explicit-inverse panel for
// the chains invok allows, and the trailing update with a one-panel lookahead (the far part on
// stream3 beside the next panel's dataflow launch). The far part is left-looking where every
// chain takes the quad tiles and the batch the explicit-inverse panels (far_update_left32: behind
// panel p, the columns of panel p + 2 from panels 0 .. p), else right-looking (every column
// right of panel p + 1 from panel p). Both give the same factor bit for bit: a tile receives the
// same slices in the same order, and the right-looking schedule's stores and reloads of fp32
// between the panels are exact.
void chol_range32(apm_ctx* c, MatF M, int k0, int k1, int R, int Cb, int fail_code, int count) {
    const Live lv = live_of(c);
    const bool left = c->far_left && c->h3_now && c->h3_all && c->inv_any && c->zt && k0 == 0 &&
                      k1 == c->nb && Cb == c->nb && R == c->nb + 1 &&
                      (k1 + c->outer32 - 1) / c->outer32 <= c->plane_bufs;
    float* D = dinv32_of(c);
    const int64_t ds = 2 * c->dstride;
    bool have_diag = false;
    const unsigned long long fact = ++c->df_fact;
    int far_pending = -1;  // the panel whose far update on stream3 is not yet joined
    for (int K = k0; K < k1; K += c->outer32) {
        const int Kend = std::min(K + c->outer32, k1);
        const int p = K / c->outer32;
        if (!have_diag)
            launch_chol_diag32(M, K, D, ds, c->ldet, c->lstride, lv, fail_code, count, c->stream);
        // explicit-inverse panel for the invok chains; with every chain invok the dataflow
        // launch covers the diagonal block and the right-hand-side row only, else all rows, those
        // of the invok chains below the diagonal block returning at once
        const bool inv = c->inv_any && c->zt && Kend - K == 8 && Kend < c->nb &&
                         R <= c->nb + 1 && planes_of(c, K).base;
        const bool compact = inv && c->inv_all;
        const long tickets = launch_chol_panel_df32(
            M, K, Kend - K, compact ? Kend + (R > c->nb ? 1 : 0) : R,
            FusedDiag<float>{1, D, ds, c->ldet, c->lstride, fail_code}, lv, count,
            c->h3_now ? c->nb : 0, c->h3ok, c->dfprog, c->nb + 1,
            (fact << 16) | ((unsigned long long)p << 4), spin_ctl(c, false), c->stream,
            planes_of(c, K), compact && R > c->nb ? c->nb : -1, inv && !compact ? c->invok : nullptr);
        if (tickets < 0) throw HipError{"dataflow Newton panel wider than 14 tiles"};
        c->ticket_base += (unsigned long long)tickets;
        if (inv) {  // the rows below the diagonal block: X_i = A_i inv(L_D)^T
            const int64_t zcs = 2 * 16 * 512 * 32;
            launch_panel_inv32(M, K, c->nb, D, ds, c->zt, 3 * 512 * 512,
                               Planes16{c->zplanes, zcs, zcs / 2, 512}, planes_of(c, K), lv,
                               count, c->invok, c->stream);
        }
        have_diag = Kend < k1;
        const int Knext = std::min(Kend + c->outer32, Cb);
        if (Knext < Cb) {
            // the next panel's columns first (narrow, with the fused diagonal tile), its dataflow
            // launch next on this stream, and the far update on stream3 beside it (right-looking:
            // the rest of panel p's trailing update, columns >= Knext; left-looking: the columns
            // of panel p + 2 from panels 0 .. p). Edge df[p] (main -> s3): panel p's columns,
            // planes and the previous narrow update are final (and so are the earlier panels').
            // The narrow update shares its tiles with the previous panel's far update: edge
            // far[p-1] (s3 -> main) orders it behind that.
            HIPC(hipEventRecord(c->ev.df[p], c->stream));
            if (far_pending >= 0) HIPC(hipStreamWaitEvent(c->stream, c->ev.far[far_pending], 0));
            // (the right-hand-side row's far columns go with the narrow update on this stream)
            tracked_update32(c, M, K, Kend - K, Kend, R, Kend, Knext, count,
                             have_diag ? Kend : -1, fail_code, nullptr, planes_of(c, K),
                             R > c->nb ? Cb : -1);
            HIPC(hipStreamWaitEvent(c->stream3, c->ev.df[p], 0));
            if (left)
                far_update_left32(c, M, p, Knext, std::min(Knext + c->outer32, Cb), fail_code,
                                  count);
            else
                tracked_update32(c, M, K, Kend - K, Knext, std::min(R, c->nb), Knext, Cb, count,
                                 -1, fail_code, c->stream3, planes_of(c, K));
            HIPC(hipEventRecord(c->ev.far[p], c->stream3));
            far_pending = p;
            continue;
        }
        if (far_pending >= 0) {  // (the previous far update shares these tiles)
            HIPC(hipStreamWaitEvent(c->stream, c->ev.far[far_pending], 0));
            far_pending = -1;
        }
        tracked_update32(c, M, K, Kend - K, Kend, R, Kend, Cb, count, have_diag ? Kend : -1,
                         fail_code, nullptr, planes_of(c, K));
    }
    if (far_pending >= 0) HIPC(hipStreamWaitEvent(c->stream, c->ev.far[far_pending], 0));
}

// B x = W^1/2 K b with the fp32 factor (its forward solve is the appended row np) and n_refine
// steps of fp64 iterative refinement; x -> v.z (newton_solve.hip)
void newton_solve32(apm_ctx* c, int count) {
    const Live lv = live_of(c);
    hipStream_t s = c->stream;
    const int nb = c->nb, np = c->np;
    const int64_t vs = c->v.vstride, ds = 2 * c->dstride;
    MatF F = b32_of(c);
    float* D = dinv32_of(c);
    double *r1 = c->rvec, *r2 = c->rvec + c->max_batch * vs, *r3 = c->rvec + 2 * c->max_batch * vs;
    chol_range32(c, F, 0, nb, nb + 1, nb, APM_STATUS_CHOL_B, count);  // B32 formed with K b
    launch_row32(F, np, np, r1, vs, lv, count, s);  // y0 = L^-1 rhs (fp32)
    const bool mw_trsv = trsv32_mw_ok(np);
    if (mw_trsv) {
        feed_chol_k(c);
        trsv32(c, false, F, D, ds, r1, c->v.z, lv, count);
    } else {
        for (int J = nb - 1; J >= 0; --J)
            launch_trsv_bwd32(F, J, D, ds, r1, c->v.z, vs, lv, count, s);
    }
    // fp64 iterative refinement against B = I + W^1/2 K W^1/2, adaptive per chain: a chain
    // leaves after the step its correction passes k_refine_check; one host read of the mask per
    // step decides whether another step is launched (usually one step suffices at N=4096)
    if (c->n_refine > 0) launch_refine_mask(lv, c->refining, count, s);
    const Live lr{c->refining, c->status};
    std::vector<int> ref_h(count);
    for (int it = 0; it < c->n_refine; ++it) {
        launch_refine(0, c->v.Ws, c->v.Kb, c->v.z, nullptr, r2, vs, np, lr, count, s);  // t
        launch_symv(c->K, r2, vs, r3, vs, c->sympart, c->sstride, np, MatF{}, nullptr, 0, lr,
                    count, s, c->symv_tpw);  // K t
        launch_refine(1, c->v.Ws, c->v.Kb, c->v.z, r3, r1, vs, np, lr, count, s);       // res
        if (mw_trsv) {
            feed_chol_k(c);
            trsv32(c, true, F, D, ds, r1, r2, lr, count);
            feed_chol_k(c);
            trsv32(c, false, F, D, ds, r2, r3, lr, count);
        } else {
            for (int J = 0; J < nb; ++J)
                launch_trsv_fwd32(F, J, nb, D, ds, r1, r2, vs, lr, count, s);
            for (int J = nb - 1; J >= 0; --J)
                launch_trsv_bwd32(F, J, D, ds, r2, r3, vs, lr, count, s);
        }
        launch_refine(2, nullptr, nullptr, c->v.z, nullptr, r3, vs, np, lr, count, s);  // x += d
        const bool last = it + 1 == c->n_refine;
        launch_refine_check(c->v.z, r3, vs, np, c->refine_tol, APM_STATUS_CHOL_B, it, last,
                            c->refine_prev, c->refining, c->status, count, s);
        ++c->n_refine_steps;
        if (last) break;
        read_back(c, {RB{c->refining, (int)sizeof(int) * count, ref_h.data()}});
        bool any = false;
        for (int b = 0; b < count; ++b) any |= ref_h[b] != 0;
        if (!any) break;
    }
}

}  // namespace

// Newton loop of laplace_approximation over the live chains; host status per chain in st_h.
void newton(apm_ctx* c, int count, std::vector<int>& st_h, bool mixed, int live0) {
    const Live lv = live_of(c);
    c->live_n = live0;
    // f = 0 for the live chains only (a fallback rerun must keep the other chains' modes)
    launch_refine(3, nullptr, nullptr, nullptr, nullptr, c->v.f, c->v.vstride, c->np, lv, count,
                  c->stream);
    std::vector<int> act(count, 1);  // max_iters == 0: every chain is unconverged
    const int64_t rrow = c->np;  // Newton rhs row (extra row block below B)
    int64_t it = 0;
    for (; it < c->max_iters; ++it) {
        // the concurrent chol(K)'s panels spread over the iterations the previous call took (one
        // per iteration at the stationary states): released all at once they ran beside the first
        // two iterations and slowed them more than they gained (-2.5 ms per theta-call)
        c->cholk_quota = 1 << 30;
        if (c->newton_last > 0 && c->cholk_next >= 0 && c->cholk_next < c->nb) {
            const int left = (c->nb - c->cholk_next + c->outer - 1) / c->outer;
            const int its = std::max<int>(1, c->newton_last - (int)it);
            c->cholk_quota = (left + its - 1) / its;
        }
        launch_newton_prep(c->lik, c->v, c->y, c->n, c->np, lv, count, c->stream);
        if (mixed) {  // K b and the fp32 B (+ its right-hand side) in one pass over K's lower half
            launch_symv(c->K, c->v.b, c->v.vstride, c->v.Kb, c->v.vstride, c->sympart, c->sstride,
                        c->np, b32_of(c), c->v.Ws, c->v.vstride, lv, count, c->stream,
                        c->symv_tpw);
        } else if (c->k_full) {
            launch_gemv(c->K, c->v.b, c->v.vstride, c->v.Kb, c->v.vstride, c->np, lv, count,
                        c->stream);
        } else {
            launch_symv(c->K, c->v.b, c->v.vstride, c->v.Kb, c->v.vstride, c->sympart, c->sstride,
                        c->np, MatF{}, nullptr, 0, lv, count, c->stream, c->symv_tpw);
        }
        if (mixed) {
            newton_solve32(c, count);
        } else {
            launch_form_B(c->K, c->A, c->v, c->np, lv, count, c->stream);
            chol_factor(c, c->A, 0, c->nb, c->nb + 1, c->nb, APM_STATUS_CHOL_B, count);
            for (int J = c->nb - 1; J >= 0; --J)
                launch_trsv_lt_step(c->A, J, rrow, c->Dinv, c->dstride, c->v.z, c->v.vstride, lv,
                                    count, c->stream);
        }
        launch_newton_update(c->v, c->np, lv, count, c->stream);
        if (mixed || !c->k_full)
            launch_symv(c->K, c->v.a, c->v.vstride, c->v.fnew, c->v.vstride, c->sympart,
                        c->sstride, c->np, MatF{}, nullptr, 0, lv, count, c->stream, c->symv_tpw);
        else
            launch_gemv(c->K, c->v.a, c->v.vstride, c->v.fnew, c->v.vstride, c->np, lv, count,
                        c->stream);
        launch_newton_check(c->v, c->n, c->np, c->tol, c->active, c->status, c->n_iter, count,
                            c->stream);
        read_back(c, {RB{c->active, (int)sizeof(int) * count, act.data()},
                      RB{c->status, (int)sizeof(int) * count, st_h.data()}});
        int live = 0;
        for (int b = 0; b < count; ++b) live += (act[b] != 0 && st_h[b] == 0);
        if (!live) break;
        c->live_n = live;
    }
    if (mixed) c->newton_last = (int)std::min<int64_t>(it + 1, c->max_iters);
    c->cholk_quota = 1 << 30;
    bool changed = false;
    for (int b = 0; b < count; ++b)
        if (act[b] != 0 && st_h[b] == 0) {
            st_h[b] = APM_STATUS_MAXITER;
            changed = true;
        }
    if (changed)
        HIPC(hipMemcpyAsync(c->status, st_h.data(), sizeof(int) * count, hipMemcpyHostToDevice,
                            c->stream));
}

// Newton for the IS estimator: mixed precision, with an fp64 rerun for any chain whose fp32
// factorisation broke down (B is SPD with eigenvalues >= 1, so only for extreme theta)
void newton_is(apm_ctx* c, int count, std::vector<int>& st_h) {
    newton(c, count, st_h, c->mixed, count);
    if (!c->mixed) return;
    std::vector<int> redo;
    for (int b = 0; b < count; ++b)
        if (st_h[b] == APM_STATUS_CHOL_B) redo.push_back(b);
    if (redo.empty()) return;
    c->n_fp64_rerun += (int64_t)redo.size();
    std::vector<int> nit(count);
    HIPC(hipMemcpyAsync(nit.data(), c->n_iter, sizeof(int) * count, hipMemcpyDeviceToHost,
                        c->stream));
    sync(c);
    for (int b : redo) {
        st_h[b] = 0;
        nit[b] = 0;
    }
    HIPC(hipMemcpyAsync(c->status, st_h.data(), sizeof(int) * count, hipMemcpyHostToDevice,
                        c->stream));
    HIPC(hipMemcpyAsync(c->n_iter, nit.data(), sizeof(int) * count, hipMemcpyHostToDevice,
                        c->stream));
    // The fp64 rerun forms B and its right-hand-side row in A's rows [0, np]; row block np is
    // the first row block of BL, which the concurrent chol(K) on stream2 may still be writing:
    // let chol(K) finish first (L_K is recomputed after the rerun anyway, theta_eval_impl)
    drain_chol_k(c);
    // only the redo chains are live now: converged chains have active = 0, failed ones status != 0
    newton(c, count, st_h, false, (int)redo.size());
}

}  // namespace apm_host
