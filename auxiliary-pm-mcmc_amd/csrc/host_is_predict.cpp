// The importance-sampling predictive distribution at test inputs (is_predict.hip):
// the fp64 tail that follows an IS theta-call (Laplace or EP proposal) on the same context.
//
// The theta-call itself is apm_theta_eval's, untouched; what it leaves behind and the tail reads:
// K's lower tiles (c->K), f_post's a = K^-1 f_post (v.a) and W^1/2 (v.Ws), the per-sample sums of
// log w_s (c->partial, k_ugemm's output that k_lme reduced into out_logf), the slot's cst, the U
// buffers. The work matrix A is free by then, and none of its contents is trusted: on the
// mixed-precision path L_K's rows were reversed in place (k_form_y2_rev), an fp64 rerun of the
// bottom block (bottom64_rerun) or the reference-route check (icm_check) may have overwritten
// them and L', so both factors are formed again, in fp64, as post_cov_lk forms them:
//   TL <- L_K = chol(K);   TR <- L' = chol(J M J),  J M J = I + Y2 Y2^T  (Y2 in BR, M built in BL)
// with TL / TR / BL / BR the np x np quadrants of A. Each block of <= np test rows then takes
//   BL rows <- k*^T (k_gram_cross against a vector of ones, which also sums c = k* . a)
//   BL rows <- p^T = k*^T L_K^-T               (chol_solve_rows against TL)
//   BR rows <- p^T J, v* = s - |p|^2           (k_is_rows)
//   BR rows <- (J h)^T = p^T J L'^-T           (chol_solve_rows against TR, the second halves of
//                                               Dinv / ldet)
//   the GEMM with the reversed U^T, the link and the weighted reduction (k_is_pred_gemm), the sum
//   of the sample tiles (k_is_finish).
#include "apm_host.h"

namespace apm_host {

namespace {

void is_predict_buffers(apm_ctx* c) {
    if (c->is_ut) return;
    const int64_t np = c->np, B = c->max_batch, sp = c->sp;
    c->is_ut = dalloc<double>(c, B * sp * np);
    c->is_w = dalloc<double>(c, B * sp + B);
    c->is_ess = c->is_w + B * sp;
    c->is_vstar = dalloc<double>(c, 3 * B * np);
    c->is_c = c->is_vstar + B * np;
    c->is_ones = c->is_c + B * np;
    c->is_part = dalloc<double>(c, B * 3 * np * (sp / 64));
    std::vector<double> ones((size_t)(B * np), 1.0);
    HIPC(hipMemcpy(c->is_ones, ones.data(), sizeof(double) * B * np, hipMemcpyHostToDevice));
}

}  // namespace

void is_predict_tail(apm_ctx* c, int count, const double* thetas, int64_t ldt, int* st_h,
                     const double* Xs, int64_t m, int64_t ldxs, double* prob, double* mean,
                     double* var, int64_t ldo, double* ess) {
    is_predict_buffers(c);
    const Live lv = live_of(c);
    hipStream_t s = c->stream;
    const int nb = c->nb, np = c->np, nst = c->sp / 64;
    const int64_t vs = c->v.vstride;
    // the chains the theta-call left OK are live again (device status: the call's final one)
    HIPC(hipMemsetD32Async(c->active, 1, count, s));
    c->live_n = 0;
    for (int b = 0; b < count; ++b) c->live_n += st_h[b] == APM_STATUS_OK;

    TestInputs in(c, count, thetas, ldt, Xs, m, ldxs);  // (alive until the blocks' syncs)

    launch_is_weights(c->partial, c->pstride, nb, c->S, c->sp, c->Sl.cst, c->d_slots, c->is_w,
                      c->is_ess, lv, count, s);
    launch_is_ut(c->Up, c->d_ubufs, np, c->is_ut, lv, count, s);

    const MatB TL = c->A;
    const MatB TR{c->A.base + np, c->A.ld, c->A.cstride};
    const MatB BL{c->A.base + (int64_t)np * c->A.ld, c->A.ld, c->A.cstride};
    // L' works with the second halves of Dinv / ldet (as the theta-call's concurrent chol(K))
    const Exec ex2{s, lv, c->Dinv + (int64_t)nb * 4096, c->ldet + nb, c->live_n};
    launch_copy_lower(c->K, TL, np, lv, count, s);
    chol_factor(c, TL, 0, nb, nb, nb, APM_STATUS_CHOL_K, count);
    // J M J = I + Y2 Y2^T in BL from a copy of L_K in TR (k_form_y2_rev reverses it in place), as
    // post_cov_lk forms it in TL; then into TR, factored there
    launch_copy_lower(TL, TR, np, lv, count, s);
    const bool syrk1 = nb >= 2;
    launch_form_y2_rev(TR, BL, np, c->v.Ws, vs, np, lv, count, s, !syrk1);
    if (syrk1) {
        tracked_update(c, BL, nb, nb, 0, nb, 0, nb, Gap{0, 0}, 2, count);
    } else {
        launch_identity_lower(BL, np, lv, count, s);
        for (int K = 0; K < nb; K += c->outer) {
            const int Kend = std::min(K + c->outer, nb);
            tracked_update(c, BL, nb + K, Kend - K, K, nb, K, nb, Gap{0, 0}, 1, count);
        }
    }
    launch_copy_lower(BL, TR, np, lv, count, s);
    FactorOpts fo;
    fo.ex = &ex2;
    chol_factor(c, TR, 0, nb, nb, nb, APM_STATUS_CHOL_C, count, fo);
    SolveOpts so;
    so.ex = &ex2;

    for (int64_t r0 = 0; r0 < m; r0 += np) {
        const int ms = in.upload(r0), mb = (ms + 63) / 64;
        launch_gram_cross(c->A, np, c->pxs, ms, mb, c->X, c->d, c->n, c->d, nb, c->theta, c->P,
                          c->psig, c->pbet, c->plam, c->kind, c->is_ones, c->v.a, vs, c->ppart,
                          (int64_t)nb * np, lv, 0, count, s);
        chol_solve_rows(c, TL, nb, /*row_start=*/nb, /*R=*/nb + mb, /*Cb=*/nb, count);
        launch_is_rows(c->A, np, ms, mb, nb, c->pkss, c->plam, c->pxn, c->ppart, (int64_t)nb * np,
                       c->is_vstar,
                       c->is_c, np, lv, count, s);
        chol_solve_rows(c, TR, nb, /*row_start=*/nb, /*R=*/nb + mb, /*Cb=*/nb, count, so);
        launch_is_pred_gemm(c->lik, c->A, np, np, np, mb, c->is_ut, c->sp, c->is_w, c->is_vstar,
                            c->is_c, np, c->is_part, np, lv, count, s);
        launch_is_finish(c->is_part, np, nst, ms, c->is_vstar, c->pmean, c->pvar, c->pprob, np, lv,
                         count, s);
        in.rows_back(r0, ms, st_h, mean, var, prob, ldo);
        sync(c);  // (the staged block is reused by the next one)
    }
    std::vector<int> st2((size_t)count);
    std::vector<double> ess_h((size_t)count);
    HIPC(hipMemcpyAsync(st2.data(), c->status, sizeof(int) * count, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(ess_h.data(), c->is_ess, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    sync(c);
    for (int b = 0; b < count; ++b) {
        if (st_h[b] == APM_STATUS_OK && st2[b] != 0) st_h[b] = st2[b];
        if (ess && st_h[b] == APM_STATUS_OK) ess[b] = ess_h[b];
    }
}

}  // namespace apm_host
