// What follows a Laplace fit on its last fp64 Newton factor: apm_laplace's covariance, the
// predictive distribution at test inputs and the gradient of the log marginal likelihood, each
// a pass of chol_solve_rows over free rows of the work matrix; and the gradient of log Z_EP on an
// EP fit's last factor, which is the Laplace gradient's second pass.
#include <cmath>

#include "apm_host.h"

namespace apm_host {

// apm_laplace's covariance C = K - V^T V (lpa.py:111-112) in the bottom-right of A: the
// augmented matrix [[B,.],[K W^1/2, K]] with the last fp64 Newton factor in its top-left
void augmented(apm_ctx* c, int count) {
    const Live lv = live_of(c);
    HIPC(hipMemsetD32Async(c->active, 1, count, c->stream));
    launch_form_aug(c->K, c->A, c->v, c->np, lv, count, c->stream);
    const int nb = c->nb;
    chol_solve_rows(c, c->A, nb, /*row_start=*/nb, /*R=*/2 * nb + 1, /*Cb=*/2 * nb, count);
}

void covariance_out(apm_ctx* c, double* C_out, int64_t ldc) {
    const int np = c->np;
    augmented(c, 1);
    std::vector<double> Cb((size_t)np * np);
    HIPC(hipMemcpy2DAsync(Cb.data(), sizeof(double) * np, c->A.base + (int64_t)np * c->A.ld + np,
                          sizeof(double) * c->A.ld, sizeof(double) * np, np,
                          hipMemcpyDeviceToHost, c->stream));
    sync(c);
    for (int64_t i = 0; i < c->n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            C_out[i * ldc + j] = Cb[(size_t)i * np + j];
            C_out[j * ldc + i] = Cb[(size_t)i * np + j];
        }
}

void laplace_on_K(apm_ctx* c, const double* K, int64_t ldk, double* f_out, double* C_out,
                  int64_t ldc, double* lml_out, int64_t* n_iter_out, int* status) {
    std::vector<double> Kp;  // (alive until the syncs below)
    upload_padded_K(c, K, ldk, Kp);
    HIPC(hipMemsetD32Async(c->active, 1, 1, c->stream));
    HIPC(hipMemsetAsync(c->status, 0, sizeof(int), c->stream));
    HIPC(hipMemsetAsync(c->n_iter, 0, sizeof(int), c->stream));
    std::vector<int> st(1, 0);
    c->live_n = 1;
    newton(c, 1, st, false, 1);
    int it = 0;
    HIPC(hipMemcpyAsync(&it, c->n_iter, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    sync(c);
    *status = st[0];
    if (n_iter_out) *n_iter_out = it;
    if (st[0] != APM_STATUS_OK) return;
    HIPC(hipMemcpyAsync(f_out, c->v.f, sizeof(double) * c->n, hipMemcpyDeviceToHost, c->stream));
    if (lml_out) {
        launch_laplace_lml(c->lik, c->v, c->y, c->n, c->ldet, c->lstride, c->nb, c->out,
                           live_of(c), 1, c->stream);
        HIPC(hipMemcpyAsync(lml_out, c->out, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    if (C_out) covariance_out(c, C_out, ldc);
    sync(c);
}

int laplace_then_live(apm_ctx* c, int count, double* lml, int* status, int64_t* n_iter) {
    // L, inv(L_kk), W^1/2, a and the mode of each chain's last iteration stay in A / Dinv / the
    // Newton vectors
    theta_eval_impl(c, APM_EST_LAPLACE, count, true, lml, status, n_iter);
    int ok = 0;
    for (int b = 0; b < count; ++b) ok += status[b] == APM_STATUS_OK;
    if (ok) {
        // converged chains left the Newton loop with active = 0 (as augmented())
        HIPC(hipMemsetD32Async(c->active, 1, count, c->stream));
        c->live_n = ok;
    }
    return ok;
}

// Laplace predictive (predict.hip) of one block of ms <= np test inputs (packed
// ms x d in pxs: TestInputs::upload) for the chains left live by an fp64 Laplace theta-call:
// W^1/2 . k* into the free rows [np, np + 64 mb) of A and mu*'s partials, the panel solves and
// outer updates of those rows against the last Newton factor (as augmented(), without the
// bottom-right SYRK), the row reduction; outputs in pmean / pvar / pprob (row stride np).
// with_cov (the joint predictive, host_predict_joint.cpp): the trailing updates also cover the
// lower tiles of the block behind the rows, A[np.., np..] -= V V^T, as augmented()'s do.
// predict_buffers() first.
void predict_buffers(apm_ctx* c) {
    if (c->pxs) return;
    const int64_t np = c->np, B = c->max_batch;
    const bool lin = kernel_kind_of(c->kind).linear != 0;
    c->pxs = dalloc<double>(c, np * std::max(c->d, 1) + (lin ? np : 0));
    if (lin) c->pxn = c->pxs + np * std::max(c->d, 1);
    c->ppart = dalloc<double>(c, B * c->nb * np);
    c->pmean = dalloc<double>(c, 3 * B * np + (lin ? 4 : 3) * B);
    c->pvar = c->pmean + B * np;
    c->pprob = c->pvar + B * np;
    c->psig = c->pprob + B * np;
    c->pkss = c->psig + B;
    c->pbet = c->pkss + B;
    if (lin) c->plam = c->pbet + B;
}

void predict_block(apm_ctx* c, int count, int ms, bool with_cov) {
    const Live lv = live_of(c);
    const int nb = c->nb, mb = (ms + 63) / 64;
    const int64_t np = c->np;
    launch_gram_cross(c->A, np, c->pxs, ms, mb, c->X, c->d, c->n, c->d, nb, c->theta, c->P,
                      c->psig, c->pbet, c->plam, c->kind, c->v.Ws, c->v.a, c->v.vstride, c->ppart,
                      nb * np, lv, 0, count, c->stream);
    chol_solve_rows(c, c->A, nb, /*row_start=*/nb, /*R=*/nb + mb, /*Cb=*/with_cov ? nb + mb : nb,
                    count);
    launch_predict_reduce(c->lik, c->A, np, ms, mb, nb, c->pkss, c->plam, c->pxn, c->ppart,
                          nb * np, c->pmean, c->pvar, c->pprob, np, lv, count, c->stream);
}

TestInputs::TestInputs(apm_ctx* c_, int count_, const double* thetas, int64_t ldt,
                       const double* Xs_, int64_t m_, int64_t ldxs_)
    : c(c_), count(count_), Xs(Xs_), m(m_), ldxs(ldxs_), sig((size_t)(4 * c_->max_batch)) {
    predict_buffers(c);
    // [s | s + beta | beta | lambda], the layout of psig / pkss / pbet / plam (the last one for a
    // kind with the linear term only)
    const int B = c->max_batch;
    for (int b = 0; b < count; ++b) {
        sig[b] = std::exp(thetas[b * ldt]);
        sig[2 * B + b] = cov_beta(c->kind, c->P, thetas + b * ldt);
        sig[B + b] = sig[b] + sig[2 * B + b];
        sig[3 * B + b] = cov_lambda(c->kind, c->P, thetas + b * ldt);
    }
    HIPC(hipMemcpyAsync(c->psig, sig.data(), sizeof(double) * (c->plam ? 4 : 3) * B,
                        hipMemcpyHostToDevice, c->stream));
}

int TestInputs::upload(int64_t r0) {
    const int ms = (int)std::min<int64_t>(c->np, m - r0);
    xs.resize((size_t)ms * c->d + (c->pxn ? ms : 0));
    for (int i = 0; i < ms; ++i)
        for (int k = 0; k < c->d; ++k) xs[(size_t)i * c->d + k] = Xs[(r0 + i) * ldxs + k];
    HIPC(hipMemcpyAsync(c->pxs, xs.data(), sizeof(double) * ms * c->d, hipMemcpyHostToDevice,
                        c->stream));
    if (c->pxn) {  // |x*_i|^2, features in order
        double* xn = xs.data() + (size_t)ms * c->d;
        for (int i = 0; i < ms; ++i) {
            double s = 0.0;
            for (int k = 0; k < c->d; ++k) s = std::fma(xs[(size_t)i * c->d + k], xs[(size_t)i * c->d + k], s);
            xn[i] = s;
        }
        HIPC(hipMemcpyAsync(c->pxn, xn, sizeof(double) * ms, hipMemcpyHostToDevice, c->stream));
    }
    return ms;
}

void TestInputs::rows_back(int64_t r0, int ms, const int* only_ok, double* mean, double* var,
                           double* prob, int64_t ldo) {
    const std::pair<double*, const double*> outs[3] = {
        {mean, c->pmean}, {var, c->pvar}, {prob, c->pprob}};
    for (const auto& o : outs) {
        if (!o.first) continue;
        if (!only_ok) {
            HIPC(hipMemcpy2DAsync(o.first + r0, sizeof(double) * ldo, o.second,
                                  sizeof(double) * c->np, sizeof(double) * ms, count,
                                  hipMemcpyDeviceToHost, c->stream));
            continue;
        }
        for (int b = 0; b < count; ++b)
            if (only_ok[b] == APM_STATUS_OK)
                HIPC(hipMemcpyAsync(o.first + b * ldo + r0, o.second + (int64_t)b * c->np,
                                    sizeof(double) * ms, hipMemcpyDeviceToHost, c->stream));
    }
}

void predict_all(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, const double* Xs,
                 int64_t m, int64_t ldxs, double* mean, double* var, double* prob, int64_t ldo) {
    TestInputs in(c, (int)count, thetas, ldt, Xs, m, ldxs);
    for (int64_t r0 = 0; r0 < m; r0 += c->np) {
        const int ms = in.upload(r0);
        predict_block(c, (int)count, ms);
        in.rows_back(r0, ms, nullptr, mean, var, prob, ldo);
        sync(c);  // (the staged block is reused by the next one)
    }
}

// Gradient of the Laplace LML w.r.t. theta (gradient.hip) for the chains left live
// by an fp64 Laplace theta-call, in two passes over the bottom rows [np, 2np) of A against the
// last Newton factor (chol_solve_rows, as augmented() and predict_block use it):
//   1. K W^1/2 in the bottom-left (k_form_aug), panel solves -> V^T; its row norms give dS, then
//      g, s2 and t = K s2;
//   2. diag(W^1/2) in the bottom-left and zeros in the bottom-right's lower tiles, panel solves
//      and trailing updates -> Z^T and -Z^T Z = -R; q = s2 + (-R) t;
// then the fused contraction of M against dK/dtheta_j (k_grad_reduce) and the sum of its
// super-tile partials into gout (count x P). grad_buffers() first.
void grad_buffers(apm_ctx* c) {
    if (c->gvec) return;
    const int64_t np = c->np, B = c->max_batch, ns = (c->nb + 1) / 2;
    c->gvec = dalloc<double>(c, 6 * B * np);
    c->gpart = dalloc<double>(c, B * (ns * (ns + 1) / 2) * c->P);
    c->gout = dalloc<double>(c, B * c->P);
}

// The second pass and the contraction, shared by the Laplace and the EP gradient: diag(W^1/2)
// (S^1/2 for EP) from v.Ws against the factor in A / Dinv -> -R in the bottom-right's lower tiles,
// then M = 1/2 a a^T - 1/2 R + 1/2 (q g^T + g q^T) against dK/dtheta_j into gout. With t (the
// Laplace gradient's K s2) q = s2 - R t is formed between the two; without it (EP, whose M has no
// implicit term) q and g are zeroed, and k_grad_reduce's 1/2 (fma(a_i, a_k, -R_ik) + fma(0, g_k,
// 0 q_k)) is 1/2 a_i a_k - 1/2 R_ik exactly.
static void grad_contract(apm_ctx* c, int count, const double* t) {
    const Live lv = live_of(c);
    const int nb = c->nb, ns = (nb + 1) / 2, nst = ns * (ns + 1) / 2;
    const int64_t np = c->np, B = c->max_batch;
    double *g = c->gvec + B * np, *s2 = g + B * np, *u = c->gvec + 4 * B * np, *q = u + B * np;
    launch_grad_fill(c->A, c->v.Ws, c->v.vstride, nb, lv, count, c->stream);
    chol_solve_rows(c, c->A, nb, /*row_start=*/nb, /*R=*/2 * nb, /*Cb=*/2 * nb, count);
    const MatB Rn{c->A.base + np * c->A.ld + np, c->A.ld, c->A.cstride};  // -R, lower tiles
    if (t) {
        launch_symv(Rn, t, np, u, np, c->sympart, c->sstride, c->np, MatF{}, nullptr, 0, lv, count,
                    c->stream, c->symv_tpw);
        launch_grad_q(s2, u, q, np, c->n, c->np, lv, count, c->stream);
    } else {
        HIPC(hipMemsetAsync(g, 0, sizeof(double) * count * np, c->stream));
        HIPC(hipMemsetAsync(q, 0, sizeof(double) * count * np, c->stream));
    }
    {   // bytes: the lower triangles of R and K (the inputs and vectors are small beside them)
        ProfScope ps(c, APM_PROF_GRAD_REDUCE, 8.0 * (double)c->n * (c->n + 1) * c->live_n);
        launch_grad_reduce(c->K, Rn, c->X, c->d, c->n, c->d, nb, c->theta, c->P, c->kind, c->v.a,
                           c->v.vstride, q, g, np, c->gpart, (int64_t)nst * c->P, c->P, lv, count,
                           c->stream);
    }
    launch_grad_sum(c->gpart, (int64_t)nst * c->P, nst, c->P, c->gout, lv, count, c->stream);
}

void grad_block(apm_ctx* c, int count) {
    const Live lv = live_of(c);
    const int nb = c->nb;
    const int64_t np = c->np, B = c->max_batch;
    double *dS = c->gvec, *g = dS + B * np, *s2 = g + B * np, *t = s2 + B * np;
    launch_form_aug(c->K, c->A, c->v, c->np, lv, count, c->stream, /*lower_only=*/!c->k_full);
    chol_solve_rows(c, c->A, nb, /*row_start=*/nb, /*R=*/2 * nb, /*Cb=*/nb, count);
    launch_grad_rows(c->lik, c->A, c->K, c->n, nb, c->v.f, c->y, c->v.vstride, dS, g, s2, np, lv,
                     count, c->stream);
    launch_symv(c->K, s2, np, t, np, c->sympart, c->sstride, c->np, MatF{}, nullptr, 0, lv, count,
                c->stream, c->symv_tpw);
    grad_contract(c, count, t);
}

// Gradient of log Z_EP w.r.t. theta for the chains left live by ep_fit: the stop
// sweep's factor, S^1/2 (v.Ws) and a are in place and rows [np, 2np) of A (that sweep's V^T) are
// free, so this is grad_block's second pass alone. grad_buffers() first.
void ep_grad_block(apm_ctx* c, int count) { grad_contract(c, count, nullptr); }

}  // namespace apm_host
