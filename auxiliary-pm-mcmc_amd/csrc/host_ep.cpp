// Parallel expectation propagation for the probit (ep.hip): the sweep loop. One
// sweep is the posterior from the current sites, which is the fp64 Newton iteration's algebra with
// W := tau~ and b := nu~ (newton(..., mixed = false, ...)), the rows of V^T = (K S^1/2) L^-T by
// grad_block's first pass, and the site kernel - the probit's closed form, or with the context's
// quadrature switch on the rule of DESIGN.md §27 for either likelihood; one host read of the
// per-chain flags per sweep.
#include "apm_host.h"

namespace apm_host {

void ep_buffers(apm_ctx* c) {
    if (c->ep.tau) return;
    const int64_t np = c->np, B = c->max_batch;
    double* base = dalloc<double>(c, 7 * B * np + B);
    c->ep = EpVecs{base,              base + 1 * B * np, base + 2 * B * np, base + 3 * B * np,
                   base + 4 * B * np, base + 5 * B * np, base + 6 * B * np, base + 7 * B * np,
                   dalloc<int>(c, B * np), np};
}

int ep_fit(apm_ctx* c, int count, std::vector<int>& st_h) {
    ep_buffers(c);
    const Live lv = live_of(c);
    hipStream_t s = c->stream;
    const int nb = c->nb, np = c->np;
    const int64_t vs = c->v.vstride;
    c->live_n = count;
    HIPC(hipMemsetD32Async(c->active, 1, count, s));
    HIPC(hipMemsetAsync(c->status, 0, sizeof(int) * count, s));
    HIPC(hipMemsetAsync(c->n_iter, 0, sizeof(int) * count, s));
    // tau~ = nu~ = 0 (the two vectors are neighbours; chains [0, count) of each)
    HIPC(hipMemsetAsync(c->ep.tau, 0, sizeof(double) * count * np, s));
    HIPC(hipMemsetAsync(c->ep.nu, 0, sizeof(double) * count * np, s));
    // mu_prev of the first sweep is not used by the stop rule, but it is read
    HIPC(hipMemsetAsync(c->v.f, 0, sizeof(double) * count * vs, s));
    st_h.assign(count, 0);
    std::vector<int> act(count, 1);
    const auto K_times = [&](const double* x, double* out) {
        if (c->k_full)
            launch_gemv(c->K, x, vs, out, vs, np, lv, count, s);
        else
            launch_symv(c->K, x, vs, out, vs, c->sympart, c->sstride, np, MatF{}, nullptr, 0, lv,
                        count, s, c->symv_tpw);
    };
    for (int64_t t = 0; t < c->ep_max_sweeps; ++t) {
        launch_ep_prep(c->ep, c->v, np, lv, count, s);
        K_times(c->v.b, c->v.Kb);  // K nu~
        // B = I + S^1/2 K S^1/2 with S^1/2 K nu~ as its appended row: L and L^-1 of that row
        launch_form_B(c->K, c->A, c->v, np, lv, count, s);
        chol_factor(c, c->A, 0, nb, nb + 1, nb, APM_STATUS_CHOL_B, count);
        for (int J = nb - 1; J >= 0; --J)
            launch_trsv_lt_step(c->A, J, np, c->Dinv, c->dstride, c->v.z, vs, lv, count, s);
        launch_newton_update(c->v, np, lv, count, s);  // a = nu~ - S^1/2 z
        K_times(c->v.a, c->v.fnew);                    // mu = K a
        // the rows of V^T = (K S^1/2) L^-T in A's rows [np, 2np) (grad_block's first pass)
        launch_form_aug(c->K, c->A, c->v, np, lv, count, s, /*lower_only=*/!c->k_full);
        chol_solve_rows(c, c->A, nb, /*row_start=*/nb, /*R=*/2 * nb, /*Cb=*/nb, count);
        {   // bytes: the n solved rows of np entries each (the vectors are small beside them)
            ProfScope ps(c, APM_PROF_EP_SITES, 8.0 * (double)c->n * np * c->live_n);
            if (c->ep_quad)
                launch_ep_sites_q(c->lik, c->A, c->K, c->n, nb, c->v, c->y, c->ep, c->ep_damping,
                                  lv, count, s);
            else
                launch_ep_sites(c->A, c->K, c->n, nb, c->v, c->y, c->ep, c->ep_damping, lv, count,
                                s);
        }
        launch_ep_chain(c->ep, c->v, c->n, np, c->ldet, c->lstride, nb, c->ep_tol,
                        APM_STATUS_EP_CAVITY, c->active, c->status, c->n_iter, count, s);
        read_back(c, {RB{c->active, (int)sizeof(int) * count, act.data()},
                      RB{c->status, (int)sizeof(int) * count, st_h.data()}});
        int live = 0;
        for (int b = 0; b < count; ++b) live += (act[b] != 0 && st_h[b] == 0);
        if (!live) break;
        c->live_n = live;
    }
    int ok = 0;
    for (int b = 0; b < count; ++b) {
        if (act[b] != 0 && st_h[b] == 0) st_h[b] = APM_STATUS_MAXITER;
        ok += st_h[b] == APM_STATUS_OK;
    }
    HIPC(hipMemcpyAsync(c->status, st_h.data(), sizeof(int) * count, hipMemcpyHostToDevice, s));
    HIPC(hipMemsetD32Async(c->active, 1, count, s));
    c->live_n = ok;
    return ok;
}

void ep_fit_counted(apm_ctx* c, int count, EpFit& f) {
    f.ok = ep_fit(c, count, f.st);
    f.sweeps.assign(count, 0);
    HIPC(hipMemcpyAsync(f.sweeps.data(), c->n_iter, sizeof(int) * count, hipMemcpyDeviceToHost,
                        c->stream));
}

void ep_gram_fit(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, EpFit& f) {
    upload_thetas(c, count, thetas, ldt);
    HIPC(hipMemsetD32Async(c->active, 1, count, c->stream));
    HIPC(hipMemsetAsync(c->status, 0, sizeof(int) * count, c->stream));
    c->k_full = false;
    launch_gram(c->K, c->X, c->d, c->n, c->d, c->theta, c->P, c->kind, c->eps, c->np, live_of(c),
                (int)count, c->stream, /*both=*/false);
    ep_fit_counted(c, (int)count, f);
}

void ep_fetch(apm_ctx* c, double* dst, int64_t ldo, const double* src, int64_t src_ld,
              int64_t count) {
    if (dst)
        HIPC(hipMemcpy2DAsync(dst, sizeof(double) * ldo, src, sizeof(double) * src_ld,
                              sizeof(double) * c->n, count, hipMemcpyDeviceToHost, c->stream));
}

}  // namespace apm_host
