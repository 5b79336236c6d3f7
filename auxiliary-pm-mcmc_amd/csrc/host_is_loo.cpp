// Leave-one-out predictive densities from the IS samples (is_loo.hip): what
// apm_is_loo enqueues after capi.cpp's argument checks.
//
// Between the cached u-call's frame (u_call_open: apm_u_eval's launches, so out_logf is bitwise
// apm_u_eval's; u_call_close: one read-back): the log-weights from the per-sample sums in
// c->partial (k_is_logw), the product again with the reducing row-wise epilogue (k_is_row_gemm,
// its twin) and the merge of the sample tiles with the cavity density (k_is_loo_finish), all on
// the main stream without a host synchronisation. Slots and U buffers are only read.
#include "apm_host.h"

namespace apm_host {

namespace {

// the staging memory, allocated at the first call: log wbar (max_batch x sp) and ess (max_batch),
// the sample-tile partials (max_batch x 5 x np x sp / 64), the four row outputs (4 x max_batch x np)
void is_loo_buffers(apm_ctx* c) {
    if (c->loo_w) return;
    const int64_t np = c->np, B = c->max_batch, sp = c->sp;
    c->loo_w = dalloc<double>(c, B * sp + B);
    c->loo_ess = c->loo_w + B * sp;
    c->loo_part = dalloc<double>(c, B * 5 * np * (sp / 64));
    c->loo_out = dalloc<double>(c, 4 * B * np);
}

}  // namespace

void is_loo_run(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs,
                double* out_logf, double* loo, double* lpd, double* ess_loo, double* gauss,
                int64_t ldo, double* ess, int* status) {
    is_loo_buffers(c);
    hipStream_t s = c->stream;
    const int64_t np = c->np, n = c->n, q = c->max_batch * np;
    const bool wide = u_call_open(c, count, slots, ubufs);
    launch_is_logw(c->partial, c->pstride, c->nb, c->S, c->sp, c->Sl.cst, c->d_slots, c->loo_w,
                   c->loo_ess, c->status, count, s);
    launch_is_row_gemm(c->lik, /*store=*/false, c->Sl, c->d_slots, c->Up, c->d_ubufs, c->y, c->n,
                       c->np, c->loo_w, c->loo_part, c->status, count, wide, s);
    launch_is_loo_finish(c->lik, c->loo_part, np, c->sp / 64, c->n, c->Sl, c->d_slots, c->y,
                         c->loo_out, q, c->status, count, s);
    u_call_close(c, count, slots,
                 {{loo, ldo, c->loo_out, np, n},
                  {lpd, ldo, c->loo_out + q, np, n},
                  {ess_loo, ldo, c->loo_out + 2 * q, np, n},
                  {gauss, ldo, c->loo_out + 3 * q, np, n}},
                 {{ess, c->loo_ess}, {out_logf, c->out}}, status);
}

}  // namespace apm_host
