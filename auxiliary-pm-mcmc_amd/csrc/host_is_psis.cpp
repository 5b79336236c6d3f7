// Pareto-smoothed leave-one-out densities and the Pareto k-hat of the importance ratios
// (is_psis.hip): what apm_is_loo_psis enqueues after capi.cpp's argument checks.
//
// Between the cached u-call's frame (u_call_open: apm_u_eval's launches, so out_logf is bitwise
// apm_u_eval's; u_call_close: one read-back): the log-weights from the per-sample sums in
// c->partial (k_is_logw, into this call's own buffer), the product again with the epilogue that
// stores every log ratio (k_is_row_gemm, its twin) and one workgroup per row for the tail fit
// (k_psis_rows), all on the main stream without a host synchronisation. Slots, U buffers and
// apm_is_loo's staging memory are only read or left alone.
#include "apm_host.h"

namespace apm_host {

namespace {

// the staging memory, one allocation at the first call, so that a failed hipMalloc (the log ratios
// are max_batch x np x sp doubles) leaves every pointer null and a later call starts afresh: the
// log ratios, then log wbar (max_batch x sp) with k_is_logw's ess behind it, then the two row
// outputs with khat_w behind them
void is_psis_buffers(apm_ctx* c) {
    if (c->psis_t) return;
    const int64_t np = c->np, B = c->max_batch, sp = c->sp;
    double* base = dalloc<double>(c, B * np * sp + (B * sp + B) + (2 * B * np + B));
    c->psis_w = base + B * np * sp;
    c->psis_out = c->psis_w + B * sp + B;
    c->psis_t = base;
}

}  // namespace

void is_psis_run(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs,
                 double* out_logf, double* loo_psis, double* khat, int64_t ldo, double* khat_w,
                 double* logratio, int64_t ldr, int* status) {
    is_psis_buffers(c);
    hipStream_t s = c->stream;
    const int64_t B = c->max_batch, np = c->np, sp = c->sp, n = c->n, S = c->S;
    double* const kw = c->psis_out + 2 * B * np;
    const bool wide = u_call_open(c, count, slots, ubufs);
    launch_is_logw(c->partial, c->pstride, c->nb, c->S, c->sp, c->Sl.cst, c->d_slots, c->psis_w,
                   c->psis_w + B * sp, c->status, count, s);
    launch_is_row_gemm(c->lik, /*store=*/true, c->Sl, c->d_slots, c->Up, c->d_ubufs, c->y, c->n,
                       c->np, c->psis_w, c->psis_t, c->status, count, wide, s);
    launch_psis_rows(c->psis_t, np * sp, c->sp, c->psis_w, c->S, c->n, c->psis_out, np, B * np, kw,
                     c->status, count, s);
    if (logratio)  // the real columns of the rows < n, chain by chain: the frame only NaN-fills it
        for (int b = 0; b < count; ++b)
            HIPC(hipMemcpy2DAsync(logratio + b * ldr, sizeof(double) * S, c->psis_t + b * np * sp,
                                  sizeof(double) * sp, sizeof(double) * S, n,
                                  hipMemcpyDeviceToHost, s));
    u_call_close(c, count, slots,
                 {{loo_psis, ldo, c->psis_out, np, n}, {khat, ldo, c->psis_out + B * np, np, n},
                  {logratio, ldr, nullptr, 0, n * S}},
                 {{khat_w, kw}, {out_logf, c->out}}, status);
}

}  // namespace apm_host
