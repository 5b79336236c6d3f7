// Pareto-smoothed leave-one-out densities and the Pareto k-hat of the importance ratios
// (is_psis.hip): what apm_is_loo_psis enqueues after capi.cpp's argument checks.
//
// The u-path of apm_u_eval on the call's slots and U buffers (u_eval_device, so out_logf is
// bitwise apm_u_eval's), the log-weights from the per-sample sums it leaves in c->partial
// (k_is_logw, into this call's own buffer), the product again with the epilogue that stores every
// log ratio (k_psis_gemm, its twin) and one workgroup per row for the tail fit (k_psis_rows).
// Everything is enqueued on the main stream without a host synchronisation; one read-back ends
// the call. Slots, U buffers and apm_is_loo's staging memory are only read or left alone.
#include <limits>

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
    upload_idx(c, count, slots, ubufs);
    HIPC(hipMemsetAsync(c->status, 0, sizeof(int) * count, s));
    bool wide = false;
    for (int b = 0; b < count; ++b) wide |= c->slot_wide[slots[b]] != 0;
    u_eval_device(c, count, wide);  // apm_u_eval's launches, k_lme included
    launch_is_logw(c->partial, c->pstride, c->nb, c->S, c->sp, c->Sl.cst, c->d_slots, c->psis_w,
                   c->psis_w + B * sp, c->status, count, s);
    launch_psis_gemm(c->lik, c->Sl, c->d_slots, c->Up, c->d_ubufs, c->y, c->n, c->np, c->psis_w,
                     c->psis_t, c->status, count, wide, s);
    launch_psis_rows(c->psis_t, np * sp, c->sp, c->psis_w, c->S, c->n, c->psis_out, np, B * np, kw,
                     c->status, count, s);
    double* const rows[2] = {loo_psis, khat};
    for (int q = 0; q < 2; ++q)
        if (rows[q])
            HIPC(hipMemcpy2DAsync(rows[q], sizeof(double) * ldo, c->psis_out + q * B * np,
                                  sizeof(double) * np, sizeof(double) * n, count,
                                  hipMemcpyDeviceToHost, s));
    if (logratio)  // the real columns of the rows < n, chain by chain
        for (int b = 0; b < count; ++b)
            HIPC(hipMemcpy2DAsync(logratio + b * ldr, sizeof(double) * S, c->psis_t + b * np * sp,
                                  sizeof(double) * sp, sizeof(double) * S, n,
                                  hipMemcpyDeviceToHost, s));
    if (khat_w) HIPC(hipMemcpyAsync(khat_w, kw, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    if (out_logf)
        HIPC(hipMemcpyAsync(out_logf, c->out, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(status, c->status, sizeof(int) * count, hipMemcpyDeviceToHost, s));
    sync(c);
    // a slot whose last theta-call failed was never written: its values mean nothing
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int b = 0; b < count; ++b)
        if (status[b] != 0 || c->slot_failed[slots[b]]) {
            for (double* o : rows)
                if (o) std::fill(o + b * ldo, o + b * ldo + n, nan);
            if (logratio) std::fill(logratio + b * ldr, logratio + b * ldr + n * S, nan);
            if (khat_w) khat_w[b] = nan;
            if (out_logf) out_logf[b] = nan;
        }
}

}  // namespace apm_host
