// Leave-one-out predictive densities from the IS samples (is_loo.hip): what
// apm_is_loo enqueues after capi.cpp's argument checks.
//
// The u-path of apm_u_eval on the call's slots and U buffers (u_eval_device: k_ugemm, its f64 twin
// for wide slots, k_lme - so out_logf is bitwise apm_u_eval's), then the log-weights from the
// per-sample sums it leaves in c->partial (k_is_logw), the product again with the row-wise
// epilogue (k_is_loo_gemm, its twin) and the merge of the sample tiles with the cavity density
// (k_is_loo_finish). Everything is enqueued on the main stream without a host synchronisation;
// one read-back ends the call. Slots and U buffers are only read.
#include <limits>

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
    const int64_t B = c->max_batch, np = c->np;
    upload_idx(c, count, slots, ubufs);
    HIPC(hipMemsetAsync(c->status, 0, sizeof(int) * count, s));
    bool wide = false;
    for (int b = 0; b < count; ++b) wide |= c->slot_wide[slots[b]] != 0;
    u_eval_device(c, count, wide);  // apm_u_eval's launches, k_lme included
    launch_is_logw(c->partial, c->pstride, c->nb, c->S, c->sp, c->Sl.cst, c->d_slots, c->loo_w,
                   c->loo_ess, c->status, count, s);
    launch_is_loo_gemm(c->lik, c->Sl, c->d_slots, c->Up, c->d_ubufs, c->y, c->n, c->np, c->loo_w,
                       c->loo_part, c->status, count, wide, s);
    launch_is_loo_finish(c->lik, c->loo_part, np, c->sp / 64, c->n, c->Sl, c->d_slots, c->y,
                         c->loo_out, B * np, c->status, count, s);
    double* const rows[4] = {loo, lpd, ess_loo, gauss};
    for (int q = 0; q < 4; ++q)
        if (rows[q])
            HIPC(hipMemcpy2DAsync(rows[q], sizeof(double) * ldo, c->loo_out + q * B * np,
                                  sizeof(double) * np, sizeof(double) * c->n, count,
                                  hipMemcpyDeviceToHost, s));
    if (ess)
        HIPC(hipMemcpyAsync(ess, c->loo_ess, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    if (out_logf)
        HIPC(hipMemcpyAsync(out_logf, c->out, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(status, c->status, sizeof(int) * count, hipMemcpyDeviceToHost, s));
    sync(c);
    // a slot whose last theta-call failed was never written: its values mean nothing
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int b = 0; b < count; ++b)
        if (status[b] != 0 || c->slot_failed[slots[b]]) {
            for (double* o : rows)
                if (o) std::fill(o + b * ldo, o + b * ldo + c->n, nan);
            if (ess) ess[b] = nan;
            if (out_logf) out_logf[b] = nan;
        }
}

}  // namespace apm_host
