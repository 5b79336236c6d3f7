// Replicate spread and weight diagnostics of the IS estimate (is_diag.hip): what
// apm_u_eval_diag and apm_is_spread enqueue after capi.cpp's argument checks.
//
// Both run the u-path of apm_u_eval on the call's slots and U buffers (k_ugemm, its f64 twin for
// wide slots) and then k_lme_blocks on the per-sample sums it leaves in c->partial. apm_is_spread
// does so n_rep times, each time after k_u_normal has redrawn the U buffers from the Philox
// stream (seed, counter + r): every replicate is enqueued on the main stream without a host
// synchronisation, the block values collect in the staging array, and one read-back ends the call
// (the cached u-call's frame: u_call_open without the launches, u_call_close).
#include "apm_host.h"

namespace apm_host {

namespace {

// the staging memory, allocated at the first call: three quantities x max_batch chains x
// APM_SPREAD_MAX_BLOCKS values, and the Philox keys [seeds: B][counters: APM_SPREAD_MAX_BLOCKS x B]
void is_diag_buffers(apm_ctx* c) {
    if (c->sd_out) return;
    const int64_t B = c->max_batch;
    c->sd_keys = dalloc<uint64_t>(c, B * (1 + APM_SPREAD_MAX_BLOCKS));
    c->sd_out = dalloc<double>(c, 3 * B * APM_SPREAD_MAX_BLOCKS);
}

}  // namespace

void is_diag_run(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs,
                 const uint64_t* seeds, const uint64_t* counters, int64_t n_rep, int64_t block,
                 double* logf, double* ess, double* wmax, int64_t ldo, int* status) {
    is_diag_buffers(c);
    hipStream_t s = c->stream;
    const int64_t B = c->max_batch, cap = APM_SPREAD_MAX_BLOCKS;
    const int nblk = (int)(c->S / block);
    const int64_t tot = n_rep * nblk;  // values per chain and quantity (<= cap: checked)
    // (the u-path is launched per replicate below, after the redraw where there is one)
    const bool wide = u_call_open(c, count, slots, ubufs, /*eval=*/false);
    std::vector<uint64_t> keys;  // (alive until the sync below)
    if (seeds) {
        keys.resize((size_t)(B + n_rep * count));
        for (int b = 0; b < count; ++b) keys[b] = seeds[b];
        for (int64_t r = 0; r < n_rep; ++r)
            for (int b = 0; b < count; ++b) keys[B + r * count + b] = counters[b] + (uint64_t)r;
        HIPC(hipMemcpyAsync(c->sd_keys, keys.data(), sizeof(uint64_t) * keys.size(),
                            hipMemcpyHostToDevice, s));
    }
    for (int64_t r = 0; r < n_rep; ++r) {
        if (seeds) {
            launch_u_normal(c->Up, c->d_ubufs, c->sd_keys, c->sd_keys + B + r * count, c->n, c->S,
                            count, s);
            ProfScope ps(c, APM_PROF_UGEMM, (double)c->n * (c->n + 1) * c->S * count);
            launch_ugemm(c->lik, c->Sl, c->d_slots, c->Up, c->d_ubufs, c->y, c->n, c->np,
                         c->partial, c->pstride, c->status, count, wide, s);
        } else {
            u_eval_device(c, count, wide);  // apm_u_eval's launches, k_lme included
        }
        launch_lme_blocks(c->partial, c->pstride, c->nb, (int)block, nblk, c->sp, c->Sl.cst,
                          c->d_slots, c->sd_out, B * cap, cap, r * nblk, c->status, count, s);
    }
    u_call_close(c, count, slots,
                 {{logf, ldo, c->sd_out, cap, tot}, {ess, ldo, c->sd_out + B * cap, cap, tot},
                  {wmax, ldo, c->sd_out + 2 * B * cap, cap, tot}},
                 {}, status);
}

}  // namespace apm_host
