// Replicate spread and weight diagnostics of the IS estimate: the block reduction
// that apm_u_eval_diag and apm_is_spread run after the u-path's k_ugemm, all fp64.
//
// The S = n_imp real samples of a chain's U buffer are cut into nblk = S / B blocks of B (leftover
// samples are ignored). With log w_s = cst + sum_i partial[i][s] (is_weights.h: the row-block
// entries added in ascending order), per block j over s in [jB, (j+1)B):
//   logf_j = logsumexp_s log w_s - log B          (an IS estimate from B samples of its own)
//   ess_j  = (sum_s w_s)^2 / sum_s w_s^2          (w_s = exp(log w_s - max): the scale cancels)
//   wmax_j = max_s w_s / sum_s w_s = 1 / sum_s exp(log w_s - max)
// A block whose maximum is not finite is degenerate: logf_j = max - log B as k_lme returns it,
// ess_j = wmax_j = 0.
#include "apm_internal.h"
#include "is_weights.h"

// One workgroup per (block j = blockIdx.x, chain b = blockIdx.y): is_weights.h's is_lme with the
// diagnostics on the block's B samples. Its plain form is k_lme, so for B = S logf_0 is bitwise
// apm_u_eval's. Three stores per workgroup at out[q qstride + b ostride + off + j], q = 0 (logf),
// 1 (ess), 2 (wmax): no atomics. Failed chains drop out through status.
__global__ __launch_bounds__(256) void k_lme_blocks(const double* __restrict__ partial,
                                                    int64_t pstride, int nb, int B, int sp,
                                                    const double* __restrict__ cst,
                                                    const int64_t* __restrict__ slots,
                                                    double* __restrict__ out, int64_t qstride,
                                                    int64_t ostride, int64_t off,
                                                    const int* __restrict__ status) {
    const int b = blockIdx.y, j = blockIdx.x;
    if (status[b] != 0) return;
    is_lme<true>(partial + b * pstride + (int64_t)j * B, nb, B, sp, cst[slots[b]],
                 out + b * ostride + off + j, qstride);
}

void launch_lme_blocks(const double* partial, int64_t pstride, int nb, int B, int nblk, int sp,
                       const double* cst, const int64_t* slots, double* out, int64_t qstride,
                       int64_t ostride, int64_t off, const int* status, int nchains,
                       hipStream_t s) {
    APM_LAUNCH(k_lme_blocks, dim3(nblk, nchains), dim3(256), 0, s, partial, pstride, nb, B, sp,
               cst, slots, out, qstride, ostride, off, status);
}
