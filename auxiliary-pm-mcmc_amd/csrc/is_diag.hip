// Replicate spread and weight diagnostics of the IS estimate: the block reduction
// that apm_u_eval_diag and apm_is_spread run after the u-path's k_ugemm, all fp64.
//
// The S = n_imp real samples of a chain's U buffer are cut into nblk = S / B blocks of B (leftover
// samples are ignored). With log w_s = cst + sum_i partial[i][s] as k_lme and k_is_weights form it
// (the row-block entries added in ascending order), per block j over s in [jB, (j+1)B):
//   logf_j = logsumexp_s log w_s - log B          (an IS estimate from B samples of its own)
//   ess_j  = (sum_s w_s)^2 / sum_s w_s^2          (w_s = exp(log w_s - max): the scale cancels)
//   wmax_j = max_s w_s / sum_s w_s = 1 / sum_s exp(log w_s - max)
// A block whose maximum is not finite is degenerate: logf_j = max - log B as k_lme returns it,
// ess_j = wmax_j = 0.
#include "apm_internal.h"

// One workgroup per (block j = blockIdx.x, chain b = blockIdx.y). Thread t takes samples t,
// t + 256, .. relative to the block start; block_max_d, then exp(v - mx) summed per thread in that
// order and block_sum_d: for B = S this is k_lme's reduction order, value for value (its first
// 1024 sums kept in LDS, the others formed again by the same ascending adds), so logf_0 is
// bitwise apm_u_eval's. Three stores per workgroup at out[q qstride + b ostride + off + j],
// q = 0 (logf), 1 (ess), 2 (wmax): no atomics. Failed chains drop out through status.
__global__ __launch_bounds__(256) void k_lme_blocks(const double* __restrict__ partial,
                                                    int64_t pstride, int nb, int B, int sp,
                                                    const double* __restrict__ cst,
                                                    const int64_t* __restrict__ slots,
                                                    double* __restrict__ out, int64_t qstride,
                                                    int64_t ostride, int64_t off,
                                                    const int* __restrict__ status) {
    const int b = blockIdx.y, j = blockIdx.x;
    if (status[b] != 0) return;
    __shared__ double red[4];
    __shared__ double lw[1024];
    const double* pb = partial + b * pstride + (int64_t)j * B;
    const double c0 = cst[slots[b]];
    double mx = -INFINITY;
    for (int t = threadIdx.x; t < B; t += 256) {
        double v = c0;
        int i = 0;
        for (; i + 16 <= nb; i += 16) {  // 16 loads in flight, added in order (as k_lme)
            double q[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) q[k] = pb[(int64_t)(i + k) * sp + t];
#pragma unroll
            for (int k = 0; k < 16; ++k) v += q[k];
        }
        for (; i < nb; ++i) v += pb[(int64_t)i * sp + t];
        if (t < 1024) lw[t] = v;
        mx = fmax(mx, v);
    }
    mx = block_max_d(mx, red);
    __syncthreads();
    double se = 0.0, s2 = 0.0;
    for (int t = threadIdx.x; t < B; t += 256) {
        double v;
        if (t < 1024) {
            v = lw[t];
        } else {
            v = c0;
            for (int i = 0; i < nb; ++i) v += pb[(int64_t)i * sp + t];
        }
        const double e = exp(v - mx);
        se += e;
        s2 = fma(e, e, s2);
    }
    se = block_sum_d(se, red);
    __syncthreads();
    s2 = block_sum_d(s2, red);
    if (threadIdx.x == 0) {
        const bool ok = isfinite(mx);
        double* o = out + b * ostride + off + j;
        o[0] = (ok ? mx + log(se) : mx) - log((double)B);
        o[qstride] = ok ? se * se / s2 : 0.0;
        o[2 * qstride] = ok ? 1.0 / se : 0.0;
    }
}

void launch_lme_blocks(const double* partial, int64_t pstride, int nb, int B, int nblk, int sp,
                       const double* cst, const int64_t* slots, double* out, int64_t qstride,
                       int64_t ostride, int64_t off, const int* status, int nchains,
                       hipStream_t s) {
    APM_LAUNCH(k_lme_blocks, dim3(nblk, nchains), dim3(256), 0, s, partial, pstride, nb, B, sp,
               cst, slots, out, qstride, ostride, off, status);
}
