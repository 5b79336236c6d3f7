// The per-sample log weight of the IS estimate and its two reductions, written once for the
// kernels that form them from the per-sample sums k_ugemm leaves in `partial`
// (partial[i sp + s]: row block i < nb, sample s):
//   log w_s = cst + sum_i partial[i sp + s],   the row blocks added in ascending order,
// then either the log-mean-exp of a run of samples (is_lme: k_lme, and k_lme_blocks with the
// block diagnostics) or the self-normalised weights of a chain (is_self_normalise: k_is_weights
// stores wbar_s, k_is_logw stores log wbar_s). Every sum over s has one shape: a thread adds its
// samples in ascending order with stride 256, block_max_d / block_sum_d end it. The callers keep
// their own chain gate (status, or Live in the theta-call's tail) and hand over the chain's row.
//
// The sum has two forms. Both add in ascending i, in fp64 without contraction, so they give the
// same bits: they differ in the loads in flight alone. Both are kept because each is what its
// callers were measured with: is_lme is launched by every theta-call and u-call and its nb loads
// per sample are its latency (16 in flight); the weights kernels run once per diagnostic call.
#pragma once
#include "apm_common.h"

__device__ __forceinline__ double is_logw(const double* __restrict__ pb, int nb, int sp, int s,
                                          double cst) {
    double v = cst;
    for (int i = 0; i < nb; ++i) v += pb[(int64_t)i * sp + s];
    return v;
}

__device__ __forceinline__ double is_logw_ahead(const double* __restrict__ pb, int nb, int sp,
                                                int s, double cst) {
    double v = cst;
    int i = 0;
    for (; i + 16 <= nb; i += 16) {  // 16 loads in flight, added in order
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) t[q] = pb[(int64_t)(i + q) * sp + s];
#pragma unroll
        for (int q = 0; q < 16; ++q) v += t[q];
    }
    for (; i < nb; ++i) v += pb[(int64_t)i * sp + s];
    return v;
}

// One workgroup of 256 threads over the B samples pb[.. + t], t < B: thread t takes samples t,
// t + 256, ..; block_max_d, then exp(v - mx) summed per thread in that order and block_sum_d. The
// first 1024 log weights are kept in LDS, the others formed again by the same ascending adds.
//   o[0] = logsumexp_t log w_t - log B;  a maximum that is not finite is returned as it is.
// DIAG: also o[qstride] = ess = (sum w)^2 / sum w^2 and o[2 qstride] = wmax = max w / sum w =
// 1 / sum e^(log w - max), both 0 for such a degenerate run. Compile-time, so that the plain form
// carries no s2, no second reduction and no branch for them.
template <bool DIAG>
__device__ __forceinline__ void is_lme(const double* __restrict__ pb, int nb, int B, int sp,
                                       double cst, double* __restrict__ o, int64_t qstride) {
    __shared__ double red[4];
    __shared__ double lw[1024];
    double mx = -INFINITY;
    for (int t = threadIdx.x; t < B; t += 256) {
        const double v = is_logw_ahead(pb, nb, sp, t, cst);
        if (t < 1024) lw[t] = v;
        mx = fmax(mx, v);
    }
    mx = block_max_d(mx, red);
    __syncthreads();
    double se = 0.0, s2 = 0.0;
    for (int t = threadIdx.x; t < B; t += 256) {
        const double e = exp((t < 1024 ? lw[t] : is_logw(pb, nb, sp, t, cst)) - mx);
        se += e;
        if constexpr (DIAG) s2 = fma(e, e, s2);
    }
    se = block_sum_d(se, red);
    if constexpr (DIAG) {
        __syncthreads();
        s2 = block_sum_d(s2, red);
    }
    if (threadIdx.x == 0) {
        const bool ok = isfinite(mx);
        o[0] = (ok ? mx + log(se) : mx) - log((double)B);
        if constexpr (DIAG) {
            o[qstride] = ok ? se * se / s2 : 0.0;
            o[2 * qstride] = ok ? 1.0 / se : 0.0;
        }
    }
}

// One workgroup of 256 threads per chain: w[s] = log w_s, its maximum, se = sum_s e^(log w_s -
// max) over the S real samples, then per sample d = log w_s - max and
//   wbar_s = e^d / se   (LOG: log wbar_s = d - log se),
// exact zeros (LOG: -inf) for the padded columns [S, sp), and *ess = 1 / sum_s wbar_s^2 from the
// same wbar_s whichever is stored: the two forms' ess are one value bitwise. (The weights' form
// keeps e^d in w between the passes, the other forms it again from d: exp gives one value.)
template <bool LOG>
__device__ __forceinline__ void is_self_normalise(const double* __restrict__ pb, int nb, int S,
                                                  int sp, double cst, double* __restrict__ w,
                                                  double* __restrict__ ess) {
    __shared__ double red[4];
    double mx = -INFINITY;
    for (int s = threadIdx.x; s < S; s += 256) {
        const double v = is_logw(pb, nb, sp, s, cst);
        w[s] = v;
        mx = fmax(mx, v);
    }
    mx = block_max_d(mx, red);
    double se = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) {
        const double e = exp(w[s] - mx);
        if constexpr (!LOG) w[s] = e;  // (kept for the last pass; LOG needs d there: e^d again)
        se += e;
    }
    se = block_sum_d(se, red);
    const double lse = LOG ? log(se) : 0.0;
    double s2 = 0.0;
    for (int s = threadIdx.x; s < sp; s += 256) {
        double wb = 0.0, l = -INFINITY;
        if (s < S) {
            if constexpr (LOG) {
                const double d = w[s] - mx;
                wb = exp(d) / se;
                l = d - lse;
            } else {
                wb = w[s] / se;
            }
        }
        w[s] = LOG ? l : wb;
        s2 = fma(wb, wb, s2);
    }
    s2 = block_sum_d(s2, red);
    if (threadIdx.x == 0) *ess = 1.0 / s2;
}
