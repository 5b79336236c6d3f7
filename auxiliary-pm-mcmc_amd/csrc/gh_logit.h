// The logit's Gauss-Hermite average of sigma at N(mu, v) on one thread: what
// the IS predictive's link (is_predict.hip) and the cavity leave-one-out density (is_loo.hip) share.
#pragma once
#include "apm_common.h"
#include "gh_table.h"

// The logit's Gauss-Hermite average of sigma at N(mu, v): k_predict_reduce's rule (gh_table.h) and
// its sign branches, one thread instead of one wave. There lane q holds pair q and the wave's
// butterfly (xor 32, 16, .. 1) adds them; gh_tree<6>(.., 0) is that butterfly's sum tree (after k
// steps lane q holds R(k, q) = R(k-1, q) + R(k-1, q ^ (32 >> (k-1)))), so the two agree bitwise
// for the same (mu, v).
template <int K>
__device__ __forceinline__ double gh_tree(double mu, double sd, int q) {
    if constexpr (K == 0) {
        const double a = sd * APM_GH_X[q];
        const double up = sigmoid_d(mu + a);
        return APM_GH_W[q] * (mu < 0.0 ? up + sigmoid_d(mu - a) : up - sigmoid_d(a - mu));
    } else {
        return gh_tree<K - 1>(mu, sd, q) + gh_tree<K - 1>(mu, sd, q ^ (32 >> (K - 1)));
    }
}
__device__ __noinline__ double gh_logit_avg(double mu, double v) {
    static_assert(APM_GH_PAIRS == 64, "gh_tree covers 64 pairs");
    const double sd = v > 0.0 ? sqrt(2.0 * v) : 0.0;
    const double acc = gh_tree<6>(mu, sd, 0);
    return mu < 0.0 ? acc : 0.5 + acc;
}
