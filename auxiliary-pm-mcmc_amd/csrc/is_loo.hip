// Leave-one-out predictive densities at the training points from the importance samples
// (DESIGN.md §23): the kernels that host_is_loo.cpp runs after the u-path of apm_u_eval.
//
// With the samples f_s = f_post + C_chol u_s of a chain's U buffer, their self-normalised weights
// wbar_s (the summands of the IS estimate, ugemm.hip's log w_s) and p_si = p(y_i | f_si):
//   loo_i     = -log sum_s wbar_s / p_si         (p(y_i | y_-i) = 1 / E[1 / p(y_i | f_i) | y])
//   lpd_i     =  log sum_s wbar_s p_si
//   ess_loo_i = (sum_s rho_si)^2 / sum_s rho_si^2,  rho_si = wbar_s / p_si
// The product is the u-path's own (k_ugemm / k_ugemm64), reduced the other way round: over the
// samples per row, once the weights are known. Every sum over s is a (max, scaled sum) pair in log
// space: 1 / p_si reaches 1e300 for a badly fitted sample, and log wbar_s = -inf (a padded column,
// a weight that underflowed) adds exactly nothing.
#include "apm_internal.h"
#include "gh_logit.h"
#include "is_weights.h"
#include "ugemm_tile.h"

// e^(t - m), exactly 0 for t = -inf whatever m is (m = -inf too where every t is)
__device__ __forceinline__ double loo_scaled(double t, double m) {
    return t == -INFINITY ? 0.0 : exp(t - m);
}

// ------------------------------------------------------------------------------- log weights
// log wbar_s of the S real samples, -inf for the padded columns [S, sp), and ess = 1 / sum
// wbar_s^2: is_weights.h's is_self_normalise, storing the logarithms (k_is_weights stores the
// weights; ess is one value). Failed chains drop out through status, as in k_lme.
__global__ __launch_bounds__(256) void k_is_logw(const double* __restrict__ partial,
                                                 int64_t pstride, int nb, int S, int sp,
                                                 const double* __restrict__ cst,
                                                 const int64_t* __restrict__ slots,
                                                 double* __restrict__ logw,
                                                 double* __restrict__ ess,
                                                 const int* __restrict__ status) {
    const int b = blockIdx.x;
    if (status[b] != 0) return;
    is_self_normalise<true>(partial + b * pstride, nb, S, sp, cst[slots[b]],
                            logw + (int64_t)b * sp, ess + b);
}

void launch_is_logw(const double* partial, int64_t pstride, int nb, int S, int sp,
                    const double* cst, const int64_t* slots, double* logw, double* ess,
                    const int* status, int nchains, hipStream_t s) {
    APM_LAUNCH(k_is_logw, dim3(nchains), dim3(256), 0, s, partial, pstride, nb, S, sp, cst, slots,
               logw, ess, status);
}

// ------------------------------------------------------------------------------- the epilogue
// Of workgroup (chain b, row block row0 / 64, sample tile sb), on its 64 x 64 tile of f = f_post +
// C_chol U held as the 2 x 2 blocks of 16 x 16 of an MFMA accumulator (f[bi][bj][r]: tile row
// rl = 32 wr + 16 bi + ROW(lane, r), tile column 32 wc + 16 bj + (lane & 15)). Per accumulator row
// of the lane and its two columns: lp = log p(y | f) as the weights' own epilogue takes it
// (lik_logp_mixed) and the log ratio t = log wbar - lp; a sample without weight has no t: -inf
// whatever its lp is. What becomes of t is chosen at compile time.
//
// lwt: the tile's 64 entries of log wbar; ob: the chain's part of the output (is_row_out below).
//
// STORE (apm_is_loo_psis): every t of the rows < n at ob[row ld + column], ld = sp, the 16 lanes
// of a row writing 16 consecutive doubles; rows >= n are skipped, and no LDS is declared
// (DESIGN.md §24 counts on that).
//
// Else (apm_is_loo) with t' = log wbar + lp, per row over the tile's 64 sample columns
//   m = max t,  sum e^(t - m),  sum e^(2 (t - m)),  m' = max t',  sum e^(t' - m')
// in a fixed order: the row's maxima first (a maximum does not depend on the order), then a lane
// adds its two column blocks, the 16 lanes of a row their sums by butterfly (xor 1, 2, 4, 8), and
// the two column-waves meet in LDS, where the pairs are rescaled to their common maximum. Rows >= n
// are taken with y = 1, not skipped: the butterflies need every lane. One store per (row < n,
// quantity q) at ob[(q npr + row) ld + sb], ld = the number of sample tiles: no atomics.
struct LooEpi {
    double v[5][64][2];
};

template <int LIK, bool STORE, bool F64MAP>
__device__ __forceinline__ void is_row_epilogue(const double (&f)[2][2][4], int row0, int n,
                                                const double* __restrict__ y,
                                                const double* __restrict__ lwt,
                                                double* __restrict__ ob, int64_t npr, int ld,
                                                int sb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
    const int r16 = lane & 15;
    const double lw0 = lwt[32 * wc + r16], lw1 = lwt[32 * wc + 16 + r16];
    LooEpi* ep = nullptr;
    if constexpr (!STORE) {
        __shared__ LooEpi loo_ep;
        ep = &loo_ep;
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = 32 * wr + 16 * bi + (F64MAP ? F64_CROW(lane, r) : F32_CROW(lane, r));
            if (STORE && row0 + rl >= n) continue;
            const double yr = row0 + rl < n ? y[row0 + rl] : 1.0;
            const double lp0 = lik_logp_mixed<LIK>(yr * f[bi][0][r]);
            const double lp1 = lik_logp_mixed<LIK>(yr * f[bi][1][r]);
            const double t0 = lw0 == -INFINITY ? lw0 : lw0 - lp0;
            const double t1 = lw1 == -INFINITY ? lw1 : lw1 - lp1;
            if constexpr (STORE) {
                double* o = ob + (int64_t)(row0 + rl) * ld + 32 * wc + r16;
                o[0] = t0;
                o[16] = t1;
            } else {
                const double u0 = lw0 == -INFINITY ? lw0 : lw0 + lp0;
                const double u1 = lw1 == -INFINITY ? lw1 : lw1 + lp1;
                double m = fmax(t0, t1), mu = fmax(u0, u1);
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    m = fmax(m, __shfl_xor(m, o, 64));
                    mu = fmax(mu, __shfl_xor(mu, o, 64));
                }
                const double e0 = loo_scaled(t0, m), e1 = loo_scaled(t1, m);
                double q0 = e0 + e1;
                double q1 = e0 * e0 + e1 * e1;
                double q2 = loo_scaled(u0, mu) + loo_scaled(u1, mu);
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    q0 += __shfl_xor(q0, o, 64);
                    q1 += __shfl_xor(q1, o, 64);
                    q2 += __shfl_xor(q2, o, 64);
                }
                if (r16 == 0) {
                    ep->v[0][rl][wc] = m;
                    ep->v[1][rl][wc] = q0;
                    ep->v[2][rl][wc] = q1;
                    ep->v[3][rl][wc] = mu;
                    ep->v[4][rl][wc] = q2;
                }
            }
        }
    if constexpr (!STORE) {
        __syncthreads();
        const int rl = threadIdx.x;
        if (rl < 64 && row0 + rl < n) {
            const double m = fmax(ep->v[0][rl][0], ep->v[0][rl][1]);
            const double a0 = loo_scaled(ep->v[0][rl][0], m), a1 = loo_scaled(ep->v[0][rl][1], m);
            const double mu = fmax(ep->v[3][rl][0], ep->v[3][rl][1]);
            const double c0 = loo_scaled(ep->v[3][rl][0], mu), c1 = loo_scaled(ep->v[3][rl][1], mu);
            const int64_t o = (int64_t)(row0 + rl) * ld + sb, qs = npr * ld;
            ob[o] = m;
            ob[o + qs] = ep->v[1][rl][0] * a0 + ep->v[1][rl][1] * a1;
            ob[o + 2 * qs] = ep->v[2][rl][0] * (a0 * a0) + ep->v[2][rl][1] * (a1 * a1);
            ob[o + 3 * qs] = mu;
            ob[o + 4 * qs] = ep->v[4][rl][0] * c0 + ep->v[4][rl][1] * c1;
        }
    }
}

// chain b's part of `out` for sample tile sb: T's 64 columns of the tile (row pitch sp), or the
// chain's five planes of np x nsb partials
template <bool STORE>
__device__ __forceinline__ double* is_row_out(double* out, int b, int sb, int np, int sp, int nsb) {
    return out + (STORE ? (int64_t)b * np * sp + sb * 64 : (int64_t)b * 5 * np * nsb);
}

// ------------------------------------------------------------------------------- the GEMM
// One 64 x 64 tile (row block i, sample block sb) of C_chol U per workgroup, from the slot's fp32
// factor and the U buffer's fp32 mirror: ugemm_tile.h's work-item order and product, which are
// k_ugemm's, so f_s is bitwise the f_s the weights were formed at.
template <int LIK, bool STORE>
__global__ __launch_bounds__(256) void k_is_row_gemm(SlotSet S, const int64_t* __restrict__ slots,
                                                     UPool P, const int64_t* __restrict__ ubufs,
                                                     const double* __restrict__ y, int n, int np,
                                                     const double* __restrict__ logw,
                                                     double* __restrict__ out,
                                                     const int* __restrict__ status, int nsb,
                                                     int nchains) {
    int b, i, sb;
    ugemm_item(np / 64, nsb, nchains, b, i, sb);
    if (status[b] != 0) return;
    __shared__ float Ut[2][64][65];

    const int64_t slot = slots[b];
    if (S.wide[slot]) return;  // k_is_row_gemm64
    const int sp = P.sp;
    f4_t acc[2][2];
    ugemm_tile32(acc, S.L + slot * S.lstride, P.base32 + ubufs[b] * P.stride, np, sp, i, sb, Ut);

    double f[2][2][4];
    ugemm_add_fpost<false>(f, acc, S.fpost64 + slot * S.vstride, i);
    is_row_epilogue<LIK, STORE, false>(f, i * 64, n, y, logw + (int64_t)b * sp + sb * 64,
                                       is_row_out<STORE>(out, b, sb, np, sp, nsb), np,
                                       STORE ? sp : nsb, sb);
}

// The same on the f64 MFMA for the call's wide slots, from the slot's fp64 factor and the fp64 U
// buffer: k_ugemm64's product (ugemm_tile64).
template <int LIK, bool STORE>
__global__ __launch_bounds__(256) void k_is_row_gemm64(SlotSet S,
                                                       const int64_t* __restrict__ slots, UPool P,
                                                       const int64_t* __restrict__ ubufs,
                                                       const double* __restrict__ y, int n, int np,
                                                       const double* __restrict__ logw,
                                                       double* __restrict__ out,
                                                       const int* __restrict__ status, int nsb) {
    const int b = blockIdx.y;
    if (status[b] != 0) return;
    const int64_t slot = slots[b];
    if (!S.wide[slot]) return;
    const int i = (int)blockIdx.x / nsb, sb = (int)blockIdx.x % nsb;
    __shared__ double La[64][17];
    __shared__ double Ub[16][65];
    const double* L = S.L64[slot];
    if (!L) return;  // (as k_ugemm64; a slot read by a u-call has its buffer attached)
    const int sp = P.sp;
    d4_t acc[2][2];
    ugemm_tile64(acc, L, P.base + ubufs[b] * P.stride, np, sp, i, sb, La, Ub);
    double f[2][2][4];
    ugemm_add_fpost<true>(f, acc, S.fpost64 + slot * S.vstride, i);
    is_row_epilogue<LIK, STORE, true>(f, i * 64, n, y, logw + (int64_t)b * sp + sb * 64,
                                      is_row_out<STORE>(out, b, sb, np, sp, nsb), np,
                                      STORE ? sp : nsb, sb);
}

template <bool STORE>
static void launch_row_gemm(int lik, SlotSet S, const int64_t* slots, UPool P,
                            const int64_t* ubufs, const double* y, int n, int np,
                            const double* logw, double* out, const int* status, int nchains,
                            bool wide, hipStream_t s) {
    const int nb = np / 64, nsb = P.sp / 64;
    const long total = (long)nb * nsb * nchains;
    APM_LIK_DISPATCH(lik, APM_LAUNCH((k_is_row_gemm<LIK, STORE>), dim3((unsigned)total), dim3(256),
                                     0, s, S, slots, P, ubufs, y, n, np, logw, out, status, nsb,
                                     nchains));
    if (wide)
        APM_LIK_DISPATCH(lik, APM_LAUNCH((k_is_row_gemm64<LIK, STORE>),
                                         dim3((unsigned)(nb * nsb), nchains), dim3(256), 0, s, S,
                                         slots, P, ubufs, y, n, np, logw, out, status, nsb));
}

void launch_is_row_gemm(int lik, bool store, SlotSet S, const int64_t* slots, UPool P,
                        const int64_t* ubufs, const double* y, int n, int np, const double* logw,
                        double* out, const int* status, int nchains, bool wide, hipStream_t s) {
    const auto go = store ? launch_row_gemm<true> : launch_row_gemm<false>;
    go(lik, S, slots, P, ubufs, y, n, np, logw, out, status, nchains, wide, s);
}

// ------------------------------------------------------------------------------- finish
// Per (chain, row i < n): the sample tiles' pairs merged in ascending order into
//   loo = -(m + log s),  lpd = m' + log s',  ess_loo = s^2 / s2,
// and the Gaussian (cavity) leave-one-out density of the slot's N(f_post, C), site i removed:
//   tau = 1 / C_ii - W_i,  nu = f_post_i / C_ii - z_i,  C_ii = rowq_i,
//   gauss = log int p(y_i | f) N(f | nu / tau, 1 / tau) df
// (probit: log Phi(y m / sqrt(1 + v)); logit: the log of the Gauss-Hermite average, gh_logit.h);
// a computed tau <= 0 gives NaN for that point's gauss only. out: [quantity 0..3][chain][npr].
template <int LIK>
__global__ __launch_bounds__(256) void k_is_loo_finish(const double* __restrict__ pp, int64_t npr,
                                                       int nst, int n, SlotSet S,
                                                       const int64_t* __restrict__ slots,
                                                       const double* __restrict__ y,
                                                       double* __restrict__ out, int64_t qstride,
                                                       const int* __restrict__ status) {
    const int b = blockIdx.y;
    if (status[b] != 0) return;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t qs = npr * nst;
    const double* p = pp + (int64_t)b * 5 * qs + (int64_t)r * nst;
    double m = -INFINITY, s = 0.0, s2 = 0.0, mu = -INFINITY, su = 0.0;
    for (int t = 0; t < nst; ++t) {
        const double mt = p[t], nm = fmax(m, mt);
        const double a = loo_scaled(m, nm), c = loo_scaled(mt, nm);
        s = s * a + p[t + qs] * c;
        s2 = s2 * (a * a) + p[t + 2 * qs] * (c * c);
        m = nm;
        const double ut = p[t + 3 * qs], nu = fmax(mu, ut);
        su = su * loo_scaled(mu, nu) + p[t + 4 * qs] * loo_scaled(ut, nu);
        mu = nu;
    }
    double* o = out + b * npr + r;
    o[0] = -(m + log(s));
    o[qstride] = mu + log(su);
    o[2 * qstride] = s * s / s2;

    const int64_t so = slots[b] * S.vstride + r;
    const double cii = S.rowq[so];
    const double tau = 1.0 / cii - S.W64[so];
    const double nu = S.fpost64[so] / cii - S.z64[so];
    double g = NAN;
    if (tau > 0.0) {
        const double mc = y[r] * (nu / tau), vc = 1.0 / tau;
        if constexpr (LIK == APM_LIK_LOGIT) g = log(gh_logit_avg(mc, vc));
        else g = log_ndtr_d(mc / sqrt(1.0 + vc));
    }
    o[3 * qstride] = g;
}

void launch_is_loo_finish(int lik, const double* pp, int64_t npr, int nst, int n, SlotSet S,
                          const int64_t* slots, const double* y, double* out, int64_t qstride,
                          const int* status, int nchains, hipStream_t s) {
    APM_LIK_DISPATCH(lik, APM_LAUNCH(k_is_loo_finish<LIK>, dim3((n + 255) / 256, nchains),
                                     dim3(256), 0, s, pp, npr, nst, n, S, slots, y, out, qstride,
                                     status));
}
