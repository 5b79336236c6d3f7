// Importance-sampling predictive distribution at test inputs: the kernels of the
// tail that host_is_predict.cpp runs after an IS theta-call, all fp64.
//
// With the importance samples f_s = f_post + C_chol u_s of the call's U buffer and their
// self-normalised weights w_s (the summands of the IS estimate, ugemm.hip's log w_s), the
// conditional mean of f*_j given f_s is
//   m_sj = c_j + h_j^T u_s,   c_j = k*_j^T a,   h_j = U_M^-1 L_K^-1 k*_j,
// and its variance v*_j = s - |L_K^-1 k*_j|^2 does not depend on s. The host leaves the rows
// (J h_j)^T = (L'^-1 J p_j)^T in the work matrix (L' the factor of J M J); the GEMM below takes them
// against the row-reversed U buffer, so no K^-1 is ever applied to a computed f_s.
#include "apm_internal.h"
#include "gh_logit.h"
#include "is_weights.h"
#include "tile64.h"

// ------------------------------------------------------------------------------- weights
// Per chain, from the per-sample values the theta-call's k_ugemm left in `partial`: the
// self-normalised weights wbar_s, exact zeros for the padded columns [S, sp), and ess = 1 / sum
// wbar_s^2 (is_weights.h's is_self_normalise, storing the weights themselves).
__global__ __launch_bounds__(256) void k_is_weights(const double* __restrict__ partial,
                                                    int64_t pstride, int nb, int S, int sp,
                                                    const double* __restrict__ cst,
                                                    const int64_t* __restrict__ slots,
                                                    double* __restrict__ wbar,
                                                    double* __restrict__ ess, Live live) {
    const int b = blockIdx.x;
    if (!live_chain(live, b)) return;
    is_self_normalise<false>(partial + b * pstride, nb, S, sp, cst[slots[b]],
                             wbar + (int64_t)b * sp, ess + b);
}

void launch_is_weights(const double* partial, int64_t pstride, int nb, int S, int sp,
                       const double* cst, const int64_t* slots, double* wbar, double* ess,
                       Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_is_weights, dim3(nchains), dim3(256), 0, s, partial, pstride, nb, S, sp, cst,
               slots, wbar, ess, live);
}

// ------------------------------------------------------------------------------- U^T, reversed
// Ut[b][s][k] = U[ubufs[b]][np - 1 - k][s] (sp x np per chain, ld = np): the NT operand of the
// GEMM, whose depth index runs over the reversed rows as the h-rows' columns do. 64x64 tiles
// through LDS; the U buffer is only read.
__global__ __launch_bounds__(256) void k_is_ut(UPool P, const int64_t* __restrict__ ubufs, int np,
                                               double* __restrict__ Ut, Live live) {
    const int b = blockIdx.z;
    if (!live_chain(live, b)) return;
    __shared__ double T[64][65];
    const double* U = P.base + ubufs[b] * P.stride;
    const int k0 = blockIdx.x * 64, s0 = blockIdx.y * 64;
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int r = e >> 6, cc = e & 63;  // U row k0 + r, sample s0 + cc
        T[r][cc] = U[(int64_t)(k0 + r) * P.sp + s0 + cc];
    }
    __syncthreads();
    double* D = Ut + (int64_t)b * P.sp * np;
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int sl = e >> 6, kl = e & 63;  // Ut row s0 + sl, column np - 64 - k0 + kl
        D[(int64_t)(s0 + sl) * np + (np - 64 - k0) + kl] = T[63 - kl][sl];
    }
}

void launch_is_ut(UPool P, const int64_t* ubufs, int np, double* Ut, Live live, int nchains,
                  hipStream_t s) {
    APM_LAUNCH(k_is_ut, dim3(np / 64, P.sp / 64, nchains), dim3(256), 0, s, P, ubufs, np, Ut, live);
}

// ------------------------------------------------------------------------------- the p-rows
// One wave per (chain, row r < 64 mb) of the solved rows p_r^T = k*_r^T L_K^-T in A's rows
// [row0, ..) x columns [0, 64 nb): v*_r = sig[b] - |p_r|^2 (row_sqnorm_d2, as k_predict_reduce;
// nothing is clamped), c_r = the tile-column partials
// of k*_r . a in order, and the reversed row p_r^T J into columns [64 nb, 128 nb) of the same row
// (the right-hand side of the solve against L'). Rows >= ms are exact zeros (k_gram_cross).
__global__ __launch_bounds__(256) void k_is_rows(MatB A, int64_t row0, int ms, int mb, int nb,
                                                 const double* __restrict__ sig,
                                                 const double* __restrict__ lam,
                                                 const double* __restrict__ xsn,
                                                 const double* __restrict__ part, int64_t pstride,
                                                 double* __restrict__ vstar,
                                                 double* __restrict__ cvec, int64_t ostride,
                                                 Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= 64 * mb) return;
    const int np = 64 * nb;
    double* row = A.base + b * A.cstride + (row0 + r) * A.ld;
    const double s = row_sqnorm_d2(row, np, lane, [&](int c, d2_t v) {
        *reinterpret_cast<d2_t*>(row + np + (np - 2 - c)) = d2_t{v.y, v.x};
    });
    if (lane != 0) return;
    // (lam: null unless the kind has the linear term; rows >= ms keep sig[b])
    vstar[b * ostride + r] = ((lam && r < ms) ? fma(lam[b], xsn[r], sig[b]) : sig[b]) - s;
    cvec[b * ostride + r] = r < ms ? sum_tile_partials(part + b * pstride + r, nb, 64 * mb) : 0.0;
}

void launch_is_rows(MatB A, int64_t row0, int ms, int mb, int nb, const double* sig,
                    const double* lam, const double* xsn, const double* part, int64_t pstride,
                    double* vstar, double* cvec, int64_t ostride, Live live, int nchains,
                    hipStream_t s) {
    APM_LAUNCH(k_is_rows, dim3(16 * mb, nchains), dim3(256), 0, s, A, row0, ms, mb, nb, sig, lam,
               xsn, part, pstride, vstar, cvec, ostride, live);
}

// ------------------------------------------------------------------------------- the link
// (the logit's Gauss-Hermite average on one thread, gh_logit_avg: gh_logit.h)
template <int LIK>
__device__ __forceinline__ double is_link(double mu, double v) {
    if constexpr (LIK == APM_LIK_LOGIT) {
        return gh_logit_avg(mu, v);
    } else {  // Phi(mu / sqrt(1 + v)) through erfc, as k_predict_reduce
        return 0.5 * erfc(-(mu / sqrt(1.0 + v)) * 0.70710678118654752440);
    }
}

// ------------------------------------------------------------------------------- the GEMM
// Workgroup (sample tile tj, row tile ti, chain b): acc = Hrev[64 ti .., :] Ut[64 tj .., :]^T over
// the depth np on the f64 MFMA (tile_gemm_nt), then the epilogue on the accumulators in place:
// m = c_r + acc, l = link(m, v*_r), and the weighted sums over the tile's 64 samples of
//   wbar_s l,  wbar_s m,  wbar_s m^2
// in a fixed order: a lane adds its two columns (bj = 0, 1), the 16 lanes of a row their sums by
// butterfly (xor 1, 2, 4, 8), and the two waves that share the rows (wc = 0, 1) meet in LDS. One
// store per (row, quantity) into pp[((b 3 + q) npr + row) nst + tj]: no atomics. Padded sample
// columns carry wbar = 0 exactly and zero U entries (m = c_r, finite), so they add exact zeros.
struct IsEpi {
    double v[3][64][2];
};

template <int LIK>
__global__ __launch_bounds__(256) void k_is_pred_gemm(
    MatB A, int64_t row0, int64_t col0, int np, const double* __restrict__ Ut, int sp,
    const double* __restrict__ wbar, const double* __restrict__ vstar,
    const double* __restrict__ cvec, int64_t ostride, double* __restrict__ pp, int64_t npr,
    Live live) {
    const int b = blockIdx.z;
    if (!live_chain(live, b)) return;
    const int tj = blockIdx.x, ti = blockIdx.y, nst = gridDim.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
    __shared__ GemmSmem sm;
    __shared__ IsEpi ep;
    d4_t acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = d4_t{0.0, 0.0, 0.0, 0.0};
    const double* H = A.base + b * A.cstride + (row0 + 64 * ti) * A.ld + col0;
    const double* Bt = Ut + ((int64_t)b * sp + 64 * tj) * np;
    tile_gemm_nt<false>(acc, H, A.ld, Bt, np, np, sm);

    const double* wb = wbar + (int64_t)b * sp + 64 * tj + 32 * wc + (lane & 15);
    const double w0 = wb[0], w1 = wb[16];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = 32 * wr + 16 * bi + F64_CROW(lane, r);  // row of the tile
            const int64_t ro = b * ostride + 64 * ti + rl;
            const double cr = cvec[ro], vr = vstar[ro];
            const double m0 = cr + acc[bi][0][r], m1 = cr + acc[bi][1][r];
            double q0 = w0 * is_link<LIK>(m0, vr) + w1 * is_link<LIK>(m1, vr);
            double q1 = w0 * m0 + w1 * m1;
            double q2 = w0 * (m0 * m0) + w1 * (m1 * m1);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                q0 += __shfl_xor(q0, o, 64);
                q1 += __shfl_xor(q1, o, 64);
                q2 += __shfl_xor(q2, o, 64);
            }
            if ((lane & 15) == 0) {
                ep.v[0][rl][wc] = q0;
                ep.v[1][rl][wc] = q1;
                ep.v[2][rl][wc] = q2;
            }
        }
    __syncthreads();
    if (threadIdx.x < 192) {
        const int q = threadIdx.x >> 6, rl = threadIdx.x & 63;
        pp[(((int64_t)b * 3 + q) * npr + 64 * ti + rl) * nst + tj] = ep.v[q][rl][0] + ep.v[q][rl][1];
    }
}

void launch_is_pred_gemm(int lik, MatB A, int64_t row0, int64_t col0, int np, int mb,
                         const double* Ut, int sp, const double* wbar, const double* vstar,
                         const double* cvec, int64_t ostride, double* pp, int64_t npr, Live live,
                         int nchains, hipStream_t s) {
    APM_LIK_DISPATCH(lik, APM_LAUNCH(k_is_pred_gemm<LIK>, dim3(sp / 64, mb, nchains), dim3(256), 0,
                                     s, A, row0, col0, np, Ut, sp, wbar, vstar, cvec, ostride, pp,
                                     npr, live));
}

// ------------------------------------------------------------------------------- finish
// per (chain, test row r < ms): the sample-tile partials in order ->
//   prob = sum wbar l,  mean = sum wbar m,  var = v*_r + sum wbar m^2 - mean^2
__global__ __launch_bounds__(256) void k_is_finish(const double* __restrict__ pp, int64_t npr,
                                                   int nst, int ms,
                                                   const double* __restrict__ vstar,
                                                   double* __restrict__ mean,
                                                   double* __restrict__ var,
                                                   double* __restrict__ prob, int64_t ostride,
                                                   Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= ms) return;
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* p = pp + (((int64_t)b * 3 + k) * npr + r) * nst;
        double s = 0.0;
        for (int t = 0; t < nst; ++t) s += p[t];
        q[k] = s;
    }
    prob[b * ostride + r] = q[0];
    mean[b * ostride + r] = q[1];
    var[b * ostride + r] = vstar[b * ostride + r] + q[2] - q[1] * q[1];
}

void launch_is_finish(const double* pp, int64_t npr, int nst, int ms, const double* vstar,
                      double* mean, double* var, double* prob, int64_t ostride, Live live,
                      int nchains, hipStream_t s) {
    APM_LAUNCH(k_is_finish, dim3((ms + 255) / 256, nchains), dim3(256), 0, s, pp, npr, nst, ms,
               vstar, mean, var, prob, ostride, live);
}
