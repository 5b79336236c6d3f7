// Joint Laplace / EP predictive at test inputs (apm_predict_joint): the kernels
// around the panel solves, trailing updates and the fp64 factorisation that
// host_predict_joint.cpp borrows from the Cholesky.
//
//   Sigma = K** - V V^T,  V_j = L^-1 (W^1/2 . k*_j)       the latent covariance across the test
//                                                         inputs (no epsilon in K**, as in k*)
//   L_S   = chol(Sigma + eps I)                           kernels.pyx's rule: epsilon on one point
//                                                         set's own Gram
//   f*_r  = mu* + L_S xi_r,  xi the Philox normal stream (seed, counter), element j n_draws + r
//   lpd   = logsumexp_r sum_j log p(y*_j | f*_rj) - log n_draws
//
// The block lives in the work matrix A behind the solved test rows: rows and columns
// [np, np + 64 mb). k_gram_test seeds it, chol_solve_rows' trailing updates subtract V V^T,
// k_joint_eps adds epsilon, chol_factor factors it in place, and k_joint_draw multiplies the
// factor with the normals.
#include "apm_internal.h"
#include "is_weights.h"
#include "pair_tile.h"
#include "philox.h"
#include "tile64.h"

// The test-test Gram into the lower tiles of the block: k_gram_cross's arithmetic (pair_tile.h;
// s, beta and lambda the host's exp, as there) with both point sets the staged test inputs, so
// that the diagonal is k** itself (r^2 = 0 exactly: s [+ beta] [+ lambda |x*|^2]) and a diagonal
// tile is symmetric to the bit. One workgroup per lower 128x128 super-tile. Beyond the ms real
// points the block is the identity, as K is beyond n: the padded rows of V are exact zeros, so the
// padded part of Sigma stays the identity and its factor cannot fail.
template <int FAM, bool BIAS, bool LIN>
__global__ __launch_bounds__(256, 2) void k_gram_test(
    MatB A, int64_t row0, const double* __restrict__ Xs, int ms, int mb, int d,
    const double* __restrict__ theta, int64_t tstride, const double* __restrict__ sig,
    const double* __restrict__ bet, const double* __restrict__ lamv, int ard, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    int si = 0, sj = blockIdx.x;  // the lower super-tile (si, sj) of index blockIdx.x, row-major
    while (sj > si) sj -= ++si;

    __shared__ PairTile lds;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tr = lane >> 3, tc = lane & 7;
    const int ti = 2 * si + (wv >> 1), tj = 2 * sj + (wv & 1);
    const bool mine = ti < mb && tj <= ti;  // (wave-uniform)
    const int ro = 64 * (wv >> 1), co = 64 * (wv & 1);
    const double* th = theta + b * tstride;
    const double sigma = sig[b];
    double beta = 0.0;
    if constexpr (BIAS) beta = bet[b];
    double lam = 0.0;
    if constexpr (LIN) lam = lamv[b];
    double* tile = A.base + b * A.cstride + (row0 + ti * 64) * A.ld + row0 + tj * 64;

    double acc[8][8];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[p][q] = 0.0;

    if constexpr (LIN) {  // the dot products first, parked in the tile this lane overwrites below
        for (int k0 = 0; k0 < d; k0 += GK) {
            const int kc = min(GK, d - k0);
            pair_stage<true>(lds, th, ard, k0, kc, Xs, d, ms, si * 128, Xs, d, ms, sj * 128);
            if (mine) pair_dot_chunk(lds, kc, ro, tr, co, tc, acc);
        }
        if (mine) {
            pair_store_tile(tile, A.ld, tr, tc, acc);
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[p][q] = 0.0;
        }
    }
    for (int k0 = 0; k0 < d; k0 += GK) {
        const int kc = min(GK, d - k0);
        pair_stage(lds, th, ard, k0, kc, Xs, d, ms, si * 128, Xs, d, ms, sj * 128);
        if (mine) pair_r2_chunk(lds, kc, ro, tr, co, tc, acc);
    }
    if (!mine) return;  // (after the last barrier)

#pragma unroll
    for (int p = 0; p < 8; ++p) {
        double dt[8];
        if constexpr (LIN) pair_load_row(tile + R8(tr, p) * A.ld + 4 * tc, dt);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int gi = ti * 64 + R8(tr, p), gj = tj * 64 + R8(tc, q);
            double v = cov_S<FAM>(sigma, acc[p][q]);
            if constexpr (BIAS) v += beta;
            if constexpr (LIN) v = fma(lam, dt[q], v);
            acc[p][q] = (gi < ms && gj < ms) ? v : (gi == gj ? 1.0 : 0.0);
        }
    }
    pair_store_tile(tile, A.ld, tr, tc, acc);
}

void launch_gram_test(MatB A, int64_t row0, const double* Xs, int ms, int mb, int d,
                      const double* theta, int64_t tstride, const double* sig, const double* bet,
                      const double* lam, int kind, Live live, int nchains, hipStream_t s) {
    const int ns = (mb + 1) / 2;
    const KernelKind kk = kernel_kind_of(kind);
    APM_FAMILY_DISPATCH(
        kk.family,
        APM_BIAS_DISPATCH(
            kk.bias,
            APM_LINEAR_DISPATCH(kk.linear,
                                APM_LAUNCH((k_gram_test<FAM, BIAS, LIN>),
                                           dim3(ns * (ns + 1) / 2, nchains), dim3(256), 0, s, A,
                                           row0, Xs, ms, mb, d, theta, tstride, sig, bet, lam,
                                           kk.iso ? 0 : 1, live))));
}

// epsilon onto the ms real diagonal entries of the block (the padded ones stay 1)
__global__ __launch_bounds__(256) void k_joint_eps(MatB A, int64_t row0, int ms, double eps,
                                                   Live live) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (!live_chain(live, b) || j >= ms) return;
    A.base[b * A.cstride + (row0 + j) * (A.ld + 1)] += eps;
}

void launch_joint_eps(MatB A, int64_t row0, int ms, double eps, Live live, int nchains,
                      hipStream_t s) {
    APM_LAUNCH(k_joint_eps, dim3((ms + 255) / 256, nchains), dim3(256), 0, s, A, row0, ms, eps,
               live);
}

// Xi^T per chain (sp rows of ldx doubles, zeroed by the host beforehand): element e = j S + r of
// the stream (seeds[b], counters[b]), which is entry (j, r) of the oracle's u_normal(seed, counter,
// ms, S), goes to row r (the draw), column j (the test point). The values are the generator's fp32
// normals, widened.
__global__ __launch_bounds__(256) void k_joint_normal(double* __restrict__ xi, int64_t xstride,
                                                      int64_t ldx, const uint64_t* __restrict__ seeds,
                                                      const uint64_t* __restrict__ counters, int ms,
                                                      int S, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;  // group of 4 normals
    const int64_t tot = (int64_t)ms * S;
    if (q * 4 >= tot) return;
    float z[4];
    philox_normal4(q, seeds[b], counters[b], z);
    double* dst = xi + b * xstride;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int64_t e = q * 4 + h;
        if (e < tot) dst[(e % S) * ldx + e / S] = (double)z[h];
    }
}

void launch_joint_normal(double* xi, int64_t xstride, int64_t ldx, const uint64_t* seeds,
                         const uint64_t* counters, int ms, int S, Live live, int nchains,
                         hipStream_t s) {
    const int64_t groups = ((int64_t)ms * S + 3) / 4;
    APM_LAUNCH(k_joint_normal, dim3((unsigned)((groups + 255) / 256), nchains), dim3(256), 0, s,
               xi, xstride, ldx, seeds, counters, ms, S, live);
}

// The draws. One workgroup per (chain, test-point tile tj, draw tile tr): the 64 x 64 tile
//   D[r][j] = sum_{k < 64 (tj + 1)} Xi^T[r][k] L_S[j][k]
// of the transposed product Xi^T L_S^T on the f64 MFMA (tile_gemm_nt, tile64.h: both operands
// row-major with the depth contiguous, A = 64 rows of Xi^T, B = row tile tj of the factor). The
// factor is lower triangular with zeros above the diagonal inside its diagonal tiles (diag_store),
// so the depth ends with column tile tj and the tiles above the diagonal are never read. With the
// draws on the tile's rows a draw's 16 lanes store 128 contiguous bytes of its row of the output.
// Epilogue: f = mu*_j + D[r][j]; stored at draws[b][r][j] where asked for; and, with labels, the
// tile's share of sum_j log p(y*_j | f_rj) per draw in a fixed order - the lane's two column
// blocks, the butterfly over its 16-lane row group, the two column halves through LDS (left
// first) - into part[b][tj sp + r]; k_joint_lme adds the tiles in ascending tj.
// The heaviest tiles (largest tj) are dispatched first.
template <int LIK>
__global__ __launch_bounds__(256) void k_joint_draw(
    MatB A, int64_t row0, int ms, int mb, const double* __restrict__ xi, int64_t xstride,
    int64_t ldx, int S, int sp, const double* __restrict__ mean, int64_t mstride,
    const double* __restrict__ ys, double* __restrict__ draws, int64_t dstride,
    double* __restrict__ part, int64_t pstride, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int nst = sp / 64;
    const int tj = mb - 1 - (int)blockIdx.x / nst, tr = (int)blockIdx.x % nst;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
    __shared__ GemmSmem sm;
    __shared__ double csum[2][64];

    const double* Lrow = A.base + b * A.cstride + (row0 + tj * 64) * A.ld + row0;
    const double* Xrow = xi + b * xstride + (int64_t)(tr * 64) * ldx;
    d4_t acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = d4_t{0.0, 0.0, 0.0, 0.0};
    tile_gemm_nt<false>(acc, Xrow, ldx, Lrow, A.ld, 64 * (tj + 1), sm);

    double mu[2], yv[2];
    int col[2];
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        col[bj] = tj * 64 + 32 * wc + 16 * bj + (lane & 15);
        mu[bj] = col[bj] < ms ? mean[b * mstride + col[bj]] : 0.0;
        yv[bj] = (ys && col[bj] < ms) ? ys[col[bj]] : 0.0;
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 32 * wr + 16 * bi + F64_CROW(lane, r);
            const int gr = tr * 64 + row;
            double lp = 0.0;
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                const double f = mu[bj] + acc[bi][bj][r];
                if (col[bj] < ms) {
                    if (draws && gr < S) draws[b * dstride + (int64_t)gr * ms + col[bj]] = f;
                    if (ys) lp += lik_logp<LIK>(yv[bj] * f);
                }
            }
            if (ys) {  // (uniform)
                lp += __shfl_xor(lp, 1, 64);
                lp += __shfl_xor(lp, 2, 64);
                lp += __shfl_xor(lp, 4, 64);
                lp += __shfl_xor(lp, 8, 64);
                if ((lane & 15) == 0) csum[wc][row] = lp;
            }
        }
    if (!ys) return;
    __syncthreads();
    if (threadIdx.x < 64)
        part[b * pstride + (int64_t)tj * sp + tr * 64 + threadIdx.x] =
            csum[0][threadIdx.x] + csum[1][threadIdx.x];
}

void launch_joint_draw(int lik, MatB A, int64_t row0, int ms, int mb, const double* xi,
                       int64_t xstride, int64_t ldx, int S, int sp, const double* mean,
                       int64_t mstride, const double* ys, double* draws, int64_t dstride,
                       double* part, int64_t pstride, Live live, int nchains, hipStream_t s) {
    APM_LIK_DISPATCH(lik, APM_LAUNCH(k_joint_draw<LIK>, dim3(mb * (sp / 64), nchains), dim3(256),
                                     0, s, A, row0, ms, mb, xi, xstride, ldx, S, sp, mean, mstride,
                                     ys, draws, dstride, part, pstride, live));
}

// logsumexp_r(sum_j log p) - log S per chain: the IS estimate's reduction (is_weights.h) over the
// mb tile rows of `part`, with no constant
__global__ __launch_bounds__(256) void k_joint_lme(const double* __restrict__ part,
                                                   int64_t pstride, int mb, int S, int sp,
                                                   double* __restrict__ out, Live live) {
    const int b = blockIdx.x;
    if (!live_chain(live, b)) return;
    is_lme<false>(part + b * pstride, mb, S, sp, 0.0, out + b, 0);
}

void launch_joint_lme(const double* part, int64_t pstride, int mb, int S, int sp, double* out,
                      Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_joint_lme, dim3(nchains), dim3(256), 0, s, part, pstride, mb, S, sp, out, live);
}
