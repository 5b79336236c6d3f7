// ARD / isotropic squared-exponential Gram builder (fp64), replacing gpdemo/kernels.pyx.
//
//   isotropic_squared_exponential_kernel  kernels.pyx:12-49   K_ij = s exp(-|x_i-x_j|^2 / (2 tau^2))
//   diagonal_squared_exponential_kernel   kernels.pyx:52-90   K_ij = s exp(-1/2 sum_k ((x_ik-x_jk)/tau_k)^2)
//   Matern 3/2 and 5/2 (no reference counterpart): the same scaled squared distance
//   through another epilogue (cov_S<FAM>, apm_internal.h), iso or ARD
//   K_ii = s + eps. both != 0: both triangles written (the reference fills K[i,j] and K[j,i];
//   the stand-alone apm_gram); both == 0: lower tiles only (the theta-call: every consumer on the
//   device path reads K's lower tiles, so the upper half is never written - half the bytes).
// X row blocks are staged through LDS in chunks of 32 features, multiplied by 1/tau_k on the way
// in (2 fp64 VALU ops per pair and feature); the tile and its transpose are written with 32-byte
// contiguous runs per lane (two coalesced 256-byte runs per row and 8 lanes).
// Roofline: 8 B written per K element (HBM) vs ~(2D + ~40 for exp) fp64 VALU ops per lower pair.
#include "apm_internal.h"
#include "pair_tile.h"

#ifndef GRAM_ABL  // ablations (tools/gram_bench.cpp): 1 no exp, 2 no stores, 3 no distance loop
#define GRAM_ABL 0
#endif

// One workgroup of 4 waves per lower 128x128 super-tile (si >= sj); wave w computes 64x64 tile
// (2si + w/2, 2sj + w%2) - the upper tile of a diagonal super-tile and tiles beyond the padded
// size are skipped - with an 8x8 block of pairs per lane (pair_tile.h: staging, distance loop
// and stores).
// K2 (the concurrent chol(K)'s working copy, host_theta.cpp chol_k_begin) receives the tiles of tile
// columns < k2cols only: the first outer panel's trailing update reads the rest from K itself.
// FAM (APM_FAM_*) selects the epilogue that turns a pair's r^2 into its covariance (cov_S); the
// distance loop, the LDS staging, the tiling and the stores are the same for every family.
// ard: theta[1 + k] scales feature k (ARD), else theta[1] scales every feature (iso).
// BIAS: the constant term: beta = exp of theta's last entry is added to cov_S for
// the data pairs only, K_ii = (s + beta) + eps; a padded row or column never sees it.
// LIN: the linear term (the SE family only): lambda = exp of theta's last entry
// (beta is then the one before it). A sweep of its own over the feature chunks stages the unscaled
// inputs into the same LDS image and sums x_i . x_j in the lane's 8x8 block by one fma per feature,
// k in order (pair_dot_chunk). There is no room for a second 8x8 block, and adding the features
// onto cov_S [+ beta] one by one would round d times at the size of K instead of once; so the
// dot products are parked in the lane's own entries of the K tile, which it overwrites below,
// while the block serves the distance sweep, and the epilogue reads them back:
// K_ij = fma(lambda, x_i . x_j, cov_S [+ beta]), K_ii = fma(lambda, |x_i|^2, s [+ beta]) + eps.
// The identity padding is selected as before: a padded row or column never sees lambda.
template <int FAM, bool BIAS, bool LIN>
__global__ __launch_bounds__(256, 2) void k_gram(MatB K, const double* __restrict__ X, int64_t ldx,
                                                 int n, int d, const double* __restrict__ theta,
                                                 int64_t tstride, int ard, double eps, Live live,
                                                 int both, MatB K2, int k2cols, int nb) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    int si, sj;  // the lower super-tile, si >= sj
    lower_tri_index(blockIdx.x, si, sj);

    __shared__ PairTile lds;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tr = lane >> 3, tc = lane & 7;
    const int ti = 2 * si + (wv >> 1), tj = 2 * sj + (wv & 1);
    const bool mine = ti < nb && tj <= ti;
    const int ro = 64 * (wv >> 1), co = 64 * (wv & 1);
    const double* th = theta + b * tstride;
    const double sigma = exp(th[0]);
    double beta = 0.0;
    if constexpr (BIAS) beta = exp(th[ard ? d + 1 : 2]);
    double lam = 0.0;
    if constexpr (LIN) lam = exp(th[(ard ? d + 1 : 2) + (BIAS ? 1 : 0)]);

    double acc[8][8];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[p][q] = 0.0;

    double* Kb = K.base + b * K.cstride;
    if constexpr (LIN) {
        for (int k0 = 0; k0 < d; k0 += GK) {
            const int kc = min(GK, d - k0);
            pair_stage<true>(lds, th, ard, k0, kc, X, ldx, n, si * 128, X, ldx, n, sj * 128);
            if (mine) pair_dot_chunk(lds, kc, ro, tr, co, tc, acc);
        }
        if (mine) {
            pair_store_tile(Kb + (int64_t)ti * 64 * K.ld + tj * 64, K.ld, tr, tc, acc);
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[p][q] = 0.0;
        }
    }
    for (int k0 = 0; k0 < d; k0 += GK) {
        const int kc = min(GK, d - k0);
        pair_stage(lds, th, ard, k0, kc, X, ldx, n, si * 128, X, ldx, n, sj * 128);
        if (mine && GRAM_ABL != 3) pair_r2_chunk(lds, kc, ro, tr, co, tc, acc);
    }
    if (!mine) return;  // (after the last barrier)

#pragma unroll
    for (int p = 0; p < 8; ++p) {
        double dt[8];  // (LIN: the row's parked dot products)
        if constexpr (LIN)
            pair_load_row(Kb + ((int64_t)ti * 64 + R8(tr, p)) * K.ld + tj * 64 + 4 * tc, dt);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int gi = ti * 64 + R8(tr, p), gj = tj * 64 + R8(tc, q);
            double val;
            if constexpr (LIN) {
                if (gi < n && gj < n)
                    val = (gi == gj) ? fma(lam, dt[q], sigma + beta) + eps
                                     : fma(lam, dt[q], cov_S<FAM>(sigma, acc[p][q]) + beta);
                else
                    val = (gi == gj) ? 1.0 : 0.0;
            } else if constexpr (BIAS) {
                if (gi < n && gj < n)
                    val = (gi == gj) ? (sigma + beta) + eps : cov_S<FAM>(sigma, acc[p][q]) + beta;
                else
                    val = (gi == gj) ? 1.0 : 0.0;
            } else if (gi < n && gj < n)
                val = (gi == gj) ? sigma + eps
                                 : (GRAM_ABL == 1 ? sigma * acc[p][q] : cov_S<FAM>(sigma, acc[p][q]));
            else
                val = (gi == gj) ? 1.0 : 0.0;
            acc[p][q] = val;
        }
    }
    if (GRAM_ABL == 2 && acc[0][0] != -1.0) return;
    pair_store_tile(Kb + (int64_t)ti * 64 * K.ld + tj * 64, K.ld, tr, tc, acc);
    if (K2.base && tj < k2cols)
        pair_store_tile(K2.base + b * K2.cstride + (int64_t)ti * 64 * K2.ld + tj * 64, K2.ld, tr,
                        tc, acc);
    if (both && ti != tj) {  // transposed tile (tj, ti)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double col[8] = {acc[0][q], acc[1][q], acc[2][q], acc[3][q],
                                   acc[4][q], acc[5][q], acc[6][q], acc[7][q]};
            pair_store_row(Kb + (int64_t)(tj * 64 + R8(tc, q)) * K.ld + ti * 64 + 4 * tr, col);
        }
    }
}

void launch_gram(MatB K, const double* X, int64_t ldx, int n, int d, const double* theta,
                 int64_t tstride, int kind, double eps, int np, Live live, int nchains,
                 hipStream_t s, bool both, MatB K2, int k2cols) {
    const int nb = np / 64, ns = (nb + 1) / 2;
    const KernelKind kk = kernel_kind_of(kind);
    APM_FAMILY_DISPATCH(
        kk.family,
        APM_BIAS_DISPATCH(
            kk.bias,
            APM_LINEAR_DISPATCH(kk.linear,
                                APM_LAUNCH((k_gram<FAM, BIAS, LIN>), dim3(ns * (ns + 1) / 2, nchains),
                                           dim3(256), 0, s, K, X, ldx, n, d, theta, tstride,
                                           kk.iso ? 0 : 1, eps, live, (int)both, K2, k2cols, nb))));
}
