// The pair-distance tile of k_gram (gram.hip), k_gram_cross (predict.hip) and k_grad_reduce
// (gradient.hip): one workgroup of 4 waves per 128x128 super-tile, wave w the 64x64 tile
// (w / 2, w % 2) of it, an 8x8 block of pairs per lane. The rows' and the columns' features are
// staged through LDS in chunks of GK, multiplied by 1/tau_k on the way in; a pair's scaled squared
// distance r^2 = sum_k ((x_ik - x_jk)/tau_k)^2 is summed over k in order (the reference's loop,
// kernels.pyx:80-88, up to the pre-scaling). Staging, operand load, distance loop and row store
// exist here only: the three kernels differ in what they do with r^2.
#pragma once
#include "apm_common.h"

#define GK 32       // features per LDS chunk
#define GP (128 + 2)  // LDS row pitch in doubles (16-byte aligned; the transposing staging stores
                      // of consecutive features land 4 banks apart instead of on one bank)
// lane (g = lane >> 3 or lane & 7) -> its 8 rows (columns) of the wave's 64x64 tile:
// {4g .. 4g+3, 32+4g .. 32+4g+3}, so that 8 lanes cover two contiguous 256-byte runs of a row
#define R8(g, p) (((p) >> 2) * 32 + 4 * (g) + ((p) & 3))

// The LDS image of one feature chunk (one __shared__ instance per kernel): xi[k][r] feature k of
// super-tile row r, xj[k][c] of super-tile column c, both pre-scaled by itau[k] = 1/tau_k.
struct PairTile {
    __attribute__((aligned(16))) double xi[GK][GP];
    __attribute__((aligned(16))) double xj[GK][GP];
    double itau[GK];
};

// Features [k0, k0 + kc) of rows [i0, i0 + 128) of Xi and of rows [j0, j0 + 128) of Xj -> LDS,
// pre-scaled; zeros for rows beyond ni (nj) and features beyond kc. The first barrier ends the
// reads of the previous chunk, the last one publishes this one. ard: th[1 + k] scales feature k,
// else th[1] every feature. RAW: the features as they are (the linear term's dot products are on
// the unscaled inputs): th, ard and itau are not touched.
template <bool RAW = false>
__device__ __forceinline__ void pair_stage(PairTile& s, const double* __restrict__ th, int ard,
                                           int k0, int kc, const double* __restrict__ Xi,
                                           int64_t ldi, int ni, int i0,
                                           const double* __restrict__ Xj, int64_t ldj, int nj,
                                           int j0) {
    const int tid = threadIdx.x;
    __syncthreads();
    if constexpr (!RAW) {
        if (tid < kc) s.itau[tid] = exp(-th[ard ? 1 + k0 + tid : 1]);
        __syncthreads();
    }
    for (int e = tid; e < 128 * GK; e += 256) {
        const int r = e / GK, k = e % GK;  // consecutive lanes: consecutive features of a row
        const int gi = i0 + r, gj = j0 + r;
        const double sc = RAW ? 1.0 : ((k < kc) ? s.itau[k] : 0.0);
        s.xi[k][r] = (k < kc && gi < ni) ? Xi[(int64_t)gi * ldi + k0 + k] * sc : 0.0;
        s.xj[k][r] = (k < kc && gj < nj) ? Xj[(int64_t)gj * ldj + k0 + k] * sc : 0.0;
    }
    __syncthreads();
}

// Feature k of a lane's 8 rows (a) and 8 columns (c); ro, co: the wave's tile within the
// super-tile (0 or 64), tr = lane >> 3, tc = lane & 7
__device__ __forceinline__ void pair_operands(const PairTile& s, int k, int ro, int tr, int co,
                                              int tc, double (&a)[8], double (&c)[8]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const d2_t va = *reinterpret_cast<const d2_t*>(&s.xi[k][ro + R8(tr, 2 * h)]);
        const d2_t vc = *reinterpret_cast<const d2_t*>(&s.xj[k][co + R8(tc, 2 * h)]);
        a[2 * h] = va.x;
        a[2 * h + 1] = va.y;
        c[2 * h] = vc.x;
        c[2 * h + 1] = vc.y;
    }
}

// acc[p][q] += the staged chunk's share of r^2 of pair (row R8(tr, p), column R8(tc, q)): per
// feature 16 fp64 LDS values feed 64 (subtract, fma) pairs, so the LDS reads stay at half the
// VALU issue (a 4x4 block per lane tied them)
__device__ __forceinline__ void pair_r2_chunk(const PairTile& s, int kc, int ro, int tr, int co,
                                              int tc, double (&acc)[8][8]) {
    for (int k = 0; k < kc; ++k) {
        double a[8], c[8];
        pair_operands(s, k, ro, tr, co, tc, a, c);
        // a row's 8 differences first, then their 8 fmas: no fma waits on the subtract issued
        // right before it (one shared temporary serialised every pair on the fp64 dependency
        // latency)
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            double df[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) df[q] = a[p] - c[q];  // pre-scaled by 1/tau_k
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[p][q] = fma(df[q], df[q], acc[p][q]);
        }
    }
}

// acc[p][q] += the staged (RAW) chunk's share of x_i . x_j of pair (row R8(tr, p), column
// R8(tc, q)): one fma per feature, k in order. The product inside an fma is exact, so (i, j) and
// (j, i) of a diagonal tile get the same bits.
__device__ __forceinline__ void pair_dot_chunk(const PairTile& s, int kc, int ro, int tr, int co,
                                               int tc, double (&acc)[8][8]) {
    for (int k = 0; k < kc; ++k) {
        double a[8], c[8];
        pair_operands(s, k, ro, tr, co, tc, a, c);
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[p][q] = fma(a[p], c[q], acc[p][q]);
    }
}

// pair_store_row's inverse: the lane's 8 values of one row back from src
__device__ __forceinline__ void pair_load_row(const double* src, double (&v)[8]) {
    const d2_t v0 = *reinterpret_cast<const d2_t*>(src);
    const d2_t v1 = *reinterpret_cast<const d2_t*>(src + 2);
    const d2_t v2 = *reinterpret_cast<const d2_t*>(src + 32);
    const d2_t v3 = *reinterpret_cast<const d2_t*>(src + 34);
    v[0] = v0.x, v[1] = v0.y, v[2] = v1.x, v[3] = v1.y;
    v[4] = v2.x, v[5] = v2.y, v[6] = v3.x, v[7] = v3.y;
}

// A lane's 8 values of one row (columns R8(g, 0..7) of the tile) as four 16-byte stores; dst: the
// row's element at tile column 4g. 8 lanes write two contiguous 256-byte runs.
__device__ __forceinline__ void pair_store_row(double* dst, const double (&v)[8]) {
    *reinterpret_cast<d2_t*>(dst) = d2_t{v[0], v[1]};
    *reinterpret_cast<d2_t*>(dst + 2) = d2_t{v[2], v[3]};
    *reinterpret_cast<d2_t*>(dst + 32) = d2_t{v[4], v[5]};
    *reinterpret_cast<d2_t*>(dst + 34) = d2_t{v[6], v[7]};
}

// The lane's 8x8 block into the 64x64 tile at `tile` (its first element; leading dimension ld)
__device__ __forceinline__ void pair_store_tile(double* tile, int64_t ld, int tr, int tc,
                                                const double (&v)[8][8]) {
#pragma unroll
    for (int p = 0; p < 8; ++p) pair_store_row(tile + R8(tr, p) * ld + 4 * tc, v[p]);
}
