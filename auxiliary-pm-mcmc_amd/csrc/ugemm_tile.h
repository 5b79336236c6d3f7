// The u-path's product C_chol U on a 64 x 64 tile (row block i, sample block sb), once per
// precision, for the two kernel pairs that form the samples f_s = f_post + C_chol u_s:
// k_ugemm / k_ugemm64 (ugemm.hip: the weights) and k_is_row_gemm / k_is_row_gemm64 (is_loo.hip:
// the row-wise epilogues of LOO and PSIS). They differ in their epilogues alone. LOO and PSIS
// need f_s bitwise as the weights were formed at it, so the work-item order, the staging and the
// accumulation order are written once, here. The one exception is k_ugemm, which carries the text
// of ugemm_tile32 itself (it measured 0.8 % slower through the call): a change to
// ugemm_tile32 is made there too.
//
// A workgroup is 256 threads, its four waves 2 x 2 over the tile (wr = wave >> 1 the row half,
// wc = wave & 1 the column half), each wave 2 x 2 blocks of 16 x 16. The LDS staging arrays are the
// calling kernel's (declared beside its epilogue's own storage).
#pragma once
#include "apm_common.h"
#include "tile32.h"  // F32_CROW
#include "tile64.h"  // F64_CROW

// The work item of workgroup blockIdx.x of the fp32 kernels' 1-D grid of nb nsb nchains.
// XCD-aware order: dispatch slot s runs on XCD s % 8, and consecutive work items land on the same
// XCD. The expression is the text of xcd_remap (update_item.h), kept here: through the call
// k_ugemm's prologue came out three instructions shorter, its loop 12 bytes earlier, and the
// kernel 0.2 to 0.5 % slower (as §26 found for its loop); a change to xcd_remap is
// made here too. Items run chain-major, then row block (heaviest,
// i.e. longest K range, first; consecutive row blocks read nearly the same rows of U), then sample
// block fastest - so the nsb workgroups that share row block i's slice of L run together on one
// XCD and read it once from its L2, and a chain's U stays within one XCD's L2 / the Infinity Cache.
// (The f64 twins run on a plain (nb nsb, nchains) grid.)
__device__ __forceinline__ void ugemm_item(int nb, int nsb, int nchains, int& b, int& i, int& sb) {
    const long total = (long)nb * nsb * nchains;
    const long slot_id = blockIdx.x, xcd = slot_id & 7, q = total >> 3, rem = total & 7;
    const long item = nchains < 8 ? slot_id  // too few chains to fill 8 XCDs evenly: plain order
                      : (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (slot_id >> 3);
    b = (int)(item / ((long)nb * nsb));
    const int rest = (int)(item % ((long)nb * nsb));
    i = nb - 1 - rest / nsb;
    sb = rest % nsb;
}

// acc = L[i*64 : i*64+64][0 : (i+1)*64] . U[0 : (i+1)*64][sb*64 : sb*64+64] on
// v_mfma_f32_16x16x4_f32 (A lane l -> A[l&15][k=l>>4], B lane l -> B[k=l>>4][l&15], C/D lane l,
// reg r -> row F32_CROW(l, r), col l&15), L of row pitch np, U of row pitch sp.
// U[kk:kk+64][sb*64 : sb*64+64] (16 KB, 16-byte loads) and the A fragments (straight from global:
// 16 contiguous floats per lane and row) of the next slice are loaded into registers while the
// current one is multiplied; U goes through two LDS buffers (row pitch 65: conflict-free
// B-fragment reads), one barrier per slice.
__device__ __forceinline__ void ugemm_tile32(f4_t (&acc)[2][2], const float* L, const float* U,
                                             int np, int sp, int i, int sb,
                                             float (&Ut)[2][64][65]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kend = (i + 1) * 64;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};

    f4_t un[4];
    f4_t an[2][4];
    auto gload = [&](int kk) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int e = tid + h * 256;  // 4-element piece, 16 per U row
            un[h] = *reinterpret_cast<const f4_t*>(U + (int64_t)(kk + e / 16) * sp + sb * 64 +
                                                   (e % 16) * 4);
        }
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
            const float* p = L + (int64_t)(i * 64 + 32 * wr + 16 * bi + r16) * np + kk + kq * 16;
#pragma unroll
            for (int t = 0; t < 4; ++t) an[bi][t] = *reinterpret_cast<const f4_t*>(p + 4 * t);
        }
    };
    gload(0);
    for (int kk = 0, cur = 0; kk < kend; kk += 64, cur ^= 1) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int e = tid + h * 256;
            const int r = e / 16, c4 = (e % 16) * 4;
            Ut[cur][r][c4] = un[h][0];
            Ut[cur][r][c4 + 1] = un[h][1];
            Ut[cur][r][c4 + 2] = un[h][2];
            Ut[cur][r][c4 + 3] = un[h][3];
        }
        float a[2][16];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int t = 0; t < 16; ++t) a[bi][t] = an[bi][t >> 2][t & 3];
        __syncthreads();
        if (kk + 64 < kend) gload(kk + 64);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            float bv[2];
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) bv[bj] = Ut[cur][kq * 16 + t][32 * wc + 16 * bj + r16];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[bi][t], bv[bj],
                                                                       acc[bi][bj], 0, 0, 0);
        }
    }
}

// The same product on v_mfma_f64_16x16x4_f64 (C/D lane l, reg r -> row F64_CROW(l, r), col l&15)
// from the slot's fp64 factor and the fp64 U buffer. The wide slots it serves are rare (extreme
// theta), so plainly staged: L and U slices of 16 through LDS, two barriers per slice.
__device__ __forceinline__ void ugemm_tile64(d4_t (&acc)[2][2], const double* L, const double* U,
                                             int np, int sp, int i, int sb, double (&La)[64][17],
                                             double (&Ub)[16][65]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = d4_t{0.0, 0.0, 0.0, 0.0};
    const int kend = (i + 1) * 64;
    for (int kk = 0; kk < kend; kk += 16) {
        for (int e = tid; e < 64 * 16; e += 256) {
            const int r = e >> 4, c = e & 15;
            La[r][c] = L[(int64_t)(i * 64 + r) * np + kk + c];
            Ub[e >> 6][e & 63] = U[(int64_t)(kk + (e >> 6)) * sp + sb * 64 + (e & 63)];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
                    acc[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                        La[32 * wr + 16 * bi + r16][4 * t + kq],
                        Ub[4 * t + kq][32 * wc + 16 * bj + r16], acc[bi][bj], 0, 0, 0);
        }
        __syncthreads();
    }
}

// f = f_post + acc in fp64, in the accumulator's own layout: f[bi][bj][r] is the tile's row
// 32 wr + 16 bi + CROW(lane, r), column 32 wc + 16 bj + (lane & 15). fp: the slot's f_post.
template <bool F64MAP, typename ACC>
__device__ __forceinline__ void ugemm_add_fpost(double (&f)[2][2][4], const ACC (&acc)[2][2],
                                                const double* fp, int i) {
    const int lane = threadIdx.x & 63, wr = threadIdx.x >> 7;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double fr = fp[i * 64 + 32 * wr + 16 * bi +
                                 (F64MAP ? F64_CROW(lane, r) : F32_CROW(lane, r))];
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) f[bi][bj][r] = fr + (double)acc[bi][bj][r];
        }
}
