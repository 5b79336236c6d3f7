// The fp64 64x64 tile product on v_mfma_f64_16x16x4_f64 (tile_gemm_nt, the routine
// apm_selftest_tile pins) with its accumulator load / store, shared by the kernels of chol.hip
// and the importance-sampling predictive GEMM (is_predict.hip).
#pragma once
#include "apm_common.h"

// v_mfma_f64_16x16x4_f64 operand/result maps (cdna_hip_programming.md §3):
//   A: lane l holds A[row = l&15][k = l>>4]; B: lane l holds B[k = l>>4][col = l&15]
//   C/D: lane l, reg r  ->  row = (l>>4) + 4r, col = l&15
#define F64_CROW(l, r) (((l) >> 4) + 4 * (r))

__device__ __forceinline__ void tile_acc_load(d4_t (&acc)[2][2], const double* T, int64_t ld,
                                              int wr, int wc, int lane) {
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[bi][bj][r] = T[(int64_t)(32 * wr + 16 * bi + F64_CROW(lane, r)) * ld +
                                   32 * wc + 16 * bj + (lane & 15)];
}

__device__ __forceinline__ void tile_acc_store(const d4_t (&acc)[2][2], double* T, int64_t ld,
                                               int wr, int wc, int lane) {
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                T[(int64_t)(32 * wr + 16 * bi + F64_CROW(lane, r)) * ld + 32 * wc + 16 * bj +
                  (lane & 15)] = acc[bi][bj][r];
}

#ifndef UPD_ABL
#define UPD_ABL 0
#endif
#ifndef UPD_WPE
#define UPD_WPE 3  // min waves per SIMD for k_chol_update (caps VGPRs at 168)
#endif
#ifndef UPD_PF
#define UPD_PF 2   // slices of global loads in flight (1 or 2)
#endif
#ifndef UPD_LATEC
#define UPD_LATEC 1  // load the old tile behind the first slices and add it at the end
#endif
#ifndef UPD_KS
#define UPD_KS 16
#endif
#define KSUB UPD_KS
#define LPITCH (UPD_KS + 1)
struct GemmSmem {
    double a[2][64][LPITCH];
    double b[2][64][LPITCH];
};

// acc += (NEG ? -1 : 1) * A[64 x depth] * B[64 x depth]^T (+ the tile C, if given) for the
// workgroup's 64x64 tile. Operands are staged through LDS in KS-deep slices shared by the four
// waves, double-buffered, with TWO slices of global loads in flight (register sets alternate with
// the slice parity; loads are unconditional - clamped to the last slice - so the compiler's
// vmcnt waits count exactly and never drain the newer set). The old C tile, when given, is loaded
// behind the first two slices and added at the end, off the critical path of the first MFMA.
// One barrier per slice; LDS pitch KS+1 keeps the fragment reads bank-conflict free.
template <bool NEG>
__device__ __forceinline__ void tile_gemm_nt(d4_t (&acc)[2][2], const double* __restrict__ A,
                                             int64_t lda, const double* __restrict__ B,
                                             int64_t ldb, int depth, GemmSmem& sm,
                                             const double* __restrict__ C = nullptr,
                                             int64_t ldc = 0) {
    constexpr int PPR = KSUB / 2;          // 16-byte pieces per row of a slice
    constexpr int PPT = 64 * PPR / 256;    // pieces per thread per operand
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int r16 = lane & 15, kq = lane >> 4;
    int prow[PPT], pcol[PPT];
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
        const int p = tid + 256 * h;
        prow[h] = p / PPR;
        pcol[h] = (p % PPR) * 2;
    }
    auto gload = [&](int sidx, d2_t (&ra)[PPT], d2_t (&rb)[PPT]) {
#if UPD_ABL == 1  // ablation (tools/upd_bench.cpp): operands always slice 0 (L1/L2 resident)
        sidx = 0;
#endif
#pragma unroll
        for (int h = 0; h < PPT; ++h) {
            const int kc = sidx * KSUB + pcol[h];
            ra[h] = *reinterpret_cast<const d2_t*>(A + (int64_t)prow[h] * lda + kc);
            rb[h] = *reinterpret_cast<const d2_t*>(B + (int64_t)prow[h] * ldb + kc);
        }
    };
    auto sstore = [&](int buf, const d2_t (&ra)[PPT], const d2_t (&rb)[PPT]) {
#pragma unroll
        for (int h = 0; h < PPT; ++h) {
            sm.a[buf][prow[h]][pcol[h]] = NEG ? -ra[h].x : ra[h].x;
            sm.a[buf][prow[h]][pcol[h] + 1] = NEG ? -ra[h].y : ra[h].y;
            sm.b[buf][prow[h]][pcol[h]] = rb[h].x;
            sm.b[buf][prow[h]][pcol[h] + 1] = rb[h].y;
        }
    };
    auto compute = [&](int cur) {
#pragma unroll
        for (int t = 0; t < KSUB / 4; ++t) {
            double a[2], b[2];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) a[bi] = sm.a[cur][32 * wr + 16 * bi + r16][4 * t + kq];
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) b[bj] = sm.b[cur][32 * wc + 16 * bj + r16][4 * t + kq];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
#if UPD_ABL == 2  // ablation: no MFMA (memory + LDS + barrier pipeline only)
                    acc[bi][bj][0] += a[bi] * b[bj];
#else
                    acc[bi][bj] =
                        __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], b[bj], acc[bi][bj], 0, 0, 0);
#endif
        }
    };
    const int nsub = depth / KSUB;  // even: depth is a multiple of 64 and KS <= 32
    d4_t old[2][2];
#if UPD_PF == 2
    d2_t ra0[PPT], rb0[PPT], ra1[PPT], rb1[PPT];
    gload(0, ra0, rb0);
    gload(1, ra1, rb1);
    if (C) tile_acc_load(old, C, ldc, wr, wc, lane);
    sstore(0, ra0, rb0);
    __syncthreads();
    for (int s = 0; s < nsub; s += 2) {
        gload(min(s + 2, nsub - 1), ra0, rb0);
        compute(0);
        sstore(1, ra1, rb1);
        __syncthreads();
        gload(min(s + 3, nsub - 1), ra1, rb1);
        compute(1);
        sstore(0, ra0, rb0);  // past the end: a clamped reload into a buffer no longer read
        __syncthreads();
    }
#else
    d2_t ra0[PPT], rb0[PPT];
    gload(0, ra0, rb0);
    if (C) tile_acc_load(old, C, ldc, wr, wc, lane);
    sstore(0, ra0, rb0);
    __syncthreads();
    for (int s = 0; s < nsub; ++s) {
        gload(min(s + 1, nsub - 1), ra0, rb0);
        compute(s & 1);
        sstore((s + 1) & 1, ra0, rb0);
        __syncthreads();
    }
#endif
    if (C) {
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) acc[bi][bj] += old[bi][bj];
    }
}
