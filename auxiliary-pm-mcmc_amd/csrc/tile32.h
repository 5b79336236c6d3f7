// fp32 / fp16x3 tile primitives shared by the fp32 factorisation's kernels (chol32_update.hip,
// chol32_panel.hip): the 64x64 tile GEMM on LDS-staged slices, the hi/lo split of fp32 operands
// into fp16 pairs, their operand planes (Planes16) and the fragment product on them.
#pragma once
#include "apm_internal.h"

#define KS32 32          // slice depth (floats) of the LDS-staged tile GEMM
#define LP32 (KS32 + 2)  // pitch 34 floats: fragment reads (16 rows x 4 k) hit 32 distinct banks
// fp16x3 operands (see k_chol_update32_t128): hi and lo halves of a 32-deep slice, 64-byte rows
// (four 16-byte pieces) with the piece index XOR-swizzled by bit 3 of the row (HS): the 16-byte
// fragment reads of an MFMA (lane = row r16 + 16 x, piece kq) then hit 16 distinct bank quads in
// every ds_read_b128 lane group, and the 8-byte stores of two consecutive rows fill the 32
// banks of a ds_write_b64 group once (the round-4 80-byte pitch left 2-way read conflicts: 48 %
// of the update's LDS cycles, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, profiles/r05_pmc_newton.txt)
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
#define LPH 32
#define HS(r, c) (((((c) >> 3) ^ (((r) >> 2) & 2)) << 3) | ((c) & 7))
struct GemmSmem32 {
    union {
        struct {
            float a[2][64][LP32];
            float b[2][64][LP32];
        };
        struct {
            _Float16 ah[2][64][LPH], al[2][64][LPH];
            _Float16 bh[2][64][LPH], bl[2][64][LPH];
        };
    };
};
// x = hi + lo with hi = fp16(x), lo = fp16(x - hi): 22 of fp32's 24 mantissa bits
__device__ __forceinline__ void split_h3(float v, _Float16& hi, _Float16& lo) {
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}
__device__ __forceinline__ void split_h3(const f4_t& v, h4_t& hi, h4_t& lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 h, l;
        split_h3(v[e], h, l);
        hi[e] = h;
        lo[e] = l;
    }
}
// 8 consecutive values (one 16-byte piece of each plane)
__device__ __forceinline__ void split_h3(const f4_t& v0, const f4_t& v1, h8_t& hi, h8_t& lo) {
    h4_t h0, l0, h1, l1;
    split_h3(v0, h0, l0);
    split_h3(v1, h1, l1);
    hi = h8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    lo = h8_t{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
}
// one value into operand planes (Planes16: fp16 bit patterns, the lo plane `lo` entries on):
// at p, or as row r, column c of the planes at P
__device__ __forceinline__ void plane_put(unsigned short* p, int64_t lo, float v) {
    _Float16 h, l;
    split_h3(v, h, l);
    p[0] = __builtin_bit_cast(unsigned short, h);
    p[lo] = __builtin_bit_cast(unsigned short, l);
}
__device__ __forceinline__ void plane_put(unsigned short* P, const Planes16& pl, int r, int c,
                                          float v) {
    plane_put(P + ((int64_t)(c >> 5) * pl.rows + r) * 32 + (c & 31), pl.lo, v);
}
// v_mfma_f32_16x16x4_f32: A lane l holds A[l&15][k=l>>4], B holds B[k=l>>4][l&15];
// D reg r of lane l is (row 4*(l>>4) + r, col l&15)  (cdna_hip_programming.md §3)
#define F32_CROW(l, r) (4 * ((l) >> 4) + (r))

__device__ __forceinline__ void tile32_load(f4_t (&acc)[2][2], const float* T, int64_t ld, int wr,
                                            int wc, int lane) {
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[bi][bj][r] = T[(int64_t)(32 * wr + 16 * bi + F32_CROW(lane, r)) * ld +
                                   32 * wc + 16 * bj + (lane & 15)];
}

__device__ __forceinline__ void tile32_store(const f4_t (&acc)[2][2], float* T, int64_t ld,
                                             int wr, int wc, int lane) {
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                T[(int64_t)(32 * wr + 16 * bi + F32_CROW(lane, r)) * ld + 32 * wc + 16 * bj +
                  (lane & 15)] = acc[bi][bj][r];
}

// acc[bi][bj] += A_bi B_bj^T over one 32-deep slice in fp16x3, for the NBI x NBJ blocks of
// 16 x 16 at rows arow0 + 16 bi of the A planes ah / al and rows brow0 + 16 bj of the B planes
// bh / bl ([row][LPH], HS layout). Lane (r16, kq) holds k = 8kq .. 8kq+7 of the slice: one
// 16-byte read per plane and block row; the B fragments stay in registers, the A fragments are
// read per block row. Per block the products are hi hi, hi lo, lo hi, in that order, block rows
// outermost: the order every fp16x3 path shares, which is what makes their tiles bitwise equal.
// skip0 / skip1: block rows 0 .. 3 / 4 .. 7 are left out (a dropped output tile).
template <int NBI, int NBJ = 4>
__device__ __forceinline__ void h3_mma(f4_t (&acc)[NBI][NBJ], const _Float16 (*ah)[LPH],
                                       const _Float16 (*al)[LPH], const _Float16 (*bh)[LPH],
                                       const _Float16 (*bl)[LPH], int arow0, int brow0, int r16,
                                       int kq, bool skip0 = false, bool skip1 = false) {
    h8_t fbh[NBJ], fbl[NBJ];
#pragma unroll
    for (int x = 0; x < NBJ; ++x) {
        const int row = brow0 + 16 * x + r16;
        fbh[x] = *reinterpret_cast<const h8_t*>(&bh[row][HS(row, 8 * kq)]);
        fbl[x] = *reinterpret_cast<const h8_t*>(&bl[row][HS(row, 8 * kq)]);
    }
#pragma unroll
    for (int bi = 0; bi < NBI; ++bi) {
        if (bi < 4 ? skip0 : skip1) continue;
        const int row = arow0 + 16 * bi + r16;
        const h8_t fah = *reinterpret_cast<const h8_t*>(&ah[row][HS(row, 8 * kq)]);
        const h8_t fal = *reinterpret_cast<const h8_t*>(&al[row][HS(row, 8 * kq)]);
#pragma unroll
        for (int bj = 0; bj < NBJ; ++bj) {
            acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fah, fbh[bj], acc[bi][bj], 0, 0, 0);
            acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fah, fbl[bj], acc[bi][bj], 0, 0, 0);
            acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fal, fbh[bj], acc[bi][bj], 0, 0, 0);
        }
    }
}

// acc += (NEG ? -1 : 1) * A[64 x depth] * B[64 x depth]^T (+ C if given): the fp32 twin of
// chol.hip's tile_gemm_nt (two slices of loads in flight, double-buffered LDS, one barrier per
// slice, the old tile loaded behind the first slices and added at the end). H3: fp16x3 operands
// on v_mfma_f32_16x16x32_f16 (as k_chol_update32_t128).
template <bool NEG, bool H3 = false>
__device__ __forceinline__ void tile_gemm_nt32(f4_t (&acc)[2][2], const float* __restrict__ A,
                                               int64_t lda, const float* __restrict__ B,
                                               int64_t ldb, int depth, GemmSmem32& sm,
                                               const float* __restrict__ C, int64_t ldc) {
    constexpr int PPR = KS32 / 4;        // 16-byte pieces per slice row
    constexpr int PPT = 64 * PPR / 256;  // pieces per thread per operand
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int r16 = lane & 15, kq = lane >> 4;
    int prow[PPT], pcol[PPT];
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
        const int p = tid + 256 * h;
        prow[h] = p / PPR;
        pcol[h] = (p % PPR) * 4;
    }
    auto gload = [&](int sidx, f4_t (&ra)[PPT], f4_t (&rb)[PPT]) {
#pragma unroll
        for (int h = 0; h < PPT; ++h) {
            const int kc = sidx * KS32 + pcol[h];
            ra[h] = *reinterpret_cast<const f4_t*>(A + (int64_t)prow[h] * lda + kc);
            rb[h] = *reinterpret_cast<const f4_t*>(B + (int64_t)prow[h] * ldb + kc);
        }
    };
    auto sstore = [&](int buf, const f4_t (&ra)[PPT], const f4_t (&rb)[PPT]) {
        if constexpr (H3) {
#pragma unroll
            for (int h = 0; h < PPT; ++h) {
                h4_t hi, lo;
                split_h3(NEG ? -ra[h] : ra[h], hi, lo);
                *reinterpret_cast<h4_t*>(&sm.ah[buf][prow[h]][HS(prow[h], pcol[h])]) = hi;
                *reinterpret_cast<h4_t*>(&sm.al[buf][prow[h]][HS(prow[h], pcol[h])]) = lo;
                split_h3(rb[h], hi, lo);
                *reinterpret_cast<h4_t*>(&sm.bh[buf][prow[h]][HS(prow[h], pcol[h])]) = hi;
                *reinterpret_cast<h4_t*>(&sm.bl[buf][prow[h]][HS(prow[h], pcol[h])]) = lo;
            }
            return;
        }
#pragma unroll
        for (int h = 0; h < PPT; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sm.a[buf][prow[h]][pcol[h] + e] = NEG ? -ra[h][e] : ra[h][e];
                sm.b[buf][prow[h]][pcol[h] + e] = rb[h][e];
            }
    };
    auto compute = [&](int cur) {
        if constexpr (H3) {
            h3_mma<2, 2>(acc, sm.ah[cur], sm.al[cur], sm.bh[cur], sm.bl[cur], 32 * wr, 32 * wc,
                         r16, kq);
            return;
        }
#pragma unroll
        for (int t = 0; t < KS32 / 4; ++t) {
            float a[2], b[2];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) a[bi] = sm.a[cur][32 * wr + 16 * bi + r16][4 * t + kq];
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) b[bj] = sm.b[cur][32 * wc + 16 * bj + r16][4 * t + kq];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
                    acc[bi][bj] =
                        __builtin_amdgcn_mfma_f32_16x16x4f32(a[bi], b[bj], acc[bi][bj], 0, 0, 0);
        }
    };
    const int nsub = depth / KS32;  // even: depth is a multiple of 64
    f4_t ra0[PPT], rb0[PPT], ra1[PPT], rb1[PPT];
    gload(0, ra0, rb0);
    gload(1, ra1, rb1);
    f4_t old[2][2];
    if (C) tile32_load(old, C, ldc, wr, wc, lane);
    sstore(0, ra0, rb0);
    __syncthreads();
    for (int s = 0; s < nsub; s += 2) {
        gload(min(s + 2, nsub - 1), ra0, rb0);
        compute(0);
        sstore(1, ra1, rb1);
        __syncthreads();
        gload(min(s + 3, nsub - 1), ra1, rb1);
        compute(1);
        sstore(0, ra0, rb0);
        __syncthreads();
    }
    if (C) {
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) acc[bi][bj] += old[bi][bj];
    }
}

// tile32_store written through to memory (sc1): the dataflow panel's published tiles
__device__ __forceinline__ void tile32_store_sc1(const f4_t (&acc)[2][2], float* T, int64_t ld,
                                                 int wr, int wc, int lane) {
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                __hip_atomic_store(T + (int64_t)(32 * wr + 16 * bi + F32_CROW(lane, r)) * ld +
                                       32 * wc + 16 * bj + (lane & 15),
                                   acc[bi][bj][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------- the 128- and 256-row fp16x3 kernels
#define KS128 32  // their slice depth

// LDS-DMA staging of operand planes (Planes16): a 16-byte global_load_lds moves 16 rows x 64 B
// per wave; lane l takes row l/4 of the group and stores LDS slot l%4, i.e. logical piece
// (l%4) ^ (bit 3 of the row) - the HS layout that h3_mma reads. plane_lane_off: the lane's
// offset (entries) from the group's first row in the plane.
__device__ __forceinline__ int plane_lane_off(int lane) {
    const int rowl = lane >> 2, piece = (lane & 3) ^ ((rowl >> 2) & 2);
    return rowl * 32 + piece * 8;
}
// one plane's slice of two row tiles (64 rows each, at p0 and p1, plane_lane_off included) into
// the 128 rows at lds: 8 loads, no registers, no VALU
__device__ __forceinline__ void stage_planes(const unsigned short* p0, const unsigned short* p1,
                                             _Float16* lds) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
        __builtin_amdgcn_global_load_lds((glb_void_t*)((q < 4 ? p0 : p1) + (16 * (q & 3)) * 32),
                                         (lds_void_t*)(lds + 16 * q * LPH), 16, 0, 0);
}
