// The trailing updates of the fp32 factorisations (the Newton matrix, the posterior factor's
// bottom block) on 64x64 tiles, 128x128 super-tiles and 256x256 quad tiles, over the lists of
// tile_lists.cpp.
#include "apm_internal.h"
#include "diag.h"
#include "tile32.h"

// The work item of an update workgroup: update_item (update_item.h); the fused diagonal step on
// entry 0 of a fused launch: fused_diag (diag.h).
__global__ __launch_bounds__(256) void k_chol_update32(MatF A, int k0, int kc,
                                                       const unsigned* __restrict__ tiles,
                                                       int ntiles, int nchains, Live live,
                                                       FusedDiag<float> fd, int hlim,
                                                       const int* __restrict__ h3ok) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1;
    __shared__ union {
        GemmSmem32 g;
        DiagSmem32 d;
    } sm;
    const UpdateItem it = update_item((long)blockIdx.x, fd.enabled, ntiles, nchains);
    const int b = it.b;
    if (!live_chain(live, b)) return;
    const Tile64 e(tiles[it.t]);
    const int i = e.i(), j = e.j();
    float* Ab = A.base + b * A.cstride;
    float* Aij = Ab + (int64_t)(i * 64) * A.ld + j * 64;
    f4_t acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};
    // fp16x3 below the appended right-hand-side row tile, per chain (k_chol_update32_t128)
    if (i < hlim && (!h3ok || h3ok[b]))
        tile_gemm_nt32<true, true>(acc, Ab + (int64_t)(i * 64) * A.ld + k0 * 64, A.ld,
                                   Ab + (int64_t)(j * 64) * A.ld + k0 * 64, A.ld, 64 * kc, sm.g,
                                   Aij, A.ld);
    else
        tile_gemm_nt32<true>(acc, Ab + (int64_t)(i * 64) * A.ld + k0 * 64, A.ld,
                             Ab + (int64_t)(j * 64) * A.ld + k0 * 64, A.ld, 64 * kc, sm.g, Aij,
                             A.ld);
    if (!it.fused) {
        tile32_store(acc, Aij, A.ld, wr, wc, lane);
        return;
    }
    tile32_store(acc, sm.d.T, DP, wr, wc, lane);
    fused_diag(sm.d, Aij, A.ld, b, i, fd, live);
}

void launch_chol_update32(MatF A, int k0, int kc, const unsigned* tiles, int ntiles, Live live,
                          int nchains, hipStream_t s, FusedDiag<float> fd, int hlim,
                          const int* h3ok) {
    if (ntiles <= 0) return;
    const long total = (long)ntiles * nchains;
    APM_LAUNCH(k_chol_update32, dim3((unsigned)total), dim3(256), 0, s, A, k0, kc, tiles,
                       ntiles, nchains, live, fd, hlim, h3ok);
}

// ------------------------------------------------------------------------- 128x128 trailing update
// The rank-64*kc outer updates with one 128x128 super-tile (2x2 tiles) per workgroup: each wave
// owns a 64x64 tile (4x4 v_mfma_f32_16x16x4_f32 accumulators), so a slice of operands staged in
// LDS feeds twice the MFMAs of the 64x64 kernel per byte loaded (8 instead of 16 B/clk/CU of
// L2->LDS traffic at the MFMA rate: the 64x64 kernel is operand-load bound).
// Super-tile entries: build_update_supertiles (tile_lists.cpp). Invalid halves load a valid
// half's operands (no out-of-range reads) and their results are dropped.
struct __attribute__((aligned(16))) GemmSmem128 {  // fp32 operands, LDS-DMA image
    float a[2][128][KS128];
    float b[2][128][KS128];
};
struct __attribute__((aligned(16))) GemmSmemH3 {
    _Float16 ah[2][128][LPH], al[2][128][LPH];
    _Float16 bh[2][128][LPH], bl[2][128][LPH];
};

// H3 = false: fp32 operands through LDS-DMA (v_mfma_f32_16x16x4_f32).
// H3 = true ("fp16x3"): each fp32 operand x is split into x_hi = fp16(x), x_lo = fp16(x - x_hi)
// while it is staged, and A B^T = A_hi B_hi^T + A_hi B_lo^T + A_lo B_hi^T on
// v_mfma_f32_16x16x32_f16 (fp32 accumulation): 3 MFMAs of 16 cycles replace 8 f32 MFMAs of 32
// cycles per 16x16x32 block, at the same operand bytes (2 x fp16 = fp32). The split keeps 22 of
// fp32's 24 mantissa bits (product error ~2.4e-7 relative, ~4x fp32's): measured on Newton
// matrices (numpy emulation, N = 1024, sigma = 1 .. e^4) the factor's residual |LL^T - B| is
// unchanged and the refinement contraction rises from ~3e-6 to ~1e-5, far below the 1e-3 of the
// acceptance test. fp16's range bounds the operands (entries of L, |L_ij| <= sqrt(B_ii) <=
// sqrt(B_ii) = sqrt(1 + W_i K_ii) <= sqrt(1 + e^theta_0 + eps): probit W < 1, logit W <= 1/4): the host flags
// the chains with theta_0 < 19 (entries < 1.4e4 < 65504) in h3ok; the others take the fp32
// path inside the same launch, so a chain's result does not depend on its batch. The appended
// right-hand-side row (forward solve of W^1/2 K b, unbounded) stays fp32: super-tiles reaching
// row tile hlim take the fp32 path.

// Update of the appended right-hand-side row tile of the Newton matrix, whose first row alone
// holds data (k_symv_reduce zeroes the other 63): C[0][c] -= sum_k A[0][k] B[c][k] for the 64 or
// 128 columns c of the super-tile, as row-vector products instead of a 64-row MFMA tile (which
// also had to take fp32 operands: the row is not bounded like the entries of L). Wave w takes 32
// of the 128 columns, 4 at a time; lane l multiplies k = 4l + 256q .. +3 (16-byte loads, each
// B row read as one contiguous 64-lane access), fp64 accumulation, butterfly reduction - a fixed
// order, so the result does not depend on the schedule.
__device__ __forceinline__ void rhs_row_update32(float* Ab, int64_t ld, int ti, int tj, bool cv0,
                                                 bool cv1, int k0, int kc, int tid) {
    const int lane = tid & 63, w = tid >> 6;
    if (!(w < 2 ? cv0 : cv1)) return;
    const int K = 64 * kc;  // <= 64 * 14 (OUTER32 is clamped to 14 tiles: apm_host.h apm_ctx::outer32)
    constexpr int QM = 4;
    float* crow = Ab + (int64_t)(ti * 64) * ld;
    const float* arow = crow + k0 * 64;
    f4_t a[QM];
#pragma unroll
    for (int q = 0; q < QM; ++q)
        a[q] = (4 * lane + 256 * q < K) ? *reinterpret_cast<const f4_t*>(arow + 4 * lane + 256 * q)
                                        : f4_t{0.f, 0.f, 0.f, 0.f};
    const int c0 = (w < 2 ? tj * 64 : (tj + 1) * 64) + 32 * (w & 1);
#pragma unroll 1
    for (int r0 = 0; r0 < 32; r0 += 4) {
        f4_t v[4][QM];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float* brow = Ab + (int64_t)(c0 + r0 + rr) * ld + k0 * 64 + 4 * lane;
#pragma unroll
            for (int q = 0; q < QM; ++q)
                v[rr][q] = (4 * lane + 256 * q < K) ? *reinterpret_cast<const f4_t*>(brow + 256 * q)
                                                    : f4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < QM; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fma((double)a[q][e], (double)v[rr][q][e], s);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
            if (lane == rr) {
                float* cp = crow + c0 + r0 + rr;
                *cp = (float)((double)*cp - s);
            }
        }
    }
}
// The right-hand-side row beside the quad-tile kernel, whose lists stop above it: the super-tiles
// of that row alone (build_update_supertiles(nb, nb + 1, ..., solo = nb)), one per workgroup.
__global__ __launch_bounds__(256) void k_rhs_row_update32(MatF A, int k0, int kc,
                                                          const unsigned* __restrict__ tiles,
                                                          int ntiles, int nchains, Live live) {
    const long w = xcd_remap((long)blockIdx.x, (long)ntiles * nchains);
    const int b = (int)(w / ntiles);
    if (!live_chain(live, b)) return;
    const SuperTile e(tiles[w % ntiles]);
    rhs_row_update32(A.base + b * A.cstride, A.ld, e.i(), e.j(), e.cv(0), e.cv(1), k0, kc,
                     threadIdx.x);
}

void launch_rhs_row_update32(MatF A, int k0, int kc, const unsigned* tiles, int ntiles, Live live,
                             int nchains, hipStream_t s) {
    if (ntiles <= 0) return;
    APM_LAUNCH(k_rhs_row_update32, dim3((unsigned)((long)ntiles * nchains)), dim3(256), 0, s, A,
               k0, kc, tiles, ntiles, nchains, live);
}

// ROLE (UPD32_*, apm_internal.h) 0: the Newton factorisation, 1: the posterior factor's bottom
// block (postcov.hip; the same code, a separate instantiation so that the two launch populations
// get separate rocprofv3 counter figures), 2: the Newton factorisation with the fp16x3 operands
// read from the dataflow kernel's planes (Planes16) instead of split while staged
template <bool H3, int ROLE>
__global__ __launch_bounds__(256, 2) void k_chol_update32_t128(MatF A, int k0, int kc,
                                                               const unsigned* __restrict__ tiles,
                                                               int ntiles, int nchains, Live live,
                                                               FusedDiag<float> fd, int hlim,
                                                               const int* __restrict__ h3ok,
                                                               int rhs, Planes16 pl) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const int r16 = lane & 15, kq = lane >> 4;
    __shared__ union {
        GemmSmem128 g;
        GemmSmemH3 h;
        DiagSmem32 d;
    } sm;
    const UpdateItem it = update_item((long)blockIdx.x, fd.enabled, ntiles, nchains);
    const int b = it.b;
    const bool fused = it.fused;
    if (!live_chain(live, b)) return;
    const SuperTile e(tiles[it.t]);
    const int ti = e.i(), tj = e.j();
    // operand row tiles of the two halves (an invalid half reuses the valid one)
    const int ra0 = e.ra0(), ra1 = e.ra1(), cb0 = e.cb0(), cb1 = e.cb1();
    float* Ab = A.base + b * A.cstride;
    if (ti == rhs) {  // the right-hand-side row alone (its super-tile row holds no other tile)
        rhs_row_update32(Ab, A.ld, ti, tj, e.cv(0), e.cv(1), k0, kc, tid);
        return;
    }
    // this wave's output tile
    const int oi = ti + wr, oj = tj + wc;
    const bool mine = e.writes(wr, wc);

    f4_t acc[4][4];
    const int nsub = (64 * kc) / KS128;
    const int li = mine ? oi : (wr ? ra1 : ra0), lj = mine ? oj : (wc ? cb1 : cb0);
    const float* Cw = Ab + (int64_t)(li * 64) * A.ld + lj * 64;
    auto load_old = [&]() {
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
            for (int bj = 0; bj < 4; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[bi][bj][r] =
                        -Cw[(int64_t)(16 * bi + F32_CROW(lane, r)) * A.ld + 16 * bj + r16];
    };
    // super-tile rows below hlim (the appended right-hand side row), chains flagged in h3ok
    const bool use_h3 = H3 && ti + (e.rv(1) ? 1 : 0) < hlim && (!h3ok || h3ok[b]);
    if (!(ROLE == UPD32_NEWTON_PLANES && use_h3)) load_old();
    // one staged slice of the fp16x3 product: this wave's 4 x 4 blocks
    auto compute_h3 = [&](int cur) {
        h3_mma<4>(acc, sm.h.ah[cur], sm.h.al[cur], sm.h.bh[cur], sm.h.bl[cur], 64 * wr, 64 * wc,
                  r16, kq);
    };
    if (ROLE == UPD32_NEWTON_PLANES && use_h3) {
        // operands already split by the dataflow panel kernel (Planes16): wave wv fills one
        // array (0: A hi, 1: A lo, 2: B hi, 3: B lo) of a slice by LDS-DMA (stage_planes)
        const unsigned short* P = pl.base + b * pl.cstride + ((wv & 1) ? pl.lo : 0) +
                                  plane_lane_off(lane);
        const unsigned short* p0 = P + (int64_t)(wv < 2 ? ra0 : cb0) * 64 * 32;
        const unsigned short* p1 = P + (int64_t)(wv < 2 ? ra1 : cb1) * 64 * 32;
        const int64_t sstep = (int64_t)pl.rows * 32;
        _Float16* lbase = &sm.h.ah[0][0][0] + wv * (2 * 128 * LPH);
        auto dma = [&](int sidx, int buf) {
            stage_planes(p0 + sidx * sstep, p1 + sidx * sstep, lbase + buf * 128 * LPH);
        };
        dma(0, 0);
        load_old();  // while the first slice is in flight
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) asm volatile("" : "+v"(acc[bi][bj]));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int s = 0; s < nsub; ++s) {
            if (s + 1 < nsub) dma(s + 1, (s + 1) & 1);  // lands while slice s is multiplied
            if (mine) compute_h3(s & 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    } else if (ROLE != UPD32_NEWTON_PLANES && use_h3) {
        // register staging: thread tid moves 16-byte pieces p = tid + 256h (row p/8, k 4(p%8))
        // of both operands
        const float* arow[4];
        const float* brow[4];
        int prow[4], pcol[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int p = tid + 256 * h;
            prow[h] = p >> 3;
            pcol[h] = (p & 7) * 4;
            const int rt = prow[h] < 64 ? ra0 : ra1, ct = prow[h] < 64 ? cb0 : cb1;
            arow[h] = Ab + (int64_t)(rt * 64 + (prow[h] & 63)) * A.ld + k0 * 64 + pcol[h];
            brow[h] = Ab + (int64_t)(ct * 64 + (prow[h] & 63)) * A.ld + k0 * 64 + pcol[h];
        }
        auto gload = [&](int sidx, f4_t (&ra)[4], f4_t (&rb)[4]) {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                ra[h] = *reinterpret_cast<const f4_t*>(arow[h] + sidx * KS128);
                rb[h] = *reinterpret_cast<const f4_t*>(brow[h] + sidx * KS128);
            }
        };
        auto sstore = [&](int buf, const f4_t (&ra)[4], const f4_t (&rb)[4]) {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                h4_t hi, lo;
                split_h3(ra[h], hi, lo);
                *reinterpret_cast<h4_t*>(&sm.h.ah[buf][prow[h]][HS(prow[h], pcol[h])]) = hi;
                *reinterpret_cast<h4_t*>(&sm.h.al[buf][prow[h]][HS(prow[h], pcol[h])]) = lo;
                split_h3(rb[h], hi, lo);
                *reinterpret_cast<h4_t*>(&sm.h.bh[buf][prow[h]][HS(prow[h], pcol[h])]) = hi;
                *reinterpret_cast<h4_t*>(&sm.h.bl[buf][prow[h]][HS(prow[h], pcol[h])]) = lo;
            }
        };
        // one slice in flight in registers (the 3 MFMAs per block leave the loop operand-bound:
        // a second slice would cost 32 VGPRs and the second workgroup per CU)
        f4_t ra[4], rb[4];
        gload(0, ra, rb);
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) asm volatile("" : "+v"(acc[bi][bj]));
        sstore(0, ra, rb);
        __syncthreads();
        for (int s = 0; s < nsub; ++s) {
            if (s + 1 < nsub) gload(s + 1, ra, rb);
            if (mine) compute_h3(s & 1);  // a wave whose tile is dropped only stages
            if (s + 1 < nsub) sstore((s + 1) & 1, ra, rb);
            __syncthreads();
        }
    } else {
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) asm volatile("" : "+v"(acc[bi][bj]));
        // LDS-DMA staging (the fp32 twin of chol.hip's k_chol_update_t128): wave wv moves operand rows
        // 32wv .. 32wv+31 of a 32-deep slice (4 global_load_lds_dwordx4 of 8 rows x 128 B); lane l
        // takes row +l/8 and stores slot l%8, i.e. global piece (l%8) ^ (l/8): the 16-byte fragment
        // reads of 8 consecutive rows hit distinct banks. No staging registers, no ds_write pass; the
        // sign of A_ij -= A_ik A_jk^T is applied to the old tile (acc = -C + sum, result = -acc).
        const int srow = 32 * wv + (lane >> 3);
        const int spiece = (lane & 7) ^ (lane >> 3);
        const int64_t ld8 = 8 * A.ld;
        const float* ga = Ab + (int64_t)((wv < 2 ? ra0 : ra1) * 64 + (srow & 63)) * A.ld + k0 * 64 +
                          4 * spiece;
        const float* gb = Ab + (int64_t)((wv < 2 ? cb0 : cb1) * 64 + (srow & 63)) * A.ld + k0 * 64 +
                          4 * spiece;
        auto glds = [&](int sidx, int buf) {
            const int o = sidx * KS128;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __builtin_amdgcn_global_load_lds((glb_void_t*)(ga + q * ld8 + o),
                                                 (lds_void_t*)&sm.g.a[buf][32 * wv + 8 * q][0], 16, 0, 0);
                __builtin_amdgcn_global_load_lds((glb_void_t*)(gb + q * ld8 + o),
                                                 (lds_void_t*)&sm.g.b[buf][32 * wv + 8 * q][0], 16, 0, 0);
            }
        };
        // lane group kq takes the slice's k values 8kq .. 8kq+7 (pieces 2kq, 2kq+1; the same k for A
        // and B): a lane's fragments for 4 MFMA steps are one 16-byte LDS read
        auto compute = [&](int cur) {
#pragma unroll
            for (int h = 0; h < KS128 / 16; ++h) {
                const int sl = ((2 * kq + h) ^ (r16 & 7)) * 4;
                f4_t a4[4], b4[4];
#pragma unroll
                for (int bi = 0; bi < 4; ++bi)
                    a4[bi] = *reinterpret_cast<const f4_t*>(&sm.g.a[cur][64 * wr + 16 * bi + r16][sl]);
#pragma unroll
                for (int bj = 0; bj < 4; ++bj)
                    b4[bj] = *reinterpret_cast<const f4_t*>(&sm.g.b[cur][64 * wc + 16 * bj + r16][sl]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
                        for (int bj = 0; bj < 4; ++bj)
                            acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                a4[bi][q], b4[bj][q], acc[bi][bj], 0, 0, 0);
            }
        };
        glds(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int s = 0; s < nsub; ++s) {
            if (s + 1 < nsub) glds(s + 1, (s + 1) & 1);  // lands while slice s is multiplied
            if (mine) compute(s & 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) acc[bi][bj] = -acc[bi][bj];
    float* Cout = Ab + (int64_t)(oi * 64) * A.ld + oj * 64;
    const bool diag_here = fused && wv == 0;  // tile (ti, tj) = (d, d) goes through the diag step
    if (mine && !diag_here) {
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
            for (int bj = 0; bj < 4; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Cout[(int64_t)(16 * bi + F32_CROW(lane, r)) * A.ld + 16 * bj + r16] =
                        acc[bi][bj][r];
    }
    if (!fused) return;
    // the GEMM loop ended on a barrier: the staging area is free for the diag working set
    if (wv == 0) {
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
            for (int bj = 0; bj < 4; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sm.d.T[(16 * bi + F32_CROW(lane, r)) * DP + 16 * bj + r16] =
                        acc[bi][bj][r];
    }
    fused_diag(sm.d, Ab + (int64_t)(ti * 64) * A.ld + tj * 64, A.ld, b, ti, fd, live);
}

void launch_chol_update32_t128(MatF A, int k0, int kc, const unsigned* tiles, int ntiles,
                               Live live, int nchains, hipStream_t s, FusedDiag<float> fd,
                               int hlim, const int* h3ok, int rhs, int role, Planes16 pl) {
    // planes exactly with the role that reads them, and that role only with fp16x3 operands
    const bool planes = role == UPD32_NEWTON_PLANES;
    if (role < UPD32_NEWTON || role > UPD32_NEWTON_PLANES || planes != (pl.base != nullptr) ||
        (planes && hlim <= 0))
        throw HipError{"launch_chol_update32_t128: the role and the operand planes disagree"};
    if (ntiles <= 0) return;
    const long total = (long)ntiles * nchains;
#define UPD32_LAUNCH(H, R)                                                                     \
    APM_LAUNCH((k_chol_update32_t128<H, R>), dim3((unsigned)total), dim3(256), 0, s, A, \
                       k0, kc, tiles, ntiles, nchains, live, fd, H ? hlim : 0,               \
                       H ? h3ok : nullptr, rhs, pl)
    if (hlim > 0) {
        if (planes) UPD32_LAUNCH(true, UPD32_NEWTON_PLANES);
        else if (role == UPD32_POST) UPD32_LAUNCH(true, UPD32_POST);
        else UPD32_LAUNCH(true, UPD32_NEWTON);
    } else {
        if (role == UPD32_POST) UPD32_LAUNCH(false, UPD32_POST);
        else UPD32_LAUNCH(false, UPD32_NEWTON);
    }
#undef UPD32_LAUNCH
}

// ------------------------------------------------------------------------- 256x256 trailing update
// The Newton factorisation's far trailing updates with fp16x3 operands from the dataflow kernel's
// planes (Planes16): one 256x256 quad tile (4x4 tiles) per workgroup of 8 waves (2 x 4), each wave
// a 128x64 block (8x4 accumulators of v_mfma_f32_16x16x32_f16, three products per block as in
// k_chol_update32_t128). Per 32-deep slice a wave issues 96 MFMAs (1536 cycles) against 24 fragment
// reads; the operands of the next slice arrive by LDS-DMA (global_load_lds_dwordx4, 8 per wave)
// while the slice is multiplied: the 128-row super-tile's 48 MFMAs per slice and barrier left the
// loop waiting on its loads (29 % MFMA busy at 0.1 % LDS bank conflicts, profiles/
// r05_pmc_newton_swizzled.txt). 128 KB of LDS: one workgroup per CU, two waves per SIMD.
// Quad entries: build_update_quads (tile_lists.cpp). Invalid row/column tiles read tile I / J (no
// out-of-range reads; their results are dropped). Only chains with fp16x3 operands and rows below
// the appended right-hand side (the caller launches k_rhs_row_update32 for that row, and
// k_chol_update32_t128 for any batch with a chain outside fp16's range). Same slices in the same
// order as k_chol_update32_t128 (h3_mma), so the tiles are bitwise those of the 128-row kernel.
// npan > 1 (ROLE 0, the left-looking far updates of chol_range32): the depth loop walks the slices
// of npan consecutive outer panels, kc tiles each, whose planes lie pstep entries apart from pl on
// (panel 0's slices, then panel 1's, ...) between the one old-tile load and the one store: the
// sum the tiles receive from npan single-panel launches, in their order, without the npan - 1
// stores and reloads of fp32 in between (which are exact), so bitwise theirs.
struct __attribute__((aligned(16))) GemmSmemQ {
    _Float16 q[2][4][256][LPH];  // [buffer][A hi, A lo, B hi, B lo][row][k] (HS layout)
};
template <int ROLE>  // 0: the Newton factorisation, 1: the posterior bottom block (same code)
__global__ __launch_bounds__(512, 1) void k_chol_update32_q256(MatF A, int k0, int kc,
                                                               const unsigned* __restrict__ quads,
                                                               int nq, int nchains, Live live,
                                                               const int* __restrict__ h3ok,
                                                               Planes16 pl, int npan,
                                                               int64_t pstep) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 2, wc = wv & 3;
    const int r16 = lane & 15, kq = lane >> 4;
    __shared__ GemmSmemQ sm;
    const long w = xcd_remap((long)blockIdx.x, (long)nq * nchains);
    const int b = (int)(w / nq), t = (int)(w % nq);
    if (!live_chain(live, b) || (h3ok && !h3ok[b])) return;
    const QuadTile e(quads[t]);
    const int I = e.i(), J = e.j();
    // this wave's two 64x64 output tiles: rows I + 2wr + {0, 1}, column J + wc
    const int oi0 = I + 2 * wr, oj = J + wc;
    const bool v0 = e.writes(2 * wr, wc), v1 = e.writes(2 * wr + 1, wc);
    float* Ab = A.base + b * A.cstride;
    f4_t acc[8][4];
    // LDS-DMA staging (stage_planes): wave wv fills rows 128 (wv & 1) .. +127 of array wv >> 1
    // (0: A hi, 1: A lo, 2: B hi, 3: B lo)
    const int arr = wv >> 1, half = wv & 1;
    const int ta = arr < 2 ? e.rt(2 * half) : e.ct(2 * half);
    const int tb = arr < 2 ? e.rt(2 * half + 1) : e.ct(2 * half + 1);
    const unsigned short* P = pl.base + b * pl.cstride + ((arr & 1) ? pl.lo : 0) +
                              plane_lane_off(lane);
    const unsigned short* p0 = P + (int64_t)ta * 64 * 32;
    const unsigned short* p1 = P + (int64_t)tb * 64 * 32;
    const int64_t sstep = (int64_t)pl.rows * 32;
    _Float16* lbase = &sm.q[0][arr][128 * half][0];
    const int nsub = (64 * kc) / KS128;             // slices per panel
    const int ntot = ROLE == 0 ? npan * nsub : nsub;
    // the slices in loop order: `off` is the next one's offset in the planes (uniform), stepping
    // to the next panel's planes behind a panel's last slice
    int64_t off = 0;
    int sin = 0;
    auto dma = [&](int buf) {
        stage_planes(p0 + off, p1 + off, lbase + buf * 4 * 256 * LPH);
        off += sstep;
        if (ROLE == 0 && ++sin == nsub) {
            sin = 0;
            off += pstep - nsub * sstep;
        }
    };
    auto compute = [&](int cur) {  // this wave's 8 x 4 blocks, a dropped tile's rows left out
        h3_mma<8>(acc, sm.q[cur][0], sm.q[cur][1], sm.q[cur][2], sm.q[cur][3], 128 * wr, 64 * wc,
                  r16, kq, !v0, !v1);
    };
    const bool mine = v0 || v1;
    dma(0);
    // the old tiles, loaded while the first slice is in flight (a dropped tile reads tile (I, J)
    // instead: unconditional loads, since a per-element load-or-not makes hipcc wait for each
    // load in turn)
#pragma unroll
    for (int bi = 0; bi < 8; ++bi) {
        const bool v = bi < 4 ? v0 : v1;
        const float* Cw = Ab + (int64_t)((v ? oi0 + (bi >> 2) : I) * 64 + 16 * (bi & 3)) * A.ld +
                          (v ? oj : J) * 64;
#pragma unroll
        for (int bj = 0; bj < 4; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[bi][bj][r] = -Cw[(int64_t)F32_CROW(lane, r) * A.ld + 16 * bj + r16];
    }
#pragma unroll
    for (int bi = 0; bi < 8; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) asm volatile("" : "+v"(acc[bi][bj]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < ntot; ++s) {
        if (s + 1 < ntot) dma((s + 1) & 1);  // lands while slice s is multiplied
        if (mine) compute(s & 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int bi = 0; bi < 8; ++bi) {
        if (!(bi < 4 ? v0 : v1)) continue;
        float* Cw = Ab + (int64_t)((oi0 + (bi >> 2)) * 64 + 16 * (bi & 3)) * A.ld + oj * 64;
#pragma unroll
        for (int bj = 0; bj < 4; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Cw[(int64_t)F32_CROW(lane, r) * A.ld + 16 * bj + r16] = -acc[bi][bj][r];
    }
}

void launch_chol_update32_q256(MatF A, int k0, int kc, const unsigned* quads, int nq, Live live,
                               int nchains, hipStream_t s, const int* h3ok, Planes16 pl,
                               int role, int npan, int64_t pstep) {
    if (nq <= 0 || !pl.base) return;
    if (npan < 1 || (npan > 1 && (role != UPD32_NEWTON || pstep <= 0)))
        throw HipError{"launch_chol_update32_q256: a multi-panel depth needs the Newton role "
                       "and the planes' panel stride"};
    if (role == UPD32_POST)
        APM_LAUNCH(k_chol_update32_q256<1>, dim3((unsigned)((long)nq * nchains)), dim3(512), 0,
                   s, A, k0, kc, quads, nq, nchains, live, h3ok, pl, 1, (int64_t)0);
    else
        APM_LAUNCH(k_chol_update32_q256<0>, dim3((unsigned)((long)nq * nchains)), dim3(512), 0,
                   s, A, k0, kc, quads, nq, nchains, live, h3ok, pl, npan, pstep);
}
