// Mixed-precision Newton solve: B = I + W^1/2 K W^1/2 factored in fp32 (f32 MFMA), the solve
// B x = W^1/2 K b refined against the fp64 B until the per-chain acceptance test passes
// (usually one step at N=4096; up to APM_REFINE = 3 steps, e.g. at N=16384).
//
// The reference factors B in fp64 at every Newton iteration (latent_posterior_approximations.py:92)
// and solves with it (:94). B's eigenvalues are >= 1 and its condition number is ~1 + max(W) *
// lambda_max(K), so the fp32 factor solves to ~cond * 6e-8 and a step of iterative refinement
// with the fp64 residual r = rhs - x - W^1/2 (K (W^1/2 x)) brings x to fp64 accuracy (measured
// Newton modes agree with the all-fp64 iteration to 1e-12 relative for typical theta and 1e-8 at
// sigma = e^4; tests/test_gpu_kernels.py checks the mode against the oracle). The IS estimator
// never uses this factor otherwise (its covariance factor is rebuilt from chol(K) in fp64,
// postcov.hip), so nothing else changes. The Laplace estimator keeps the fp64 factor (its log|B|
// is part of the returned value).
//
// Kernels: fp32 copies of the diag / panel / trailing-update steps of chol.hip on the same 64x64
// tile lists (f32 MFMA v_mfma_f32_16x16x4_f32: twice the fp64 MFMA rate, half the bytes), blocked
// forward / backward TRSV with fp32 tiles and fp64 vectors, and the refinement vector ops.
#include <algorithm>
#include <vector>

#include "apm_internal.h"
#include "diag.h"

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
__device__ __forceinline__ void split_h3(const f4_t& v, h4_t& hi, h4_t& lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const _Float16 x = (_Float16)v[e];
        hi[e] = x;
        lo[e] = (_Float16)(v[e] - (float)x);
    }
}
// v_mfma_f32_16x16x4_f32: A lane l holds A[l&15][k=l>>4], B holds B[k=l>>4][l&15];
// D reg r of lane l is (row 4*(l>>4) + r, col l&15)  (cdna_hip_programming.md §3)
#define F32_CROW(l, r) (4 * ((l) >> 4) + (r))

__device__ __forceinline__ bool live32(const Live& lv, int b) {
    return lv.active[b] != 0 && lv.status[b] == 0;
}

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
        if constexpr (H3) {  // lane (r16, kq): k = 8kq .. 8kq+7 of the slice
            h8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                ah[x] = *reinterpret_cast<const h8_t*>(&sm.ah[cur][32 * wr + 16 * x + r16][HS(32 * wr + 16 * x + r16, 8 * kq)]);
                al[x] = *reinterpret_cast<const h8_t*>(&sm.al[cur][32 * wr + 16 * x + r16][HS(32 * wr + 16 * x + r16, 8 * kq)]);
                bh[x] = *reinterpret_cast<const h8_t*>(&sm.bh[cur][32 * wc + 16 * x + r16][HS(32 * wc + 16 * x + r16, 8 * kq)]);
                bl[x] = *reinterpret_cast<const h8_t*>(&sm.bl[cur][32 * wc + 16 * x + r16][HS(32 * wc + 16 * x + r16, 8 * kq)]);
            }
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) {
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[bi], bh[bj], acc[bi][bj], 0, 0, 0);
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[bi], bl[bj], acc[bi][bj], 0, 0, 0);
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[bi], bh[bj], acc[bi][bj], 0, 0, 0);
                }
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

// ------------------------------------------------------------------------------- panel, update
// Same XCD-aware work mapping as k_chol_update (chol.hip).
__device__ __forceinline__ long xcd_remap32(long L, long total) {
    const long xcd = L & 7, q = total >> 3, r = total & 7;
    const long base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (L >> 3);
}

// fd.enabled: workgroups 0 .. nchains-1 update the diagonal tile tiles[0] = (d, d) of chain b and
// factor it in place (diag_compute + diag_store, fp64 arithmetic, fp32 storage) - see k_chol_update (chol.hip).
__global__ __launch_bounds__(256) void k_chol_update32(MatF A, int k0, int kc,
                                                       const unsigned* __restrict__ tiles,
                                                       int ntiles, int nchains, Live live,
                                                       FusedDiag<float> fd, int hlim,
                                                       const int* __restrict__ h3ok) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1;
    __shared__ union {
        GemmSmem32 g;
        DiagSmem32 d;  // fp32 arithmetic: the Newton factor is refined in fp64
    } sm;
    int b, t;
    const bool fused = fd.enabled && (int)blockIdx.x < nchains;
    if (fused) {
        b = blockIdx.x;
        t = 0;
    } else {
        const int nt = fd.enabled ? ntiles - 1 : ntiles;
        const long L = (long)blockIdx.x - (fd.enabled ? nchains : 0);
        const long w = xcd_remap32(L, (long)nt * nchains);
        b = (int)(w / nt);
        t = (int)(w % nt) + (fd.enabled ? 1 : 0);
    }
    if (!live32(live, b)) return;
    const unsigned ij = tiles[t];
    const int i = (int)(ij >> 16), j = (int)(ij & 0xffff);
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
    if (!fused) {
        tile32_store(acc, Aij, A.ld, wr, wc, lane);
        return;
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sm.d.T[(32 * wr + 16 * bi + F32_CROW(lane, r)) * DP + 32 * wc + 16 * bj +
                       (lane & 15)] = acc[bi][bj][r];
    __syncthreads();
    if (wv == 0) {
        const bool ok = diag_compute<true, float>(sm.d, lane);
        if (lane == 0) sm.d.ok = ok;
    }
    __syncthreads();
    if (!sm.d.ok) {
        if (threadIdx.x == 0) live.status[b] = fd.fail_code;
        return;
    }
    diag_store<float>(sm.d, Aij, A.ld, fd.Dinv + b * fd.dstride + (int64_t)i * 4096,
                      fd.ldet + b * fd.lstride + i, threadIdx.x, 256);
}

void launch_chol_update32(MatF A, int k0, int kc, const unsigned* tiles, int ntiles, Live live,
                          int nchains, hipStream_t s, FusedDiag<float> fd, int hlim,
                          const int* h3ok) {
    if (ntiles <= 0) return;
    const long total = (long)ntiles * nchains;
    APM_LAUNCH(k_chol_update32, dim3((unsigned)total), dim3(256), 0, s, A, k0, kc, tiles,
                       ntiles, nchains, live, fd, hlim, h3ok);
}

// ------------------------------------------------------------------ dataflow in-panel factorisation
// One launch factors the tile columns [K, K + ncols) of an outer panel (the diagonal tile (K, K)
// already factored): workgroup (row tile i, chain b) walks its row through the panel's columns,
// for column k the left-looking update A_ik -= L_i[K:k] L_k[K:k]^T (the in-panel k_chol_update32
// step, same operands, same code) and then either the diagonal factorisation (i == k; diag.h) or
// the panel TRSM A_ik <- A_ik inv(L_kk)^T (tile_gemm_nt32 over the whole tile, the accumulation
// order of the per-column panel launch it replaced).
// Results are bitwise those of the launch sequence it replaces (2 launches per column), whose
// dependent-launch boundaries and the diagonal tile's latency at the tail of every update launch
// were ~110 us per column.
//
// Row k's progress is a per-(chain, row) word: base + s after s of its columns are final
// (base = factorisation and panel, monotonic, so no reset between launches; s = 15: the chain
// failed, waiters leave). A row waits for row k (k < i, lower workgroup index) before its update
// of column k (s >= k-K: L_k[K:k] final) and before the TRSM (s >= k-K+1: L_kk and inv(L_kk)
// final). Only the diagonal-block rows publish; their tiles are stored write-through (sc1) and
// drained before one lane's agent-scope flag store; a waiter polls relaxed (one lane, s_sleep),
// then one agent-scope acquire (MI355X_MICROARCH.md, inter-workgroup visibility). Workgroups
// depend only on lower indices (row-major over (row, chain)), so in-order dispatch guarantees
// progress; a bounded spin marks the chain failed instead of hanging (the Newton loop then reruns
// it in fp64).
#define DF_FAILED 15
#ifndef DF_UNROLLED
#define DF_UNROLLED true
#endif
// DF_TRACE (diagnostic builds only, tools/df_trace.py): wall-clock stamps of chain 0's first
// outer panel, [row - K][column - K][event], read back by apm_debug_df_trace
#ifdef DF_TRACE
__device__ unsigned long long df_trace[64 * 16 * 8];
#define DF_STAMP(ev)                                                                         \
    do {                                                                                     \
        if (b == 0 && K == 0 && threadIdx.x == 0 && i - K < 64)                              \
            __hip_atomic_store(&df_trace[((i - K) * 16 + (k - K)) * 8 + (ev)],                \
                               (unsigned long long)__builtin_amdgcn_s_memrealtime(),         \
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                  \
    } while (0)
extern "C" int apm_debug_df_trace(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(df_trace), sizeof(df_trace)) == hipSuccess ? 0 : 1;
}
#else
#define DF_STAMP(ev) \
    do {             \
    } while (0)
#endif
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

#ifndef DF_WPE
#define DF_WPE 2  // min workgroups per CU of the dataflow panel kernel
#endif
#ifndef DF_BULK_WPE
#define DF_BULK_WPE 3  // ... and of its bulk-row twin (no diagonal factorisation, no waits)
#endif
// BULK = false: rows [K, R) as described above. BULK = true: rows [row0, R) below an outer panel
// whose diagonal block is already factored (every diagonal tile and its inverse final): the same
// row walk without the waits and without the diagonal factorisation code (whose registers hold
// the combined kernel at 2 workgroups per CU). Used for the fp32 bottom block of the posterior
// factor (postcov.hip): with zrow > 0, row tile i is zero in the tile columns < zrow - 1 - i (the
// anti-triangular L_K J), so its walk starts at column max(K, zrow - 1 - i) and reads no zero tile.
template <bool BULK>
__global__ __launch_bounds__(256, BULK ? DF_BULK_WPE : DF_WPE) void k_chol_panel_df32(MatF A, int K, int ncols, int R, int nchains,
                                                         FusedDiag<float> fd, Live live, int hlim,
                                                         const int* __restrict__ h3ok,
                                                         unsigned long long* prog,
                                                         int64_t pstride,
                                                         unsigned long long base, SpinCtl sc,
                                                         Planes16 pl, int rhs_as = -1,
                                                         const int* __restrict__ inv_skip = nullptr,
                                                         int row0 = 0,
                                                         int zrow = 0) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1;
    __shared__ union {
        GemmSmem32 g;
        DiagSmem32 d;
    } sm;
    __shared__ unsigned long long seen;
    const int Kend = K + ncols;
    int b, i;
    if constexpr (BULK) {
        // no dependencies between these workgroups: XCD-aware and chain-major (dispatch slot s
        // runs on XCD s % 8, which takes a contiguous range of chains), so that the workgroups
        // sharing a chain's diagonal-block tiles share an L2 and few chains' panels are live in
        // the Infinity Cache at a time
        const long rows = R - row0, total = rows * nchains, L = blockIdx.x;
        const long xcd = L & 7, q = total >> 3, rm = total & 7;
        const long item = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + (L >> 3);
        b = (int)(item / rows);
        i = row0 + (int)(item % rows);
    } else {
        // logical index = arrival ticket (SpinCtl): row i waits only on rows k < i of its chain,
        // i.e. on workgroups that have already arrived - resident or finished, whatever the
        // dispatch order
        if (threadIdx.x == 0)
            seen = __hip_atomic_fetch_add(sc.ticket, 1ull, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT) - sc.base;
        __syncthreads();
        const unsigned long long lin = seen;
        __syncthreads();  // (`seen` is reused by the waits)
        if (lin >= (unsigned long long)(R - K) * nchains) {
            // tickets out of step with the host's count (a launch that never ran): rows would go
            // unprocessed, so every chain of the launch fails (fp64 rerun) instead
            if (threadIdx.x == 0) {
                for (int c = 0; c < nchains; ++c) live.status[c] = fd.fail_code;
                atomicAdd(sc.timeouts, 1ull);
            }
            return;
        }
        b = (int)(lin % nchains);
        i = K + (int)(lin / nchains);
        // explicit-inverse panels (k_panel_inv_gemm32): this launch walks the diagonal block and
        // the right-hand-side row only, the last logical row being that row
        if (rhs_as >= 0 && i == Kend) i = rhs_as;
        // ... or the whole panel, the rows below the diagonal block of the chains that take the
        // explicit-inverse panel excepted (inv_skip: the host's invok flags; a batch with a chain
        // outside their range: that chain walks, the others do not)
        if (inv_skip && i >= Kend && i < hlim && inv_skip[b]) return;
    }
    const bool pub = !BULK && i < Kend;  // rows of the diagonal block: later rows wait on them
    unsigned long long* pr = prog + b * pstride;
    auto publish = [&](unsigned long long v) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its sc1 stores drained
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(pr + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // one lane polls row k's word relaxed, then ONE agent acquire for the workgroup; false: the
    // chain failed (or the spin bound was hit)
    auto wait_row = [&](int k, unsigned long long need) -> bool {
        if (threadIdx.x == 0) {
            unsigned long long v =
                __hip_atomic_load(pr + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int spins = 0; v < need; ++spins) {
                if (spins > sc.limit) {  // counted apart from breakdowns (APM_PROF_DF_TIMEOUTS)
                    atomicAdd(sc.timeouts, 1ull);
                    v = base + DF_FAILED;
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
                v = __hip_atomic_load(pr + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            seen = v;
        }
        __syncthreads();
        return (seen & 15) != DF_FAILED;
    };
    auto leave_failed = [&]() {
        if (threadIdx.x == 0) live.status[b] = fd.fail_code;
        if (pub) publish(base + DF_FAILED);
    };
    if (!live32(live, b)) {
        if (pub) publish(base + DF_FAILED);
        return;
    }
    if (i == K) return;  // (K, K) was factored by the launch before
    float* Ab = A.base + b * A.cstride;
    const bool h3 = i < hlim && (!h3ok || h3ok[b]);
    const int last = min(Kend - 1, i);
    // the diagonal tile's update by all but the last of its row's panel columns, accumulated at
    // the step before (off the diagonal chain); the step itself adds the last column's slices and
    // the old tile - the same slices in the same order as one call over the whole depth
    f4_t dacc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) dacc[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};
    const float* Ai = Ab + (int64_t)(i * 64) * A.ld;
    // first column of the walk (BULK with a zero pattern: the row's first nonzero tile column)
    const int kstart = (BULK && zrow > 0) ? max(K, zrow - 1 - i) : K;
    if (BULK && pl.base && kstart > K && (i + 1) * 64 <= pl.rows) {
        // the operand planes of the row's known-zero tiles in this panel (the trailing update
        // reads every panel column of the row)
        for (int k = K; k < kstart; ++k) {
            unsigned short* hp = pl.base + b * pl.cstride +
                                 ((int64_t)(2 * (k - K) + wc) * pl.rows + i * 64 + 32 * wr) * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                hp[64 * q + lane] = 0;
                hp[pl.lo + 64 * q + lane] = 0;
            }
        }
    }
    for (int k = kstart; k <= last; ++k) {
        const int c = k - kstart;
        DF_STAMP(0);
        float* Aik = Ab + (int64_t)(i * 64) * A.ld + k * 64;
        f4_t acc[2][2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};
        if (c > 0) {  // left-looking update by the panel's earlier columns (k_chol_update32)
            if (BULK) {
                // (every diagonal-block tile is final: written by the launch before)
            } else if (i != k) {
                if (!wait_row(k, base + c)) {
                    leave_failed();
                    return;
                }
                DF_STAMP(1);
            } else {  // own earlier tiles only: refresh this CU's L1 (they were re-stored)
                if (threadIdx.x == 0) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __syncthreads();
            }
            if (!BULK && i == k) {  // the diagonal tile: its last column's slices and the old tile
#pragma unroll
                for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = dacc[bi][bj];
                if (h3)
                    tile_gemm_nt32<true, true>(acc, Ai + (k - 1) * 64, A.ld, Ai + (k - 1) * 64,
                                               A.ld, 64, sm.g, Aik, A.ld);
                else
                    tile_gemm_nt32<true>(acc, Ai + (k - 1) * 64, A.ld, Ai + (k - 1) * 64, A.ld,
                                         64, sm.g, Aik, A.ld);
            } else if (h3) {
                tile_gemm_nt32<true, true>(acc, Ai + kstart * 64, A.ld,
                                           Ab + (int64_t)(k * 64) * A.ld + kstart * 64, A.ld,
                                           64 * c, sm.g, Aik, A.ld);
            } else {
                tile_gemm_nt32<true>(acc, Ai + kstart * 64, A.ld,
                                     Ab + (int64_t)(k * 64) * A.ld + kstart * 64, A.ld, 64 * c,
                                     sm.g, Aik, A.ld);
            }
            if (!BULK && k + 1 == i) {  // next step is the diagonal tile: its columns K .. k-1 now
                if (h3)
                    tile_gemm_nt32<true, true>(dacc, Ai + K * 64, A.ld, Ai + K * 64, A.ld, 64 * c,
                                               sm.g, nullptr, 0);
                else
                    tile_gemm_nt32<true>(dacc, Ai + K * 64, A.ld, Ai + K * 64, A.ld, 64 * c, sm.g,
                                         nullptr, 0);
            }
        } else {
            tile32_load(acc, Aik, A.ld, wr, wc, lane);
        }
        DF_STAMP(2);
        if constexpr (!BULK) if (i == k) {  // diagonal tile: factor and publish (row i is then done)
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sm.d.T[(32 * wr + 16 * bi + F32_CROW(lane, r)) * DP + 32 * wc + 16 * bj +
                               (lane & 15)] = acc[bi][bj][r];
            __syncthreads();
            DF_STAMP(5);
            if (wv == 0) {
                const bool ok = diag_compute<DF_UNROLLED, float>(sm.d, lane);
                if (lane == 0) sm.d.ok = ok;
            }
            __syncthreads();
            DF_STAMP(6);
            if (!sm.d.ok) {
                leave_failed();
                return;
            }
            diag_store<float, float, true>(sm.d, Aik, A.ld,
                                           fd.Dinv + b * fd.dstride + (int64_t)i * 4096,
                                           fd.ldet + b * fd.lstride + i, threadIdx.x, 256);
            publish(base + c + 1);
            DF_STAMP(7);
            return;
        }
        // panel TRSM: A_ik inv(L_kk)^T, the updated tile and inv(L_kk) staged as tile_gemm_nt32's
        // two 32-deep slices (A operand: acc; B operand: inv(L_kk) row-major)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sm.g.a[wc][32 * wr + 16 * bi + F32_CROW(lane, r)][16 * bj + (lane & 15)] =
                        acc[bi][bj][r];
        // inv(L_KK) comes from the launch before; later columns' from row k's workgroup
        if (!BULK && c > 0 && !wait_row(k, base + c + 1)) {
            leave_failed();
            return;
        }
        DF_STAMP(3);
        {
            const float* D = fd.Dinv + b * fd.dstride + (int64_t)k * 4096;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int p = threadIdx.x + 256 * h;  // 16-byte piece: row p / 16, column 4 (p % 16)
                const int row = p >> 4, col = 4 * (p & 15);
                const f4_t v = *reinterpret_cast<const f4_t*>(D + row * 64 + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) sm.g.b[col >> 5][row][(col & 31) + e] = v[e];
            }
        }
        __syncthreads();
        f4_t x[2][2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) x[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};
        const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
        for (int cur = 0; cur < 2; ++cur)
#pragma unroll
            for (int t = 0; t < KS32 / 4; ++t) {
                float a[2], bb[2];
#pragma unroll
                for (int bi = 0; bi < 2; ++bi) a[bi] = sm.g.a[cur][32 * wr + 16 * bi + r16][4 * t + kq];
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) bb[bj] = sm.g.b[cur][32 * wc + 16 * bj + r16][4 * t + kq];
#pragma unroll
                for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj)
                        x[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[bi], bb[bj], x[bi][bj],
                                                                        0, 0, 0);
            }
        if (pub) {
            tile32_store_sc1(x, Aik, A.ld, wr, wc, lane);
            publish(base + c + 1);
            DF_STAMP(4);
        } else {
            tile32_store(x, Aik, A.ld, wr, wc, lane);
            if (pl.base && (i + 1) * 64 <= pl.rows) {
                // the trailing update's fp16x3 operand planes: this wave's 32x32 block is rows
                // 32wr .. +31 of slice 2(k - K) + wc (Planes16)
                unsigned short* hp = pl.base + b * pl.cstride +
                                     ((int64_t)(2 * (k - K) + wc) * pl.rows + i * 64 + 32 * wr) * 32;
#pragma unroll
                for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float v = x[bi][bj][r];
                            const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
                            const int o = (16 * bi + F32_CROW(lane, r)) * 32 + 16 * bj + (lane & 15);
                            hp[o] = __builtin_bit_cast(unsigned short, h);
                            hp[pl.lo + o] = __builtin_bit_cast(unsigned short, l);
                        }
            }
            __syncthreads();  // the staging area is reused by the next column's update
        }
    }
}

long launch_chol_panel_df32(MatF A, int K, int ncols, int R, FusedDiag<float> fd, Live live,
                            int nchains, int hlim, const int* h3ok, unsigned long long* prog,
                            int64_t pstride, unsigned long long base, SpinCtl sc, hipStream_t s,
                            Planes16 pl, int rhs_as, const int* inv_skip) {
    // the progress word holds the step in 4 bits, 15 = failed: a wider panel is refused (the
    // caller raises) instead of being left unfactored
    if (ncols > 14) return -1;
    if (ncols < 1 || R - K <= 1) return 0;  // (one column: its panel TRSM)
    const long grid = (long)(R - K) * nchains;
    APM_LAUNCH(k_chol_panel_df32<false>, dim3((unsigned)grid), dim3(256), 0, s, A, K,
                       ncols, R, nchains, fd, live, hlim, h3ok, prog, pstride, base, sc, pl,
                       rhs_as, inv_skip);
    return grid;
}

void launch_chol_panel_bulk32(MatF A, int K, int ncols, int row0, int R, int zrow,
                              FusedDiag<float> fd, Live live, int nchains, int hlim,
                              const int* h3ok, hipStream_t s, Planes16 pl) {
    if (ncols < 1 || R <= row0) return;
    APM_LAUNCH(k_chol_panel_df32<true>, dim3((unsigned)((long)(R - row0) * nchains)),
                       dim3(256), 0, s, A, K, ncols, R, nchains, fd, live, hlim, h3ok, nullptr,
                       (int64_t)0, 0ull, SpinCtl{nullptr, 0ull, nullptr, 0}, pl, -1,
                       (const int*)nullptr, row0, zrow);
}

// ------------------------------------------------------------------------- 128x128 trailing update
// The rank-64*kc outer updates with one 128x128 super-tile (2x2 tiles) per workgroup: each wave
// owns a 64x64 tile (4x4 v_mfma_f32_16x16x4_f32 accumulators), so a slice of operands staged in
// LDS feeds twice the MFMAs of the 64x64 kernel per byte loaded (8 instead of 16 B/clk/CU of
// L2->LDS traffic at the MFMA rate: the 64x64 kernel is operand-load bound).
// Super-tile entries (build_update_supertiles): (i << 18) | (j << 4) | rv0 | rv1<<1 | cv0<<2 |
// cv1<<3, rows i, i+1 and columns j, j+1 (tile units) with per-half validity; a tile (i+a, j+b)
// is written iff rv_a && cv_b && j+b <= i+a. Invalid halves load a valid half's operands (no
// out-of-range reads) and their results are dropped.
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;
#define KS128 32
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
#ifndef H3_ABL
#define H3_ABL 0
#endif

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
// ROLE 0: the Newton factorisation, 1: the posterior factor's bottom block (postcov.hip; the same
// code, a separate instantiation so that the two launch populations get separate rocprofv3
// counter figures), 2: the Newton factorisation with the fp16x3 operands read from the dataflow
// kernel's planes (Planes16) instead of split while staged, 3: the right-hand-side row tile alone
// beside the quad-tile kernel (a name only)
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
        DiagSmem32 d;  // fp32 arithmetic: the Newton factor is refined in fp64
    } sm;
    int b, t;
    const bool fused = fd.enabled && (int)blockIdx.x < nchains;
    if (fused) {
        b = blockIdx.x;
        t = 0;
    } else {
        const int nt = fd.enabled ? ntiles - 1 : ntiles;
        const long L = (long)blockIdx.x - (fd.enabled ? nchains : 0);
        const long w = xcd_remap32(L, (long)nt * nchains);
        b = (int)(w / nt);
        t = (int)(w % nt) + (fd.enabled ? 1 : 0);
    }
    if (!live32(live, b)) return;
    const unsigned e = tiles[t];
    const int ti = (int)(e >> 18), tj = (int)((e >> 4) & 0x3fff);
    const bool rv0 = e & 1u, rv1 = e & 2u, cv0 = e & 4u, cv1 = e & 8u;
    // operand row tiles of the two halves (an invalid half reuses the valid one)
    const int ra0 = rv0 ? ti : ti + 1, ra1 = rv1 ? ti + 1 : ti;
    const int cb0 = cv0 ? tj : tj + 1, cb1 = cv1 ? tj + 1 : tj;
    float* Ab = A.base + b * A.cstride;
    if (ti == rhs) {  // the right-hand-side row alone (its super-tile row holds no other tile)
        rhs_row_update32(Ab, A.ld, ti, tj, cv0, cv1, k0, kc, tid);
        return;
    }
    // this wave's output tile
    const int oi = ti + wr, oj = tj + wc;
    const bool mine = (wr ? rv1 : rv0) && (wc ? cv1 : cv0) && oj <= oi;

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
    const bool use_h3 = H3 && ti + (rv1 ? 1 : 0) < hlim && (!h3ok || h3ok[b]);
    if (!(ROLE == 2 && use_h3)) load_old();
    if (ROLE == 2 && use_h3) {
        // operands already split by the dataflow panel kernel (Planes16): LDS-DMA staging, no
        // registers, no VALU. Wave wv fills one array (0: A hi, 1: A lo, 2: B hi, 3: B lo) of a
        // slice, 8 global_load_lds_dwordx4 of 16 rows x 64 B; lane l takes row 16q + l/4 and
        // stores LDS slot l%4, i.e. logical piece (l%4) ^ (bit 3 of the row) - the HS layout that
        // compute() reads
        const int rowl = lane >> 2, piece = (lane & 3) ^ ((rowl >> 2) & 2);
        const int t0 = wv < 2 ? ra0 : cb0, t1 = wv < 2 ? ra1 : cb1;
        const unsigned short* P = pl.base + b * pl.cstride + ((wv & 1) ? pl.lo : 0) +
                                  (int64_t)rowl * 32 + piece * 8;
        const unsigned short* p0 = P + (int64_t)t0 * 64 * 32;
        const unsigned short* p1 = P + (int64_t)t1 * 64 * 32;
        const int64_t sstep = (int64_t)pl.rows * 32;
        _Float16* lbase = &sm.h.ah[0][0][0] + wv * (2 * 128 * LPH);
        auto dma = [&](int sidx, int buf) {
            const int64_t o = sidx * sstep;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                __builtin_amdgcn_global_load_lds(
                    (glb_void_t*)((q < 4 ? p0 : p1) + o + (16 * (q & 3)) * 32),
                    (lds_void_t*)(lbase + (buf * 128 + 16 * q) * LPH), 16, 0, 0);
        };
        auto compute = [&](int cur) {
            h8_t bh[4], bl[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                bh[x] = *reinterpret_cast<const h8_t*>(&sm.h.bh[cur][64 * wc + 16 * x + r16][HS(64 * wc + 16 * x + r16, 8 * kq)]);
                bl[x] = *reinterpret_cast<const h8_t*>(&sm.h.bl[cur][64 * wc + 16 * x + r16][HS(64 * wc + 16 * x + r16, 8 * kq)]);
            }
#pragma unroll
            for (int bi = 0; bi < 4; ++bi) {
                const h8_t ah =
                    *reinterpret_cast<const h8_t*>(&sm.h.ah[cur][64 * wr + 16 * bi + r16][HS(64 * wr + 16 * bi + r16, 8 * kq)]);
                const h8_t al =
                    *reinterpret_cast<const h8_t*>(&sm.h.al[cur][64 * wr + 16 * bi + r16][HS(64 * wr + 16 * bi + r16, 8 * kq)]);
#pragma unroll
                for (int bj = 0; bj < 4; ++bj) {
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[bj], acc[bi][bj], 0, 0, 0);
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[bj], acc[bi][bj], 0, 0, 0);
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[bj], acc[bi][bj], 0, 0, 0);
                }
            }
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
            if (mine) compute(s & 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    } else if (ROLE != 2 && use_h3) {
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
#if H3_ABL == 1  // ablation (tools/upd16_bench.cpp): every slice reads slice 0 (cache-resident)
            sidx = 0;
#endif
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                ra[h] = *reinterpret_cast<const f4_t*>(arow[h] + sidx * KS128);
                rb[h] = *reinterpret_cast<const f4_t*>(brow[h] + sidx * KS128);
            }
        };
        auto split = [](const f4_t& v, h4_t& hi, h4_t& lo) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const _Float16 x = (_Float16)v[e];
                hi[e] = x;
                lo[e] = (_Float16)(v[e] - (float)x);
            }
        };
        auto sstore = [&](int buf, const f4_t (&ra)[4], const f4_t (&rb)[4]) {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                h4_t hi, lo;
                split(ra[h], hi, lo);
                *reinterpret_cast<h4_t*>(&sm.h.ah[buf][prow[h]][HS(prow[h], pcol[h])]) = hi;
                *reinterpret_cast<h4_t*>(&sm.h.al[buf][prow[h]][HS(prow[h], pcol[h])]) = lo;
                split(rb[h], hi, lo);
                *reinterpret_cast<h4_t*>(&sm.h.bh[buf][prow[h]][HS(prow[h], pcol[h])]) = hi;
                *reinterpret_cast<h4_t*>(&sm.h.bl[buf][prow[h]][HS(prow[h], pcol[h])]) = lo;
            }
        };
        // lane (r16, kq): k = 8kq .. 8kq+7 of the slice = one 16-byte read per half and tile;
        // the B fragments stay in registers, the A fragments are read per tile row
        auto compute = [&](int cur) {
#if H3_ABL == 2  // ablation: no MFMA
            return;
#endif
            h8_t bh[4], bl[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                bh[x] = *reinterpret_cast<const h8_t*>(&sm.h.bh[cur][64 * wc + 16 * x + r16][HS(64 * wc + 16 * x + r16, 8 * kq)]);
                bl[x] = *reinterpret_cast<const h8_t*>(&sm.h.bl[cur][64 * wc + 16 * x + r16][HS(64 * wc + 16 * x + r16, 8 * kq)]);
            }
#pragma unroll
            for (int bi = 0; bi < 4; ++bi) {
                const h8_t ah =
                    *reinterpret_cast<const h8_t*>(&sm.h.ah[cur][64 * wr + 16 * bi + r16][HS(64 * wr + 16 * bi + r16, 8 * kq)]);
                const h8_t al =
                    *reinterpret_cast<const h8_t*>(&sm.h.al[cur][64 * wr + 16 * bi + r16][HS(64 * wr + 16 * bi + r16, 8 * kq)]);
#pragma unroll
                for (int bj = 0; bj < 4; ++bj) {
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[bj], acc[bi][bj], 0, 0, 0);
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[bj], acc[bi][bj], 0, 0, 0);
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[bj], acc[bi][bj], 0, 0, 0);
                }
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
            if (mine) compute(s & 1);  // a wave whose tile is dropped only stages
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
    __syncthreads();
    if (wv == 0) {
        const bool ok = diag_compute<true, float>(sm.d, lane);
        if (lane == 0) sm.d.ok = ok;
    }
    __syncthreads();
    if (!sm.d.ok) {
        if (tid == 0) live.status[b] = fd.fail_code;
        return;
    }
    diag_store<float>(sm.d, Ab + (int64_t)(ti * 64) * A.ld + tj * 64, A.ld,
                      fd.Dinv + b * fd.dstride + (int64_t)ti * 4096, fd.ldet + b * fd.lstride + ti,
                      tid, 256);
}

void launch_chol_update32_t128(MatF A, int k0, int kc, const unsigned* tiles, int ntiles,
                               Live live, int nchains, hipStream_t s, FusedDiag<float> fd,
                               int hlim, const int* h3ok, int rhs, int role, Planes16 pl) {
    if (ntiles <= 0) return;
    const long total = (long)ntiles * nchains;
#define UPD32_LAUNCH(H, R)                                                                     \
    APM_LAUNCH((k_chol_update32_t128<H, R>), dim3((unsigned)total), dim3(256), 0, s, A, \
                       k0, kc, tiles, ntiles, nchains, live, fd, H ? hlim : 0,               \
                       H ? h3ok : nullptr, rhs, pl)
    if (hlim > 0) {
        if (role == 3) UPD32_LAUNCH(true, 3);  // the right-hand-side row alone
        else if (pl.base) UPD32_LAUNCH(true, 2);
        else if (role) UPD32_LAUNCH(true, 1);
        else UPD32_LAUNCH(true, 0);
    } else {
        if (role) UPD32_LAUNCH(false, 1); else UPD32_LAUNCH(false, 0);
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
// Quad entries (build_update_quads): (I << 20) | (J << 8) | rmask << 4 | cmask, row tiles I .. I+3
// and column tiles J .. J+3 with per-tile validity; tile (I+a, J+c) is written iff rmask bit a,
// cmask bit c and J+c <= I+a. Invalid row/column tiles read tile I / J (no out-of-range reads;
// their results are dropped). Only chains with fp16x3 operands and rows below the appended
// right-hand side (the caller launches k_chol_update32_t128 for that row and for any batch with
// a chain outside fp16's range). Same slices in the same order as k_chol_update32_t128, so the
// tiles are bitwise those of the 128-row kernel.
struct __attribute__((aligned(16))) GemmSmemQ {
    _Float16 q[2][4][256][LPH];  // [buffer][A hi, A lo, B hi, B lo][row][k] (HS layout)
};
template <int ROLE>  // 0: the Newton factorisation, 1: the posterior bottom block (same code)
__global__ __launch_bounds__(512, 1) void k_chol_update32_q256(MatF A, int k0, int kc,
                                                               const unsigned* __restrict__ quads,
                                                               int nq, int nchains, Live live,
                                                               const int* __restrict__ h3ok,
                                                               Planes16 pl) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 2, wc = wv & 3;
    const int r16 = lane & 15, kq = lane >> 4;
    __shared__ GemmSmemQ sm;
    const long w = xcd_remap32((long)blockIdx.x, (long)nq * nchains);
    const int b = (int)(w / nq), t = (int)(w % nq);
    if (!live32(live, b) || (h3ok && !h3ok[b])) return;
    const unsigned e = quads[t];
    const int I = (int)(e >> 20), J = (int)((e >> 8) & 0xfff), rm = (e >> 4) & 15, cm = e & 15;
    auto rt = [&](int a) { return (rm >> a) & 1 ? I + a : I; };
    auto ct = [&](int c) { return (cm >> c) & 1 ? J + c : J; };
    // this wave's two 64x64 output tiles: rows I + 2wr + {0, 1}, column J + wc
    const int oi0 = I + 2 * wr, oj = J + wc;
    const bool v0 = ((rm >> (2 * wr)) & 1) && ((cm >> wc) & 1) && oj <= oi0;
    const bool v1 = ((rm >> (2 * wr + 1)) & 1) && ((cm >> wc) & 1) && oj <= oi0 + 1;
    float* Ab = A.base + b * A.cstride;
    f4_t acc[8][4];
    // LDS-DMA staging: wave wv fills rows 128 (wv & 1) .. +127 of array wv >> 1 (0: A hi, 1: A lo,
    // 2: B hi, 3: B lo); lane l takes row 16q + l/4 and LDS slot l%4 = logical piece
    // (l%4) ^ (bit 3 of the row) (the HS layout compute() reads)
    const int arr = wv >> 1, half = wv & 1;
    const int rowl = lane >> 2, piece = (lane & 3) ^ ((rowl >> 2) & 2);
    const int ta = arr < 2 ? rt(2 * half) : ct(2 * half);
    const int tb = arr < 2 ? rt(2 * half + 1) : ct(2 * half + 1);
    const unsigned short* P = pl.base + b * pl.cstride + ((arr & 1) ? pl.lo : 0) +
                              (int64_t)rowl * 32 + piece * 8;
    const unsigned short* p0 = P + (int64_t)ta * 64 * 32;
    const unsigned short* p1 = P + (int64_t)tb * 64 * 32;
    const int64_t sstep = (int64_t)pl.rows * 32;
    _Float16* lbase = &sm.q[0][arr][128 * half][0];
    auto dma = [&](int sidx, int buf) {
        const int64_t o = sidx * sstep;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            __builtin_amdgcn_global_load_lds(
                (glb_void_t*)((q < 4 ? p0 : p1) + o + (16 * (q & 3)) * 32),
                (lds_void_t*)(lbase + (buf * 4 * 256 + 16 * q) * LPH), 16, 0, 0);
    };
    auto compute = [&](int cur) {
        h8_t bh[4], bl[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int row = 64 * wc + 16 * x + r16;
            bh[x] = *reinterpret_cast<const h8_t*>(&sm.q[cur][2][row][HS(row, 8 * kq)]);
            bl[x] = *reinterpret_cast<const h8_t*>(&sm.q[cur][3][row][HS(row, 8 * kq)]);
        }
#pragma unroll
        for (int bi = 0; bi < 8; ++bi) {
            if (!(bi < 4 ? v0 : v1)) continue;
            const int row = 128 * wr + 16 * bi + r16;
            const h8_t ah = *reinterpret_cast<const h8_t*>(&sm.q[cur][0][row][HS(row, 8 * kq)]);
            const h8_t al = *reinterpret_cast<const h8_t*>(&sm.q[cur][1][row][HS(row, 8 * kq)]);
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[bj], acc[bi][bj], 0, 0, 0);
                acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[bj], acc[bi][bj], 0, 0, 0);
                acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[bj], acc[bi][bj], 0, 0, 0);
            }
        }
    };
    const bool mine = v0 || v1;
    const int nsub = (64 * kc) / KS128;
    dma(0, 0);
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
    for (int s = 0; s < nsub; ++s) {
        if (s + 1 < nsub) dma(s + 1, (s + 1) & 1);  // lands while slice s is multiplied
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
                               int role) {
    if (nq <= 0 || !pl.base) return;
    if (role == 1)
        APM_LAUNCH(k_chol_update32_q256<1>, dim3((unsigned)((long)nq * nchains)), dim3(512), 0,
                   s, A, k0, kc, quads, nq, nchains, live, h3ok, pl);
    else
        APM_LAUNCH(k_chol_update32_q256<0>, dim3((unsigned)((long)nq * nchains)), dim3(512), 0,
                   s, A, k0, kc, quads, nq, nchains, live, h3ok, pl);
}

// ------------------------------------------------------------------------- explicit-inverse panel
// The rows below an outer panel's 512x512 diagonal block L_D solve X_i L_D^T = A_i. The dataflow
// walk does that per row tile as 8 dependent column steps (left-looking update, TRSM by the
// 64x64 inverse), each re-reading the row's earlier panel tiles (~95 us per walk, ~120 TFLOP/s
// fp32-equivalent). Here the diagonal block's inverse Z = inv(L_D) (lower triangular) is formed
// once per chain and panel, and every row tile becomes one GEMM X_i = A_i Z^T with independent
// output columns: X_i[:, c] = sum_{k <= c} A_i[:, k] Z_ck^T. Rounding differs from the walk's
// (the fp64 refinement, not bitwise equality, pins it: DESIGN.md §3.1).
//
// Z = inv(L_D) by recursive doubling in 64-tile units (fp32 MFMA): with L_D split into
// [[L11, 0], [L21, L22]] of m x m tiles, Z21 = -Z22 (L21 Z11). Level m = 1, 2, 4 takes the
// 8 / (2m) diagonal pairs of the level at once, so Z needs 3 dependent launches of 64x64 tile
// products (depth <= 4 tiles) instead of a 7-step substitution per column (150-270 us per panel
// at 64 chains, round 5). Scratch per chain (zt, 3 x 512 x 512 fp32): Z row-major, Z^T, and T^T,
// the operands of tile_gemm_nt32's A B^T form; Z also goes out as fp16x3 planes (512 rows).
__device__ __forceinline__ void zput16(unsigned short* Z, const Planes16& zp, int zr, int zc,
                                       float v) {
    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
    const int64_t o = ((int64_t)(zc >> 5) * zp.rows + zr) * 32 + (zc & 31);
    Z[o] = __builtin_bit_cast(unsigned short, h);
    Z[o + zp.lo] = __builtin_bit_cast(unsigned short, l);
}
#define ZS 512  // scratch leading dimension
// one level m of the doubling: workgroup (chain, pair p, column tb) of the pair whose L21 sits at
// tile rows r0 = 2mp + m, columns c0 = 2mp computes column tb of T = L21 Z11 (stored transposed),
// then column tb of Z21 = -Z22 T (stored as Z, Z^T and planes); level 1 first writes the pair's
// two diagonal tiles Z_ii = inv(L_ii). Three launches per panel (m = 1, 2, 4: 4 workgroups per
// chain each) - the stages were 7 launches, each waiting for CU slots behind the far update
// (~60 us apiece there against ~15 alone)
__device__ __forceinline__ void own_stores_visible() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_zinv_level32(MatF A, int K, int m,
                                                      const float* __restrict__ Dinv,
                                                      int64_t dstride, float* zt, int64_t zstride,
                                                      Planes16 zpl, Live live,
                                                      const int* __restrict__ h3ok) {
    const int b = blockIdx.x >> 2, w = blockIdx.x & 3;
    if (!live32(live, b) || (h3ok && !h3ok[b])) return;
    const int p = w / m, tb = w % m;
    const int r0 = 2 * m * p + m, c0 = 2 * m * p;
    __shared__ GemmSmem32 sm;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const int r16 = lane & 15;
    float* Zr = zt + b * zstride;
    float* ZT = Zr + ZS * ZS;
    float* Tt = ZT + ZS * ZS;
    unsigned short* Zp = zpl.base + b * zpl.cstride;
    const float* Ab = A.base + b * A.cstride;
    if (m == 1) {  // the pair's diagonal tiles (row-major inverses in Dinv)
        for (int q = 0; q < 2; ++q) {
            const int t = c0 + q;
            const float* D = Dinv + b * dstride + (int64_t)(K + t) * 4096;
            for (int e = tid; e < 4096; e += 256) {
                const int r = e >> 6, c = e & 63;
                const float v = D[e];
                Zr[(int64_t)(64 * t + r) * ZS + 64 * t + c] = v;
                ZT[(int64_t)(64 * t + c) * ZS + 64 * t + r] = v;
                zput16(Zp, zpl, 64 * t + r, 64 * t + c, v);
            }
        }
        own_stores_visible();
    }
    f4_t acc[2][2];
    auto zero = [&]() {
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};
    };
    // column tb of T: T_a,tb = sum_{k=tb}^{m-1} L21_ak Z11_k,tb
    for (int ta = 0; ta < m; ++ta) {
        zero();
        tile_gemm_nt32<false>(acc, Ab + (int64_t)((K + r0 + ta) * 64) * A.ld + (K + c0 + tb) * 64,
                              A.ld, ZT + (int64_t)((c0 + tb) * 64) * ZS + (c0 + tb) * 64, ZS,
                              64 * (m - tb), sm, nullptr, 0);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = 32 * wr + 16 * bi + F32_CROW(lane, r), cc = 32 * wc + 16 * bj + r16;
                    Tt[(int64_t)((c0 + tb) * 64 + cc) * ZS + (r0 + ta) * 64 + rr] = acc[bi][bj][r];
                }
    }
    own_stores_visible();
    // column tb of Z21: Z21_a,tb = -sum_{k=0}^{a} Z22_ak T_k,tb
    for (int ta = 0; ta < m; ++ta) {
        zero();
        tile_gemm_nt32<true>(acc, Zr + (int64_t)((r0 + ta) * 64) * ZS + r0 * 64, ZS,
                             Tt + (int64_t)((c0 + tb) * 64) * ZS + r0 * 64, ZS, 64 * (ta + 1), sm,
                             nullptr, 0);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = 32 * wr + 16 * bi + F32_CROW(lane, r), cc = 32 * wc + 16 * bj + r16;
                    const float v = acc[bi][bj][r];
                    const int zr = (r0 + ta) * 64 + rr, zc = (c0 + tb) * 64 + cc;
                    Zr[(int64_t)zr * ZS + zc] = v;
                    ZT[(int64_t)zc * ZS + zr] = v;
                    zput16(Zp, zpl, zr, zc, v);
                }
    }
}

// k_panel_inv_gemm32: workgroup (chain b, row tiles i0 = Kend + 2p and i0 + 1) computes
// X_i = A_i Z^T for the panel's 8 column tiles in fp16x3 (A_i split while staged, Z from its
// planes by LDS-DMA). 8 waves: wave w takes row tile i0 + (w >> 2) and column tiles w & 3 and
// 7 - (w & 3) (depths (w & 3) + 1 and 8 - (w & 3) tiles: 9 each), so every staged Z slice feeds
// two row tiles (one row tile per workgroup staged Z per 64 output rows and left the loop waiting
// on its slices: 15 - 17 % MFMA busy). The workgroup reads its row tiles whole before it writes
// X in place (and the panel's planes for the trailing update). 160 KB of LDS: one workgroup per
// CU, two waves per SIMD.
struct __attribute__((aligned(16))) InvGemmSmem {
    _Float16 a[2][2][128][LPH];  // [buffer][hi, lo][row][k] (HS layout)
    _Float16 z[2][2][512][LPH];  // [buffer][hi, lo][Z row][k]
};
__global__ __launch_bounds__(512, 1) void k_panel_inv_gemm32(MatF A, int K, int Kend, int nb,
                                                             Planes16 zpl, Planes16 pl, Live live,
                                                             int nchains,
                                                             const int* __restrict__ h3ok) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, kq = lane >> 4;
    __shared__ InvGemmSmem sm;
    const int npair = (nb - Kend + 1) / 2;
    const long w = xcd_remap32((long)blockIdx.x, (long)npair * nchains);
    const int b = (int)(w / npair), i0 = Kend + 2 * (int)(w % npair);
    const bool two = i0 + 1 < nb;  // (an odd count leaves the last workgroup one row tile)
    if (!live32(live, b) || (h3ok && !h3ok[b])) return;
    float* Ab = A.base + b * A.cstride + (int64_t)(i0 * 64) * A.ld + K * 64;
    const int rt = wv >> 2, c0 = wv & 3, c1 = 7 - (wv & 3);
    f4_t acc0[4][4], acc1[4][4];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) {
            acc0[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};
            acc1[bi][bj] = f4_t{0.f, 0.f, 0.f, 0.f};
        }
    // A staging: thread t moves row t/4 (of the two row tiles; a missing second tile re-reads the
    // first), k 8(t%4) .. +7 of the 32-deep slice (split in registers)
    const int arow = tid >> 2, acol = 8 * (tid & 3);
    const float* ag = Ab + (int64_t)((two || arow < 64) ? arow : arow - 64) * A.ld + acol;
    f4_t ra0, ra1;
    auto aload = [&](int sidx) {
        ra0 = *reinterpret_cast<const f4_t*>(ag + KS128 * sidx);
        ra1 = *reinterpret_cast<const f4_t*>(ag + KS128 * sidx + 4);
    };
    auto astore = [&](int buf) {
        h4_t h0, l0, h1, l1;
        split_h3(ra0, h0, l0);
        split_h3(ra1, h1, l1);
        const h8_t hi = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        const h8_t lo = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        *reinterpret_cast<h8_t*>(&sm.a[buf][0][arow][HS(arow, acol)]) = hi;
        *reinterpret_cast<h8_t*>(&sm.a[buf][1][arow][HS(arow, acol)]) = lo;
    };
    // Z staging by LDS-DMA: rows [64 kb, 512) of slice s (the column tiles that need it); wave
    // wv takes plane wv & 1 and the 16-row groups g = (wv >> 1) + 4t; lane l: row 16g + l/4,
    // LDS slot l%4 = logical piece (l%4) ^ (bit 3 of the row)
    const int rowl = lane >> 2, piece = (lane & 3) ^ ((rowl >> 2) & 2), pln = wv & 1;
    const unsigned short* zg = zpl.base + b * zpl.cstride + (pln ? zpl.lo : 0) +
                               (int64_t)rowl * 32 + piece * 8;
    auto dma = [&](int sidx, int buf) {
        const int kb = sidx >> 1;
        for (int g = 4 * kb + (wv >> 1); g < 32; g += 4)
            __builtin_amdgcn_global_load_lds(
                (glb_void_t*)(zg + ((int64_t)sidx * zpl.rows + 16 * g) * 32),
                (lds_void_t*)&sm.z[buf][pln][16 * g][0], 16, 0, 0);
    };
    auto mm = [&](f4_t (&acc)[4][4], int cc, int cur) {
        h8_t bh[4], bl[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int row = 64 * cc + 16 * x + r16;
            bh[x] = *reinterpret_cast<const h8_t*>(&sm.z[cur][0][row][HS(row, 8 * kq)]);
            bl[x] = *reinterpret_cast<const h8_t*>(&sm.z[cur][1][row][HS(row, 8 * kq)]);
        }
#pragma unroll
        for (int bi = 0; bi < 4; ++bi) {
            const int row = 64 * rt + 16 * bi + r16;
            const h8_t ah = *reinterpret_cast<const h8_t*>(&sm.a[cur][0][row][HS(row, 8 * kq)]);
            const h8_t al = *reinterpret_cast<const h8_t*>(&sm.a[cur][1][row][HS(row, 8 * kq)]);
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[bj], acc[bi][bj], 0, 0, 0);
                acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[bj], acc[bi][bj], 0, 0, 0);
                acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[bj], acc[bi][bj], 0, 0, 0);
            }
        }
    };
    const bool mine = two || rt == 0;  // a missing second row tile: its waves only stage
    constexpr int nsub = 512 / KS128;
    aload(0);
    dma(0, 0);
    astore(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nsub; ++s) {
        if (s + 1 < nsub) {
            aload(s + 1);
            dma(s + 1, (s + 1) & 1);
        }
        const int kb = s >> 1;
        if (mine && kb <= c0) mm(acc0, c0, s & 1);
        if (mine && kb <= c1) mm(acc1, c1, s & 1);
        if (s + 1 < nsub) astore((s + 1) & 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // X in place (both row tiles were read whole above) and the panel's planes, one output
    // column tile at a time through LDS (the loop ended on a barrier; each wave its own 64 x 68
    // fp32 region): the accumulators go in by ds_write_b32, then every lane moves 8 consecutive
    // columns of a row - two 16-byte stores of X, one 16-byte store each of its hi and lo planes
    // (round 6: the accumulator layout, 4 rows x 1 column per lane and block, went out as 4-byte
    // stores of X and 2-byte plane stores, 3 scattered stores per element: 4 VALU per MFMA and
    // the fabric's narrow-store cost in the counters, profiles/r05_pmc_newton_final.txt)
    const int i = i0 + rt;
    float* Ai = Ab + (int64_t)(rt * 64) * A.ld;
    const bool planes = pl.base && (i + 1) * 64 <= pl.rows;
    constexpr int EP = 68;  // LDS row pitch (floats): 16-byte rows, lane groups 4 rows apart
                            // on different banks
    float* ew = reinterpret_cast<float*>(&sm) + wv * (64 * EP);
    auto put = [&](const f4_t (&acc)[4][4], int cc) {
        if (mine) {
#pragma unroll
            for (int bi = 0; bi < 4; ++bi)
#pragma unroll
                for (int bj = 0; bj < 4; ++bj)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        ew[(16 * bi + F32_CROW(lane, r)) * EP + 16 * bj + r16] = acc[bi][bj][r];
        }
        __syncthreads();
        if (mine) {
            // lane: row 8q + (lane >> 3), columns 8 (lane & 7) .. +7 of the tile
            const int c8 = 8 * (lane & 7), col = 64 * cc + c8;
            unsigned short* hp =
                planes ? pl.base + b * pl.cstride + (int64_t)(col >> 5) * pl.rows * 32 + (col & 31)
                       : nullptr;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int rr = 8 * q + (lane >> 3);
                const f4_t v0 = *reinterpret_cast<const f4_t*>(ew + rr * EP + c8);
                const f4_t v1 = *reinterpret_cast<const f4_t*>(ew + rr * EP + c8 + 4);
                float* dst = Ai + (int64_t)rr * A.ld + col;
                *reinterpret_cast<f4_t*>(dst) = v0;
                *reinterpret_cast<f4_t*>(dst + 4) = v1;
                if (planes) {
                    h4_t h0, l0, h1, l1;
                    split_h3(v0, h0, l0);
                    split_h3(v1, h1, l1);
                    const h8_t hi = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                    const h8_t lo = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
                    unsigned short* o = hp + (int64_t)(i * 64 + rr) * 32;
                    *reinterpret_cast<h8_t*>(o) = hi;
                    *reinterpret_cast<h8_t*>(o + pl.lo) = lo;
                }
            }
        }
        __syncthreads();  // (the region is rewritten for the second column tile)
    };
    put(acc0, c0);
    put(acc1, c1);
}

void launch_panel_inv32(MatF A, int K, int nb, const float* Dinv, int64_t dstride, float* zt,
                        int64_t zstride, Planes16 zpl, Planes16 pl, Live live, int nchains,
                        const int* h3ok, hipStream_t s) {
    for (int m = 1; m <= 4; m *= 2)
        APM_LAUNCH(k_zinv_level32, dim3((unsigned)(4 * nchains)), dim3(256), 0, s, A, K,
                           m, Dinv, dstride, zt, zstride, zpl, live, h3ok);
    const int Kend = K + 8;
    if (nb > Kend)
        APM_LAUNCH(k_panel_inv_gemm32,
                           dim3((unsigned)((long)((nb - Kend + 1) / 2) * nchains)), dim3(512), 0,
                           s, A, K, Kend, nb, zpl, pl, live, nchains, h3ok);
}

// Host: 256x256 quad tiles covering tiles (i, j), i in [i0, R), j0 <= j <= min(i, jend-1), in
// 2x2-quad blocks (8x8 tiles, the L2 locality of build_update_supertiles)
std::vector<unsigned> build_update_quads(int i0, int R, int j0, int jend) {
    std::vector<unsigned> v;
    const int nr = (R - i0 + 3) / 4, nc = (jend - j0 + 3) / 4, S = 2;
    for (int P = 0; P < nr; P += S)
        for (int Q = 0; Q < nc; Q += S)
            for (int p = P; p < std::min(P + S, nr); ++p)
                for (int q = Q; q < std::min(Q + S, nc); ++q) {
                    const int I = i0 + 4 * p, Jq = j0 + 4 * q;
                    unsigned rm = 0, cm = 0;
                    for (int a = 0; a < 4; ++a) {
                        if (I + a < R) rm |= 1u << a;
                        if (Jq + a < jend) cm |= 1u << a;
                    }
                    bool any = false;
                    for (int a = 0; a < 4; ++a)
                        for (int c = 0; c < 4; ++c)
                            any |= ((rm >> a) & 1) && ((cm >> c) & 1) && Jq + c <= I + a;
                    if (!any) continue;
                    v.push_back(((unsigned)I << 20) | ((unsigned)Jq << 8) | (rm << 4) | cm);
                }
    return v;
}

// Host: 128x128 super-tiles covering tiles (i, j), i in [i0, R) minus the row gap [glo, ghi),
// j0 <= j <= min(i, jend-1), in 4x4-super-tile blocks (the L2 locality of build_update_tiles);
// super-tile rows start at i0, columns at j0. Entries without any valid tile are omitted.
std::vector<unsigned> build_update_supertiles(int i0, int R, int j0, int jend, int glo, int ghi,
                                              int solo) {
    std::vector<unsigned> v;
    auto rowv = [&](int i) { return i < R && !(i >= glo && i < ghi); };
    const int S = 4;  // super-tiles per block edge (8x8 tiles, as build_update_tiles)
    std::vector<int> rows;  // first row tile of each super-tile row; rows[p] + 1 valid iff paired
    std::vector<bool> pair;
    for (int i = i0; i < R;) {
        const bool two = i != solo && i + 1 != solo;
        rows.push_back(i);
        pair.push_back(two);
        i += two ? 2 : 1;
    }
    const int nr = (int)rows.size(), nc = (jend - j0 + 1) / 2;
    for (int P = 0; P < nr; P += S)
        for (int Q = 0; Q < nc; Q += S)
            for (int p = P; p < std::min(P + S, nr); ++p)
                for (int q = Q; q < std::min(Q + S, nc); ++q) {
                    const int i = rows[p], j = j0 + 2 * q;
                    const bool rv0 = rowv(i), rv1 = pair[p] && rowv(i + 1);
                    const bool cv0 = j < jend, cv1 = j + 1 < jend;
                    bool any = false;
                    for (int a = 0; a < 2; ++a)
                        for (int c = 0; c < 2; ++c)
                            any |= (a ? rv1 : rv0) && (c ? cv1 : cv0) && j + c <= i + a;
                    if (!any) continue;
                    v.push_back(((unsigned)i << 18) | ((unsigned)j << 4) | (rv0 ? 1u : 0u) |
                                (rv1 ? 2u : 0u) | (cv0 ? 4u : 0u) | (cv1 ? 8u : 0u));
                }
    return v;
}

// ------------------------------------------------------------------------------- B in fp32
// (formed by k_symv_part in the same pass as K b, below)

// out[b][:] = row `row` of Bf (fp32 -> fp64)
__global__ __launch_bounds__(256) void k_row32(MatF Bf, int64_t row, int np, double* out,
                                               int64_t ostride, Live live) {
    const int b = blockIdx.y;
    if (!live32(live, b)) return;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < np) out[b * ostride + c] = (double)Bf.base[b * Bf.cstride + row * Bf.ld + c];
}

void launch_row32(MatF Bf, int64_t row, int np, double* out, int64_t ostride, Live live,
                  int nchains, hipStream_t s) {
    APM_LAUNCH(k_row32, dim3((np + 255) / 256, nchains), dim3(256), 0, s, Bf, row, np,
                       out, ostride, live);
}

// ------------------------------------------------------------------------------- K x (symmetric)
// y = K x reading only K's lower tiles (half the bytes of a full GEMV): workgroup (ti, tj) reads
// tile K_ij straight into registers - thread t holds rows 4(t/16) .. +3, columns 4(t%16) .. +3
// (8 x 16-byte loads, 512-byte rows per 16 lanes, all issued at once) - and writes the partial
// products K_ij x_j (row sums: 16-lane shuffles) to part[ti][tj] and, off the diagonal, K_ij^T x_i
// (column sums: shuffles across the 4 row groups of a wave, then the 4 waves through LDS) to
// part[tj][ti]; k_symv_reduce adds the nb partials of every row in a fixed order (deterministic,
// no atomics). With `Bf` set, the same pass also writes the fp32 Newton matrix tile
// I + W^1/2 K W^1/2 (fusing k_form_B32 into the x = b pass).
// TPW > 1: a workgroup takes TPW consecutive tiles of its chain, the next tile's 32 KB loaded
// into registers while the current one is reduced (the same per-tile sums: bitwise equal)
__device__ __forceinline__ void symv_tile_ij(int t, int& ti, int& tj) {
    ti = (int)floor((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}
template <int TPW>
__global__ __launch_bounds__(256) void k_symv_part(MatB K, const double* __restrict__ x,
                                                   int64_t xstride, double* __restrict__ part,
                                                   int64_t pstride, int nb, MatF Bf,
                                                   const double* __restrict__ Ws, int64_t wstride,
                                                   Live live) {
    const int b = blockIdx.y;
    if (!live32(live, b)) return;
    const int ntile = nb * (nb + 1) / 2;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rg = tid >> 4, cg = tid & 15;  // rows 4rg .. 4rg+3, columns 4cg .. 4cg+3
    __shared__ double cs[4][64];
    auto load = [&](int t, d2_t (&v)[4][2]) {
        int ti, tj;
        symv_tile_ij(t, ti, tj);
        const double* Kt =
            K.base + b * K.cstride + (int64_t)(ti * 64 + 4 * rg) * K.ld + tj * 64 + 4 * cg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[r][0] = *reinterpret_cast<const d2_t*>(Kt + (int64_t)r * K.ld);
            v[r][1] = *reinterpret_cast<const d2_t*>(Kt + (int64_t)r * K.ld + 2);
        }
    };
    int t = blockIdx.x * TPW;
    d2_t v[4][2];
    load(t, v);
    for (int tt = 0; tt < TPW && t < ntile; ++tt, ++t) {
        d2_t vn[4][2];
        if (TPW > 1 && tt + 1 < TPW && t + 1 < ntile) load(t + 1, vn);
        int ti, tj;
        symv_tile_ij(t, ti, tj);
        const double* xb = x + b * xstride;
        const d2_t xj0 = *reinterpret_cast<const d2_t*>(xb + tj * 64 + 4 * cg);
        const d2_t xj1 = *reinterpret_cast<const d2_t*>(xb + tj * 64 + 4 * cg + 2);
        const d2_t xi0 = *reinterpret_cast<const d2_t*>(xb + ti * 64 + 4 * rg);
        const d2_t xi1 = *reinterpret_cast<const d2_t*>(xb + ti * 64 + 4 * rg + 2);
        const double xjv[4] = {xj0.x, xj0.y, xj1.x, xj1.y}, xiv[4] = {xi0.x, xi0.y, xi1.x, xi1.y};
        if (Bf.base) {
            const double* wb = Ws + b * wstride;
            float* Fb = Bf.base + b * Bf.cstride + (int64_t)(ti * 64 + 4 * rg) * Bf.ld + tj * 64 +
                        4 * cg;
            const int gr0 = ti * 64 + 4 * rg, gc0 = tj * 64 + 4 * cg;
            const d2_t wc0 = *reinterpret_cast<const d2_t*>(wb + gc0);
            const d2_t wc1 = *reinterpret_cast<const d2_t*>(wb + gc0 + 2);
            const double wcv[4] = {wc0.x, wc0.y, wc1.x, wc1.y};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double wr_ = wb[gr0 + r];
                const double kv[4] = {v[r][0].x, v[r][0].y, v[r][1].x, v[r][1].y};
                f4_t o;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    o[c] = (float)((gr0 + r == gc0 + c ? 1.0 : 0.0) + (wr_ * kv[c]) * wcv[c]);
                *reinterpret_cast<f4_t*>(Fb + (int64_t)r * Bf.ld) = o;
            }
        }
        double* pb = part + b * pstride;
        // row sums over this thread's 4 columns, then over the 16 lanes of the row group
        double rs[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double sr = v[r][0].x * xjv[0];
            sr = fma(v[r][0].y, xjv[1], sr);
            sr = fma(v[r][1].x, xjv[2], sr);
            sr = fma(v[r][1].y, xjv[3], sr);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sr += __shfl_xor(sr, o, 64);
            rs[r] = sr;
        }
        if (cg < 4) pb[((int64_t)ti * nb + tj) * 64 + 4 * rg + cg] = rs[cg];
        if (ti != tj) {  // (uniform per workgroup)
            // column sums over this thread's 4 rows, then over the 4 row groups of the wave and
            // the 4 waves
            double csum[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double kc0 = c < 2 ? (c == 0 ? v[0][0].x : v[0][0].y) : (c == 2 ? v[0][1].x : v[0][1].y);
                const double kc1 = c < 2 ? (c == 0 ? v[1][0].x : v[1][0].y) : (c == 2 ? v[1][1].x : v[1][1].y);
                const double kc2 = c < 2 ? (c == 0 ? v[2][0].x : v[2][0].y) : (c == 2 ? v[2][1].x : v[2][1].y);
                const double kc3 = c < 2 ? (c == 0 ? v[3][0].x : v[3][0].y) : (c == 2 ? v[3][1].x : v[3][1].y);
                double sc = kc0 * xiv[0];
                sc = fma(kc1, xiv[1], sc);
                sc = fma(kc2, xiv[2], sc);
                sc = fma(kc3, xiv[3], sc);
                sc += __shfl_xor(sc, 16, 64);
                sc += __shfl_xor(sc, 32, 64);
                csum[c] = sc;
            }
            if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 4; ++c) cs[w][4 * lane + c] = csum[c];
            }
            __syncthreads();
            if (tid < 64)
                pb[((int64_t)tj * nb + ti) * 64 + tid] = cs[0][tid] + cs[1][tid] + cs[2][tid] + cs[3][tid];
            if (TPW > 1) __syncthreads();  // cs is rewritten by the next tile
        }
        if (TPW > 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r][0] = vn[r][0];
                v[r][1] = vn[r][1];
            }
        }
    }
}

// y[i] = sum_tj part[i/64][tj][i%64]; with Bf: also the Newton right-hand-side block of the fp32
// matrix (row np = W^1/2 y, rows np+1 .. np+63 zero)
__global__ __launch_bounds__(256) void k_symv_reduce(const double* __restrict__ part,
                                                     int64_t pstride, int nb, double* y,
                                                     int64_t ystride, MatF Bf,
                                                     const double* __restrict__ Ws,
                                                     int64_t wstride, Live live) {
    const int b = blockIdx.y;
    if (!live32(live, b)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int np = nb * 64;
    if (i >= np) return;
    const double* pb = part + b * pstride + (int64_t)(i >> 6) * nb * 64 + (i & 63);
    // 16 loads in flight per thread, then added in the same order (a rolled loop waited for
    // each load in turn)
    double s = 0.0;
    int tj = 0;
    for (; tj + 16 <= nb; tj += 16) {
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = pb[(int64_t)(tj + q) * 64];
#pragma unroll
        for (int q = 0; q < 16; ++q) s += v[q];
    }
    for (; tj < nb; ++tj) s += pb[(int64_t)tj * 64];
    y[b * ystride + i] = s;
    if (Bf.base) {
        float* col = Bf.base + b * Bf.cstride + (int64_t)np * Bf.ld + i;
        col[0] = (float)(Ws[b * wstride + i] * s);
        for (int r = 1; r < 64; ++r) col[(int64_t)r * Bf.ld] = 0.0f;
    }
}

void launch_symv(MatB K, const double* x, int64_t xstride, double* y, int64_t ystride,
                 double* part, int64_t pstride, int np, MatF Bf, const double* Ws,
                 int64_t wstride, Live live, int nchains, hipStream_t s, int symv_tpw) {
    const int nb = np / 64, nt = nb * (nb + 1) / 2;
    if (symv_tpw >= 4)
        APM_LAUNCH(k_symv_part<4>, dim3((nt + 3) / 4, nchains), dim3(256), 0, s, K, x,
                           xstride, part, pstride, nb, Bf, Ws, wstride, live);
    else if (symv_tpw == 2)
        APM_LAUNCH(k_symv_part<2>, dim3((nt + 1) / 2, nchains), dim3(256), 0, s, K, x,
                           xstride, part, pstride, nb, Bf, Ws, wstride, live);
    else
        APM_LAUNCH(k_symv_part<1>, dim3(nt, nchains), dim3(256), 0, s, K, x, xstride,
                           part, pstride, nb, Bf, Ws, wstride, live);
    APM_LAUNCH(k_symv_reduce, dim3((np + 255) / 256, nchains), dim3(256), 0, s, part,
                       pstride, nb, y, ystride, Bf, Ws, wstride, live);
}

// ------------------------------------------------------------------------------- TRSV
// 64x64 fp32 tile -> LDS (pitch 65), coalesced rows; thread (q, c) then reads row c.
__device__ __forceinline__ void stage_tile32(float (*T)[65], const float* src, int64_t ld) {
    for (int e = threadIdx.x; e < 4096; e += 256) T[e >> 6][e & 63] = src[(int64_t)(e >> 6) * ld + (e & 63)];
}

// Forward step J (J = 0 .. nb-1) of L y = r: every workgroup forms y_J = inv(L_JJ) r_J; workgroup
// I == J stores it, workgroups I > J update r_I -= L_IJ y_J (r updated in place).
__global__ __launch_bounds__(256) void k_trsv_fwd32(MatF A, int J, const float* Dinv,
                                                    int64_t dstride, double* r, double* y,
                                                    int64_t vstride, Live live) {
    const int b = blockIdx.y;
    if (!live32(live, b)) return;
    const int I = J + blockIdx.x;
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    __shared__ float T[64][65];
    __shared__ double vj[64];
    __shared__ double part[4][64];
    double* rb = r + b * vstride;
    stage_tile32(T, Dinv + b * dstride + (int64_t)J * 4096, 64);
    if (tid < 64) vj[tid] = rb[J * 64 + tid];
    __syncthreads();
    double s = 0.0;
    for (int m = q * 16; m < q * 16 + 16; ++m) s += (double)T[c][m] * vj[m];
    part[q][c] = s;
    __syncthreads();
    const double yc = part[0][c] + part[1][c] + part[2][c] + part[3][c];
    if (I == J) {
        if (tid < 64) y[b * vstride + J * 64 + tid] = yc;
        return;
    }
    __syncthreads();  // part and T are reused
    if (tid < 64) vj[tid] = yc;
    stage_tile32(T, A.base + b * A.cstride + (int64_t)(I * 64) * A.ld + J * 64, A.ld);
    __syncthreads();
    s = 0.0;
    for (int m = q * 16; m < q * 16 + 16; ++m) s += (double)T[c][m] * vj[m];
    part[q][c] = s;
    __syncthreads();
    if (tid < 64) rb[I * 64 + tid] -= part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
}

// Backward step J (J = nb-1 .. 0) of L^T z = r: z_J = inv(L_JJ)^T r_J; I < J: r_I -= L_JI^T z_J.
// The transposed products read tile rows with consecutive lanes on consecutive columns.
__global__ __launch_bounds__(256) void k_trsv_bwd32(MatF A, int J, const float* Dinv,
                                                    int64_t dstride, double* r, double* z,
                                                    int64_t vstride, Live live) {
    const int b = blockIdx.y;
    if (!live32(live, b)) return;
    const int I = blockIdx.x;
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    __shared__ double vj[64];
    __shared__ double part[4][64];
    __shared__ double zj[64];
    double* rb = r + b * vstride;
    if (tid < 64) vj[tid] = rb[J * 64 + tid];
    __syncthreads();
    const float* D = Dinv + b * dstride + (int64_t)J * 4096;
    double s = 0.0;
    for (int m = q * 16; m < q * 16 + 16; ++m) s += (double)D[m * 64 + c] * vj[m];
    part[q][c] = s;
    __syncthreads();
    if (tid < 64) zj[tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    __syncthreads();
    if (I == J) {
        if (tid < 64) z[b * vstride + J * 64 + tid] = zj[tid];
        return;
    }
    const float* L = A.base + b * A.cstride + (int64_t)(J * 64) * A.ld + I * 64;
    s = 0.0;
    for (int m = q * 16; m < q * 16 + 16; ++m) s += (double)L[(int64_t)m * A.ld + c] * zj[m];
    part[q][c] = s;
    __syncthreads();
    if (tid < 64) rb[I * 64 + tid] -= part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
}

#define TRF_MAXNP 8192  // the multi-workgroup TRSV keeps the solution in LDS (fp64)

// ------------------------------------------------------- multi-workgroup TRSV (G workgroups/chain)
// The solve of one chain split over G workgroups of 256 threads: workgroup g owns the block steps
// s = g, g+G, g+2G, ... (FWD: J = s, BWD: J = nb-1-s) and, for its step, streams the block row's
// tiles against the solution blocks of the earlier steps, taken from an LDS copy of the solution
// that it refreshes from global memory. Steps hand over through the solution itself: `out` is
// NaN-filled before the launch (k_nan_fill) and every element is published with an agent-scope
// atomic store; readers poll each element they need with agent-scope atomic loads until it is not
// NaN (no flags, no fences: each value carries its own readiness, and gfx950 agent-scope atomics
// bypass the XCD-private L2). The contributions of all but the previous step's block are summed
// before waiting for it, so the critical path per step is one hand-over, one tile and the 64x64
// inverse product. Polling is bounded (SpinCtl.limit polls per element): a chain whose solution
// never appears (a NaN produced by the factor, or a hand-over that took too long) is marked
// failed and counted (APM_PROF_TRSV_TIMEOUTS) instead of spinning; the Newton loop reruns it in
// fp64. Roles come from arrival tickets (SpinCtl): chain b is served by tickets bG .. bG+G-1, so
// the G roles of every chain but the one holding the newest ticket have all arrived - at most
// G - 1 workgroups of a launch can wait on one that has not (role g waits on every role, the
// round-robin step order has no lower-index-only form), and they wait only until any other
// workgroup on the GPU retires and frees a slot for it.
#define TRM_G 8         // workgroups per chain
#define TRM_CHUNK 4     // solution blocks fetched per poll round
__global__ __launch_bounds__(256) void k_nan_fill(double* out, int64_t vstride, int np,
                                                  Live live) {
    const int b = blockIdx.y;
    if (!live32(live, b)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < np) out[b * vstride + i] = __builtin_nan("");
}

template <bool FWD>
__global__ __launch_bounds__(256) void k_trsv32_mw(MatF A, int nb, const float* Dinv,
                                                   int64_t dstride, const double* r, double* out,
                                                   int64_t vstride, Live live, int fail_code,
                                                   int G, int nchains, SpinCtl sc) {
    __shared__ int bad;
    __shared__ unsigned long long tk;
    if (threadIdx.x == 0) {
        bad = 0;
        tk = __hip_atomic_fetch_add(sc.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) -
             sc.base;
    }
    __syncthreads();  // `bad` is read by every poll loop
    if (tk >= (unsigned long long)nchains * G) {
        // tickets out of step with the host's count (a launch that never ran): fail every chain
        // of the launch (fp64 rerun) rather than leave a role unserved
        if (threadIdx.x == 0) {
            for (int c = 0; c < nchains; ++c) live.status[c] = fail_code;
            atomicAdd(sc.timeouts, 1ull);
        }
        return;
    }
    const int b = (int)(tk / G), g = (int)(tk % G);
    if (!live32(live, b)) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int row = t >> 2, q = t & 3;  // tile row, 16-column quarter
    extern __shared__ double trm_sm[];
    double* xs = trm_sm;               // np: solution blocks fetched so far (solve order)
    double* red = xs + nb * 64;        // 4 x 64 column-sum partials (BWD)
    double* rj = red + 4 * 64;         // 64: right-hand side of the step
    const float* Lb = A.base + b * A.cstride;
    const float* Db = Dinv + b * dstride;
    const double* rb = r + b * vstride;
    double* ob = out + b * vstride;
    auto blk = [&](int idx) { return FWD ? idx : nb - 1 - idx; };  // solve order -> block
    // fetch solution blocks of solve-order indices [a, e) into LDS (polling)
    auto fetch = [&](int a, int e) {
        for (int x = t; x < (e - a) * 64; x += 256) {
            const int I = blk(a + x / 64), o = I * 64 + (x & 63);
            double v = __hip_atomic_load(ob + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int n = 0;
            while (__builtin_isnan(v) && n < sc.limit && !bad) {
                __builtin_amdgcn_s_sleep(1);
                v = __hip_atomic_load(ob + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ++n;
            }
            if (__builtin_isnan(v)) bad = 1;
            xs[o] = v;
        }
    };
    // 16-byte pieces of tile (J, I) (FWD: L_JI) or (I, J) (BWD: L_IJ) for this thread
    auto piece = [&](int J, int I, int u) -> f4_t {
        const int64_t o = FWD ? (int64_t)(J * 64 + row) * A.ld + I * 64 + 16 * q + 4 * u
                              : (int64_t)(I * 64 + row) * A.ld + J * 64 + 16 * q + 4 * u;
        return *reinterpret_cast<const f4_t*>(Lb + o);
    };
    int have = 0;  // solve-order blocks [0, have) are in LDS
    for (int s = g; s < nb; s += G) {
        const int J = blk(s);
        // the step's critical-path operands, independent of the solution: the previous step's
        // tile and this thread's 16 entries of inv(L_JJ), loaded before any wait
        f4_t plast[4];
        if (s > 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) plast[u] = piece(J, blk(s - 1), u);
        }
        float dreg[16];
        {
            const float* D = Db + (int64_t)J * 4096;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                dreg[e] = FWD ? D[row * 64 + 16 * q + e] : D[(16 * q + e) * 64 + row];
        }
        double acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = 0.0;
        // all earlier blocks but the previous step's, then that one; the early tiles stream with
        // two tiles' loads in flight ahead of the one being consumed (the step's critical path
        // is this one workgroup's read of its block row). The solution blocks this workgroup
        // has not seen yet (the other roles' last steps) are fetched only when the stream reaches
        // them, so the tiles of the blocks already in LDS are read while those steps finish.
        const int early = s > 0 ? s - 1 : 0;
        auto ensure = [&](int idx) {  // (uniform: `have` is the same in every thread)
            if (idx < have) return;
            const int e = early < have + TRM_CHUNK ? early : have + TRM_CHUNK;
            fetch(have, e);
            have = e;
            __syncthreads();
        };
        __syncthreads();
        {
            f4_t p0[4], p1[4], p2[4];
            auto ld4 = [&](f4_t (&v)[4], int idx) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = piece(J, blk(idx), u);
            };
            auto use = [&](const f4_t (&v)[4], int I) {
                if (FWD) {
                    const double* x = xs + I * 64 + 16 * q;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[0] = fma((double)v[u][e], x[4 * u + e], acc[0]);
                } else {
                    const double x = xs[I * 64 + row];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[4 * u + e] = fma((double)v[u][e], x, acc[4 * u + e]);
                }
            };
            if (early > 0) ld4(p0, 0);
            if (early > 1) ld4(p1, 1);
            int idx = 0;
            for (; idx + 2 < early; idx += 3) {  // same order of accumulation as one at a time
                ld4(p2, idx + 2);
                ensure(idx);
                use(p0, blk(idx));
                if (idx + 3 < early) ld4(p0, idx + 3);
                ensure(idx + 1);
                use(p1, blk(idx + 1));
                if (idx + 4 < early) ld4(p1, idx + 4);
                ensure(idx + 2);
                use(p2, blk(idx + 2));
            }
            if (idx < early) {
                ensure(idx);
                use(p0, blk(idx));
            }
            if (idx + 1 < early) {
                ensure(idx + 1);
                use(p1, blk(idx + 1));
            }
            if (s > 0) {
                if (have < s) {
                    fetch(s - 1, s);
                    have = s;
                }
                __syncthreads();
                use(plast, blk(s - 1));
            }
        }
        if (FWD) {
            double sum = acc[0];
            sum += __shfl_xor(sum, 1, 64);
            sum += __shfl_xor(sum, 2, 64);
            if (q == 0) rj[row] = rb[J * 64 + row] - sum;
        } else {  // column sums: lanes 4*(row%16) + q share columns 16q..16q+15
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                acc[c] += __shfl_xor(acc[c], 4, 64);
                acc[c] += __shfl_xor(acc[c], 8, 64);
                acc[c] += __shfl_xor(acc[c], 16, 64);
                acc[c] += __shfl_xor(acc[c], 32, 64);
            }
            if (lane < 4) {
#pragma unroll
                for (int c = 0; c < 16; ++c) red[w * 64 + 16 * lane + c] = acc[c];
            }
            __syncthreads();
            if (t < 64) rj[t] = rb[J * 64 + t] - (red[t] + red[64 + t] + red[128 + t] + red[192 + t]);
        }
        __syncthreads();
        // x_J[c] = sum_m inv(L_JJ)[c][m] rj[m] (FWD) or inv(L_JJ)[m][c] rj[m] (BWD): thread (c, q)
        // sums m = 16q .. 16q+15
        {
            double sum = 0.0;
#pragma unroll
            for (int e = 0; e < 16; ++e) sum = fma((double)dreg[e], rj[16 * q + e], sum);
            sum += __shfl_xor(sum, 1, 64);
            sum += __shfl_xor(sum, 2, 64);
            if (q == 0) {
                xs[J * 64 + row] = sum;
                __hip_atomic_store(ob + J * 64 + row, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    __syncthreads();
    if (t == 0 && bad) {
        live.status[b] = fail_code;
        atomicAdd(sc.timeouts, 1ull);
    }
}

bool trsv32_mw_ok(int np) { return np <= TRF_MAXNP; }

// dynamic LDS above the default 64 KiB cap (np up to TRF_MAXNP); apm_create calls it with the
// context's device current
void trsv32_mw_init() {
    const int mx = (int)(sizeof(double) * (TRF_MAXNP + 4 * 64 + 64));
    (void)hipFuncSetAttribute((const void*)k_trsv32_mw<true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, mx);
    (void)hipFuncSetAttribute((const void*)k_trsv32_mw<false>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, mx);
}

long launch_trsv32_mw(bool fwd, MatF A, int nb, const float* Dinv, int64_t dstride,
                      const double* r, double* out, int64_t vstride, Live live, int nchains,
                      int fail_code, SpinCtl sc, hipStream_t s) {
    const size_t lds = sizeof(double) * (nb * 64 + 4 * 64 + 64);
    const int np = nb * 64;
    const int G = TRM_G;
    APM_LAUNCH(k_nan_fill, dim3((np + 255) / 256, nchains), dim3(256), 0, s, out, vstride,
                       np, live);
    if (fwd)
        APM_LAUNCH(k_trsv32_mw<true>, dim3(nchains * G), dim3(256), lds, s, A, nb,
                           Dinv, dstride, r, out, vstride, live, fail_code, G, nchains, sc);
    else
        APM_LAUNCH(k_trsv32_mw<false>, dim3(nchains * G), dim3(256), lds, s, A, nb,
                           Dinv, dstride, r, out, vstride, live, fail_code, G, nchains, sc);
    return (long)nchains * G;
}

void launch_trsv_fwd32(MatF A, int J, int nb, const float* Dinv, int64_t dstride, double* r,
                       double* y, int64_t vstride, Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_trsv_fwd32, dim3(nb - J, nchains), dim3(256), 0, s, A, J, Dinv, dstride,
                       r, y, vstride, live);
}

void launch_trsv_bwd32(MatF A, int J, const float* Dinv, int64_t dstride, double* r, double* z,
                       int64_t vstride, Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_trsv_bwd32, dim3(J + 1, nchains), dim3(256), 0, s, A, J, Dinv, dstride,
                       r, z, vstride, live);
}

// ------------------------------------------------------------------------------- refinement
// mode 0: t = Ws * x                                 (before the fp64 gemv Kt = K t)
// mode 1: res = Ws * Kb - x - Ws * Kt                (residual of B x = W^1/2 K b)
// mode 2: x += d                                     (corrected solution)
// mode 3: out = 0                                    (Newton start f = 0 of the live chains)
__global__ __launch_bounds__(256) void k_refine(int mode, const double* __restrict__ Ws,
                                                const double* __restrict__ Kb, double* x,
                                                const double* __restrict__ Kt, double* out,
                                                int64_t vstride, int np, Live live) {
    const int b = blockIdx.y;
    if (!live32(live, b)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const int64_t o = b * vstride + i;
    if (mode == 0)
        out[o] = Ws[o] * x[o];
    else if (mode == 1)
        out[o] = Ws[o] * Kb[o] - x[o] - Ws[o] * Kt[o];
    else if (mode == 2)
        x[o] += out[o];
    else
        out[o] = 0.0;
}

// Acceptance test of refinement step `step` (0-based), run after x += d on the chains still
// refining (live.active = the refining mask). The error left after a correction d_k is about
// rho |d_k| with the contraction rho ~ |d_k| / |d_{k-1}| (d_0 = the first solve x), so a chain
// is accepted when max|d_k|^2 <= tol^2 max|x| max|d_{k-1}| — for the first step exactly
// max|d| <= tol max|x| (refined error ~ tol^2 relative). Accepted chains leave the refining mask;
// after the last allowed step the others get status = fail_code, which sends them to the fp64
// rerun (host_newton.cpp newton_is): the fp32 factor is too inaccurate for them (extreme theta).
// prev[b] keeps max|d_{k-1}|.
__global__ __launch_bounds__(256) void k_refine_check(const double* __restrict__ x,
                                                      const double* __restrict__ d,
                                                      int64_t vstride, int np, double tol,
                                                      int fail_code, int step, int last,
                                                      double* prev, int* refining, Live live) {
    const int b = blockIdx.x;
    if (!live32(live, b)) return;
    double mx = 0.0, md = 0.0;
#pragma unroll 4  // (loads of 4 steps in flight)
    for (int i = threadIdx.x; i < np; i += 256) {
        mx = fmax(mx, fabs(x[b * vstride + i]));
        md = fmax(md, fabs(d[b * vstride + i]));
    }
    __shared__ double sx[256], sd[256];
    sx[threadIdx.x] = mx;
    sd[threadIdx.x] = md;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            sx[threadIdx.x] = fmax(sx[threadIdx.x], sx[threadIdx.x + h]);
            sd[threadIdx.x] = fmax(sd[threadIdx.x], sd[threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double pm = step == 0 ? sx[0] : prev[b];
        if (sd[0] * sd[0] <= tol * tol * sx[0] * pm)
            refining[b] = 0;  // converged: leaves the refining mask (live.active == refining)
        else if (last)
            live.status[b] = fail_code;
        else
            prev[b] = sd[0];
    }
}

void launch_refine_check(const double* x, const double* d, int64_t vstride, int np, double tol,
                         int fail_code, int step, bool last, double* prev, int* refining,
                         const int* status, int nchains, hipStream_t s) {
    APM_LAUNCH(k_refine_check, dim3(nchains), dim3(256), 0, s, x, d, vstride, np, tol,
                       fail_code, step, (int)last, prev, refining,
                       Live{refining, const_cast<int*>(status)});
}

__global__ void k_refine_mask(Live live, int* refining, int nchains) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nchains) refining[b] = live32(live, b) ? 1 : 0;
}

void launch_refine_mask(Live live, int* refining, int nchains, hipStream_t s) {
    APM_LAUNCH(k_refine_mask, dim3((nchains + 255) / 256), dim3(256), 0, s, live,
                       refining, nchains);
}

void launch_refine(int mode, const double* Ws, const double* Kb, double* x, const double* Kt,
                   double* out, int64_t vstride, int np, Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_refine, dim3((np + 255) / 256, nchains), dim3(256), 0, s, mode, Ws, Kb,
                       x, Kt, out, vstride, np, live);
}
