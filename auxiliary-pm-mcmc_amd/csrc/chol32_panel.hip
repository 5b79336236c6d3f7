// The in-panel steps of the fp32 factorisations: the dataflow walk of an outer panel's columns
// (k_chol_panel_df32) and the explicit-inverse panel (k_zinv_level32, k_panel_inv_gemm32).
#include "apm_internal.h"
#include "diag.h"
#include "tile32.h"

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
        const long rows = R - row0, item = xcd_remap((long)blockIdx.x, rows * nchains);
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
    if (!live_chain(live, b)) {
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
                const bool ok = diag_compute<true, float>(sm.d, lane);
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
                        for (int r = 0; r < 4; ++r)
                            plane_put(hp + (16 * bi + F32_CROW(lane, r)) * 32 + 16 * bj + (lane & 15),
                                      pl.lo, x[bi][bj][r]);
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
    if (!live_chain(live, b) || (h3ok && !h3ok[b])) return;
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
                plane_put(Zp, zpl, 64 * t + r, 64 * t + c, v);
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
                    plane_put(Zp, zpl, zr, zc, v);
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
    const long w = xcd_remap((long)blockIdx.x, (long)npair * nchains);
    const int b = (int)(w / npair), i0 = Kend + 2 * (int)(w % npair);
    const bool two = i0 + 1 < nb;  // (an odd count leaves the last workgroup one row tile)
    if (!live_chain(live, b) || (h3ok && !h3ok[b])) return;
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
        h8_t hi, lo;
        split_h3(ra0, ra1, hi, lo);
        *reinterpret_cast<h8_t*>(&sm.a[buf][0][arow][HS(arow, acol)]) = hi;
        *reinterpret_cast<h8_t*>(&sm.a[buf][1][arow][HS(arow, acol)]) = lo;
    };
    // Z staging by LDS-DMA: rows [64 kb, 512) of slice s (the column tiles that need it); wave
    // wv takes plane wv & 1 and the 16-row groups g = (wv >> 1) + 4t (lane mapping:
    // plane_lane_off)
    const int pln = wv & 1;
    const unsigned short* zg = zpl.base + b * zpl.cstride + (pln ? zpl.lo : 0) +
                               plane_lane_off(lane);
    auto dma = [&](int sidx, int buf) {
        const int kb = sidx >> 1;
        for (int g = 4 * kb + (wv >> 1); g < 32; g += 4)
            __builtin_amdgcn_global_load_lds(
                (glb_void_t*)(zg + ((int64_t)sidx * zpl.rows + 16 * g) * 32),
                (lds_void_t*)&sm.z[buf][pln][16 * g][0], 16, 0, 0);
    };
    auto mm = [&](f4_t (&acc)[4][4], int cc, int cur) {
        h3_mma<4>(acc, sm.a[cur][0], sm.a[cur][1], sm.z[cur][0], sm.z[cur][1], 64 * rt, 64 * cc,
                  r16, kq);
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
                    h8_t hi, lo;
                    split_h3(v0, v1, hi, lo);
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
