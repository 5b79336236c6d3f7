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
// Kernels, here: K b with the fp32 Newton matrix formed in the same pass, blocked forward /
// backward TRSV with fp32 tiles and fp64 vectors, and the refinement vector ops. The
// factorisation itself: fp32 copies of the diag / panel / trailing-update steps of chol.hip on
// the same tile lists (f32 MFMA v_mfma_f32_16x16x4_f32: twice the fp64 MFMA rate, half the bytes;
// fp16x3 operands where their range allows), in chol32_panel.hip and chol32_update.hip.
#include "apm_internal.h"
#include "tile32.h"

// ------------------------------------------------------------------------------- B in fp32
// (formed by k_symv_part in the same pass as K b, below)

// out[b][:] = row `row` of Bf (fp32 -> fp64)
__global__ __launch_bounds__(256) void k_row32(MatF Bf, int64_t row, int np, double* out,
                                               int64_t ostride, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
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
template <int TPW>
__global__ __launch_bounds__(256) void k_symv_part(MatB K, const double* __restrict__ x,
                                                   int64_t xstride, double* __restrict__ part,
                                                   int64_t pstride, int nb, MatF Bf,
                                                   const double* __restrict__ Ws, int64_t wstride,
                                                   Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int ntile = nb * (nb + 1) / 2;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rg = tid >> 4, cg = tid & 15;  // rows 4rg .. 4rg+3, columns 4cg .. 4cg+3
    __shared__ double cs[4][64];
    auto load = [&](int t, d2_t (&v)[4][2]) {
        int ti, tj;
        lower_tri_index(t, ti, tj);
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
        lower_tri_index(t, ti, tj);
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
    if (!live_chain(live, b)) return;
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
    if (!live_chain(live, b)) return;
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
    if (!live_chain(live, b)) return;
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
    if (!live_chain(live, b)) return;
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
    if (!live_chain(live, b)) return;
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
    if (!live_chain(live, b)) return;
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
    if (!live_chain(live, b)) return;
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
    if (b < nchains) refining[b] = live_chain(live, b) ? 1 : 0;
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
