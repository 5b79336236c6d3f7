// Gradient of the Laplace log marginal likelihood with respect to theta: the
// kernels around the two Schur-complement passes that host_laplace.cpp's grad_block borrows from the
// Cholesky (chol_solve_rows on the bottom rows of the work matrix against the last Newton factor).
//
//   v = phi(f)/Phi(y f),  g = y v,  d3 = -[(2v + y f)(-f v - y v^2) + y v]      (f = K a, the mode)
//   (the probit; the logit: g = y sigma(-y f), d3 = -y W (1 - 2 sigma(y f)) - lik_grad_d3)
//   dS_i = K_ii - |L^-1 (W^1/2 . K[:, i])|^2,  s2 = 1/2 dS . d3
//   R = Z^T Z with Z = L^-1 diag(W^1/2),  q = s2 - R (K s2)
//   M = 1/2 a a^T - 1/2 R + 1/2 (q g^T + g q^T)
//   dLML/dtheta_j = sum_ik M_ik (dK/dtheta_j)_ik
//   dK/dtheta_0 = S (K without its jitter: s on the diagonal, not s + epsilon),
//   dK/dtheta_{k+1} = G_ik ((x_ik - x_jk)/tau_k)^2 (ARD), the sum over k of these (iso); G = S for
//   the SE family, cov_G (apm_internal.h) for Matern 3/2 and 5/2
//   dK/dtheta_{P-1} = beta on every data pair (a biased kind, K = S + beta 1 1^T + epsilon I)
//   dK/dtheta_{P-1} = lambda x_i . x_k on every data pair (a kind with the linear term, DESIGN.md
//   §25; beta's entry is then P - 2)
// with W, L, a of the last Newton iteration (latent_posterior_approximations.py:81-106).
#include "apm_internal.h"
#include "pair_tile.h"

// nothing moves across: neither the compiler's passes (memory clobber) nor the machine scheduler
#define APM_WALL()                           \
    do {                                     \
        asm volatile("" ::: "memory");       \
        __builtin_amdgcn_sched_barrier(0);   \
    } while (0)

// One wave per (chain, training row r): dS_r from the squared norm of row np + r of the work
// matrix over its first 64 nb columns (the row of (K W^1/2) L^-T; row_sqnorm_d2) and K's own
// diagonal entry, then g_r and s2_r at the mode. Rows >= n get exact zeros.
template <int LIK>
__global__ __launch_bounds__(256) void k_grad_rows(MatB A, MatB K, int n, int nb,
                                                   const double* __restrict__ f,
                                                   const double* __restrict__ y, int64_t vstride,
                                                   double* __restrict__ dS, double* __restrict__ g,
                                                   double* __restrict__ s2, int64_t gstride,
                                                   Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int np = 64 * nb;
    if (r >= np) return;
    const int64_t o = b * gstride + r;
    if (r >= n) {  // (wave-uniform)
        if (lane == 0) dS[o] = g[o] = s2[o] = 0.0;
        return;
    }
    const double s = row_sqnorm_d2(A.base + b * A.cstride + (int64_t)(np + r) * A.ld, np, lane);
    if (lane != 0) return;
    const double ds = K.base[b * K.cstride + (int64_t)r * K.ld + r] - s;
    const double fi = f[b * vstride + r], yi = y[r];
    const LikGD3 l = lik_grad_d3<LIK>(fi, yi);
    dS[o] = ds;
    g[o] = l.grad;
    s2[o] = 0.5 * ds * l.d3;
}

void launch_grad_rows(int lik, MatB A, MatB K, int n, int nb, const double* f, const double* y,
                      int64_t vstride, double* dS, double* g, double* s2, int64_t gstride,
                      Live live, int nchains, hipStream_t s) {
    APM_LIK_DISPATCH(lik, APM_LAUNCH(k_grad_rows<LIK>, dim3((64 * nb + 3) / 4, nchains), dim3(256),
                                     0, s, A, K, n, nb, f, y, vstride, dS, g, s2, gstride, live));
}

// Right-hand side of the second pass: rows [np, 2np) x columns [0, np) of the work matrix
// <- diag(W^1/2) (whole tiles, zero off the diagonal; W^1/2 is zero beyond the data), and zeros
// in the lower tiles of the bottom-right block, which the trailing updates then turn into -Z^T Z.
__global__ __launch_bounds__(256) void k_grad_fill(MatB A, const double* __restrict__ Ws,
                                                   int64_t vstride, int nb, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int t = blockIdx.x, nbl = nb * nb;
    int ti, tj;
    int64_t c0 = 0;
    if (t < nbl) {
        ti = t / nb;
        tj = t % nb;
    } else {  // lower-triangular tile index -> (ti, tj) of the bottom-right block
        lower_tri_index(t - nbl, ti, tj);
        c0 = (int64_t)nb * 64;
    }
    const bool dg = t < nbl && ti == tj;
    const double* wb = Ws + b * vstride + ti * 64;
    double* At = A.base + b * A.cstride + ((int64_t)nb * 64 + ti * 64) * A.ld + c0 + tj * 64;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        const int e = threadIdx.x + 256 * h;  // piece: row e / 32, columns 2 (e % 32) .. +1
        const int r = e >> 5, c = 2 * (e & 31);
        d2_t v{0.0, 0.0};
        if (dg && (r >> 1) == (c >> 1)) {
            if (r == c) v.x = wb[r];
            else v.y = wb[r];
        }
        *reinterpret_cast<d2_t*>(At + (int64_t)r * A.ld + c) = v;
    }
}

void launch_grad_fill(MatB A, const double* Ws, int64_t vstride, int nb, Live live, int nchains,
                      hipStream_t s) {
    APM_LAUNCH(k_grad_fill, dim3(nb * nb + nb * (nb + 1) / 2, nchains), dim3(256), 0, s, A, Ws,
               vstride, nb, live);
}

// q = s2 - R t with u = (-R) t from the symmetric product over the bottom-right block's lower
// tiles (launch_symv); exact zeros beyond the data
__global__ __launch_bounds__(256) void k_grad_q(const double* __restrict__ s2,
                                                const double* __restrict__ u,
                                                double* __restrict__ q, int64_t gstride, int n,
                                                int np, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const int64_t o = b * gstride + i;
    q[o] = i < n ? s2[o] + u[o] : 0.0;
}

void launch_grad_q(const double* s2, const double* u, double* q, int64_t gstride, int n, int np,
                   Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_grad_q, dim3((np + 255) / 256, nchains), dim3(256), 0, s, s2, u, q, gstride, n,
               np, live);
}

// The contraction sum_ik M_ik (dK/dtheta_j)_ik for every j in one pass over the inputs: k_gram's
// tiling - one workgroup of 4 waves per lower 128x128 super-tile (si, sj) and chain, wave w the
// 64x64 tile (2si + w/2, 2sj + w%2) (the upper tile of a diagonal super-tile and tiles beyond the
// padded size are skipped), 8x8 pairs per lane, the staging and the operand load of pair_tile.h.
// Per pair the lane first forms w = c M_ik S_ik once: M from Rn (the
// bottom-right block of the work matrix, -R in its lower tiles), a, q and g; S from K off the
// diagonal and s = exp(theta_0) on it (no epsilon); c the count of the symmetric sum - 2 for
// i > k, 1 on the diagonal, 0 for the upper half of a diagonal tile and for any row or column
// beyond the data (K is identity-padded there: masked, not multiplied). Then theta_0's sum is
// sum w, and feature k's is sum w df_k^2: each lane its 8 rows (8 pairs each, in order) and the 8
// row sums in order, the wave's butterfly, the 4 waves in order. ARD writes one partial per
// feature; iso adds the features in order into one. Partials go to part[b][t][0..P) for
// super-tile t; k_grad_sum adds them in tile order. No atomics, no hand-over between workgroups:
// every output depends on its own chain and on fixed positions only.
//
// FAM (APM_FAM_*): for the SE family the one weight w serves theta_0 and the length scales
// (G = S). For a Matern family the length scales need c M G, and G needs the pair's complete r^2
// before the per-feature sums start; a second 8x8 block of registers is not available (242
// VGPRs), so the kernel makes two passes over the staged feature chunks: the first accumulates
// r^2 into w (pair_r2_chunk, k in order), the K / R / vector stage adds c M S into theta_0's sum
// and overwrites w with c M G (cov_G of the lane's own r^2), the second is the SE pass. Every
// sum keeps the order above. ard: theta[1 + k] scales feature k, else theta[1] every feature.
//
// BIAS (the constant term): K's lower tiles hold S + beta. The SE instantiation
// takes the two-pass route and forms S = G from the lane's own r^2 (K is not read at all); the
// Matern ones, which have no registers left for a second exp chain beside w, take theta_0's
// weight as K - beta, which loses up to u (S + beta) per pair (§22 bounds what that does to the
// sum). One more sum per super-tile, beta sum c M_ik over the data pairs (dK/dtheta_{P-1} = beta
// on every pair, the diagonal included): the pairs in the order the stage visits them (SE: a
// row's 8 pairs, then the 8 row sums; Matern: one running sum over the two runs' rows), the
// wave's butterfly, the 4 waves in order; it is entry P - 1 of the partials.
//
// LIN (the linear term, DESIGN.md §25, SE only): K's lower tiles hold S [+ beta] + lambda x x^T,
// so the instantiation takes the biased SE route, S from the lane's own r^2 with K not read, which
// keeps theta_0's weight exact; beta's entry moves to P - 2. lambda's own entry P - 1 is not
// written here: k_grad_lin below does.
template <int FAM, bool BIAS, bool LIN>
__global__ __launch_bounds__(256, FAM == APM_FAM_SE ? 1 : 2) void k_grad_reduce(
    MatB K, MatB Rn, const double* __restrict__ X, int64_t ldx, int n, int d, int nb,
    const double* __restrict__ theta, int64_t tstride, int ard, const double* __restrict__ avec,
    int64_t vstride, const double* __restrict__ qvec, const double* __restrict__ gvec,
    int64_t gstride, double* __restrict__ part, int64_t pstride, int P, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int t = blockIdx.x;
    int si, sj;  // the lower super-tile, si >= sj
    lower_tri_index(t, si, sj);

    __shared__ PairTile lds;
    __shared__ double red[4][GK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tr = lane >> 3, tc = lane & 7;
    const int ti = 2 * si + (wv >> 1), tj = 2 * sj + (wv & 1);
    const bool mine = ti < nb && tj <= ti;  // (wave-uniform)
    const int ro = 64 * (wv >> 1), co = 64 * (wv & 1);
    const double* th = theta + b * tstride;
    double* pb = part + b * pstride + (int64_t)t * P;

    double w[8][8];
    double s0 = 0.0, sb = 0.0;
    if constexpr (FAM != APM_FAM_SE || BIAS || LIN) {  // first pass: w <- the pairs' r^2
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = 0; q < 8; ++q) w[p][q] = 0.0;
        for (int k0 = 0; k0 < d; k0 += GK) {
            const int kc = min(GK, d - k0);
            pair_stage(lds, th, ard, k0, kc, X, ldx, n, si * 128, X, ldx, n, sj * 128);
            if (mine) pair_r2_chunk(lds, kc, ro, tr, co, tc, w);
        }
    }
    if (mine) {
        const double sigma = exp(th[0]);
        const double* ab = avec + b * vstride;
        const double* qb = qvec + b * gstride;
        const double* gb = gvec + b * gstride;
        if constexpr ((BIAS || LIN) && FAM == APM_FAM_SE) {
            // the stage below without K: S = G from the lane's own r^2, and beta's sum beside
            // theta_0's (a row's 8 pairs in order, then the 8 row sums in order)
            double ak[8], qk[8], gk[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int gj = tj * 64 + R8(tc, q);
                ak[q] = ab[gj];
                qk[q] = qb[gj];
                gk[q] = gb[gj];
            }
            const double* Rt = Rn.base + b * Rn.cstride + tj * 64 + 4 * tc;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int gi = ti * 64 + R8(tr, p);
                const double* rr = Rt + (int64_t)gi * Rn.ld;
                const d2_t r0 = *reinterpret_cast<const d2_t*>(rr);
                const d2_t r1 = *reinterpret_cast<const d2_t*>(rr + 2);
                const d2_t r2 = *reinterpret_cast<const d2_t*>(rr + 32);
                const d2_t r3 = *reinterpret_cast<const d2_t*>(rr + 34);
                const double rv[8] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
                const double ai = ab[gi], qi = qb[gi], gg = gb[gi];
                double sp = 0.0, spb = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int gj = tj * 64 + R8(tc, q);
                    const double m = 0.5 * (fma(ai, ak[q], rv[q]) + fma(qi, gk[q], gg * qk[q]));
                    const double sv = (gi == gj) ? sigma : cov_S<FAM>(sigma, w[p][q]);
                    const double cnt = (gi > gj) ? 2.0 : 1.0;
                    const bool in = gi < n && gj <= gi;  // (gj <= gi < n)
                    w[p][q] = in ? cnt * (m * sv) : 0.0;
                    sp += w[p][q];
                    if constexpr (BIAS) spb += in ? cnt * m : 0.0;
                }
                s0 += sp;
                if constexpr (BIAS) sb += spb;
            }
        } else if constexpr (FAM == APM_FAM_SE) {
            double ak[8], qk[8], gk[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int gj = tj * 64 + R8(tc, q);
                ak[q] = ab[gj];
                qk[q] = qb[gj];
                gk[q] = gb[gj];
            }
            const double* Kt = K.base + b * K.cstride + tj * 64 + 4 * tc;
            const double* Rt = Rn.base + b * Rn.cstride + tj * 64 + 4 * tc;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int gi = ti * 64 + R8(tr, p);
                const double* kr = Kt + (int64_t)gi * K.ld;
                const double* rr = Rt + (int64_t)gi * Rn.ld;
                const d2_t k0 = *reinterpret_cast<const d2_t*>(kr);
                const d2_t k1 = *reinterpret_cast<const d2_t*>(kr + 2);
                const d2_t k2 = *reinterpret_cast<const d2_t*>(kr + 32);
                const d2_t k3 = *reinterpret_cast<const d2_t*>(kr + 34);
                const d2_t r0 = *reinterpret_cast<const d2_t*>(rr);
                const d2_t r1 = *reinterpret_cast<const d2_t*>(rr + 2);
                const d2_t r2 = *reinterpret_cast<const d2_t*>(rr + 32);
                const d2_t r3 = *reinterpret_cast<const d2_t*>(rr + 34);
                const double kv[8] = {k0.x, k0.y, k1.x, k1.y, k2.x, k2.y, k3.x, k3.y};
                const double rv[8] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
                const double ai = ab[gi], qi = qb[gi], gg = gb[gi];
                double sp = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int gj = tj * 64 + R8(tc, q);
                    const double m = 0.5 * (fma(ai, ak[q], rv[q]) + fma(qi, gk[q], gg * qk[q]));
                    const double sv = (gi == gj) ? sigma : kv[q];
                    const double cnt = (gi > gj) ? 2.0 : 1.0;
                    const bool in = gi < n && gj <= gi;  // (gj <= gi < n)
                    w[p][q] = in ? cnt * (m * sv) : 0.0;
                    sp += w[p][q];
                }
                s0 += sp;
            }
        } else {
            // w <- G of the pair's r^2 while nothing else is live (a few sqrt / exp chains in
            // flight, not 64: their temporaries must fit beside w)
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int q = 4 * h; q < 4 * h + 4; ++q) w[p][q] = cov_G<FAM>(sigma, w[p][q]);
                    APM_WALL();
                }
            // The SE stage above gives birth to w row by row; here all 64 are live throughout, so
            // the stage runs over the tile's two runs of 4 columns in turn (half the column
            // operands and half a row of K and R at a time). theta_0 takes c M S, the length
            // scales c M G. A row's 8 pairs are still added in order (sp[p] carries the row's
            // sum from the first run into the second), then the 8 row sums in order: the SE
            // stage's order. The lane's coordinates are redefined (to themselves) before each
            // run, so that a run's addresses, masks and row operands are formed when it needs
            // them and not held from the loops above or for the next run; with the walls this
            // keeps the instantiation at 248 VGPRs without spills (the compiler otherwise hoists
            // and shares them and spills up to 114 registers).
            int trs = tr, tcs = tc;
            double beta = 0.0;
            if constexpr (BIAS) beta = exp(th[P - 1 - (LIN ? 1 : 0)]);
            const double* Kt = K.base + b * K.cstride + tj * 64;
            const double* Rt = Rn.base + b * Rn.cstride + tj * 64;
            double sp[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) sp[p] = 0.0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                asm volatile("" : "+v"(trs), "+v"(tcs));  // (per run: nothing kept for the next)
                double ak[4], qk[4], gk[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int gj = tj * 64 + R8(tcs, 4 * h + q);
                    ak[q] = ab[gj];
                    qk[q] = qb[gj];
                    gk[q] = gb[gj];
                }
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int gi = ti * 64 + R8(trs, p);
                    const double* kr = Kt + (int64_t)gi * K.ld + 4 * tcs + 32 * h;
                    const double* rr = Rt + (int64_t)gi * Rn.ld + 4 * tcs + 32 * h;
                    const d2_t k0 = *reinterpret_cast<const d2_t*>(kr);
                    const d2_t k1 = *reinterpret_cast<const d2_t*>(kr + 2);
                    const d2_t r0 = *reinterpret_cast<const d2_t*>(rr);
                    const d2_t r1 = *reinterpret_cast<const d2_t*>(rr + 2);
                    const double kv[4] = {k0.x, k0.y, k1.x, k1.y};
                    const double rv[4] = {r0.x, r0.y, r1.x, r1.y};
                    const double ai = ab[gi], qi = qb[gi], gg = gb[gi];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int gj = tj * 64 + R8(tcs, 4 * h + q);
                        const double m = 0.5 * (fma(ai, ak[q], rv[q]) + fma(qi, gk[q], gg * qk[q]));
                        double sv = (gi == gj) ? sigma : kv[q];
                        if constexpr (BIAS) sv = (gi == gj) ? sigma : kv[q] - beta;
                        const double cnt = (gi > gj) ? 2.0 : 1.0;
                        const bool in = gi < n && gj <= gi;  // (gj <= gi < n)
                        sp[p] += in ? cnt * (m * sv) : 0.0;
                        if constexpr (BIAS) sb += in ? cnt * m : 0.0;
                        w[p][4 * h + q] = in ? cnt * (m * w[p][4 * h + q]) : 0.0;
                    }
                    // (the next rows' loads are not to be hoisted over this row: no room)
                    APM_WALL();
                }
            }
#pragma unroll
            for (int p = 0; p < 8; ++p) s0 += sp[p];
        }
    } else if constexpr (FAM == APM_FAM_SE && !BIAS && !LIN) {  // (a two-pass w is zero already)
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = 0; q < 8; ++q) w[p][q] = 0.0;
    }
    s0 = wave_sum_d(s0);
    if constexpr (BIAS) sb = wave_sum_d(sb);

    double iso = 0.0;  // (thread 0: the features' sums in order)
    for (int k0 = 0; k0 < d; k0 += GK) {
        const int kc = min(GK, d - k0);
        pair_stage(lds, th, ard, k0, kc, X, ldx, n, si * 128, X, ldx, n, sj * 128);
        for (int k = 0; k < kc; ++k) {
            double sk = 0.0;
            if (mine) {
                double a[8], c[8];
                pair_operands(lds, k, ro, tr, co, tc, a, c);
                double sp[8];  // one chain of 8 fmas per row: 8 independent chains in flight
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    double df[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) df[q] = a[p] - c[q];  // pre-scaled by 1/tau_k
#pragma unroll
                    for (int q = 0; q < 8; ++q) df[q] *= df[q];
                    sp[p] = 0.0;
#pragma unroll
                    for (int q = 0; q < 8; ++q) sp[p] = fma(w[p][q], df[q], sp[p]);
                }
#pragma unroll
                for (int p = 0; p < 8; ++p) sk += sp[p];
                sk = wave_sum_d(sk);
            }
            if (lane == 0) red[wv][k] = sk;
        }
        __syncthreads();
        if (ard != 0) {
            if (tid < kc) pb[1 + k0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        } else if (tid == 0) {
            for (int k = 0; k < kc; ++k) iso += ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        }
    }
    __syncthreads();
    if (lane == 0) {
        red[wv][0] = s0;
        if constexpr (BIAS) red[wv][1] = sb;
    }
    __syncthreads();
    if (tid == 0) {
        pb[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        if (ard == 0) pb[1] = iso;
        if constexpr (BIAS)
            pb[P - 1 - (LIN ? 1 : 0)] = exp(th[P - 1 - (LIN ? 1 : 0)]) *
                                        (((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]);
    }
}

// lambda's entry of the gradient (the linear term): part[b][t][P - 1] <-
// lambda sum c M_ik (x_i . x_k) over the data pairs of lower super-tile t, a kernel of its own
// beside k_grad_reduce with its tiling, its M and its order of sums. The first sweep stages the
// unscaled inputs (pair_stage<true>) and accumulates the pairs' dot products in the lane's 8x8
// block, features in order; the stage then streams the lower tiles of Rn once more and forms M as
// k_grad_reduce does (K is not read): a row's 8 pairs in order, the 8 row sums in order, the
// wave's butterfly, the 4 waves in order; k_grad_sum adds the super-tiles in order. Nothing of
// k_grad_reduce's 64 live weights has to make room for the 64 dot products this way, and its
// non-linear instantiations stay what they were.
__global__ __launch_bounds__(256, 2) void k_grad_lin(
    MatB Rn, const double* __restrict__ X, int64_t ldx, int n, int d, int nb,
    const double* __restrict__ theta, int64_t tstride, const double* __restrict__ avec,
    int64_t vstride, const double* __restrict__ qvec, const double* __restrict__ gvec,
    int64_t gstride, double* __restrict__ part, int64_t pstride, int P, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int t = blockIdx.x;
    int si, sj;  // the lower super-tile, si >= sj
    lower_tri_index(t, si, sj);

    __shared__ PairTile lds;
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tr = lane >> 3, tc = lane & 7;
    const int ti = 2 * si + (wv >> 1), tj = 2 * sj + (wv & 1);
    const bool mine = ti < nb && tj <= ti;  // (wave-uniform)
    const int ro = 64 * (wv >> 1), co = 64 * (wv & 1);
    const double* th = theta + b * tstride;

    double w[8][8];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) w[p][q] = 0.0;
    for (int k0 = 0; k0 < d; k0 += GK) {
        const int kc = min(GK, d - k0);
        pair_stage<true>(lds, th, 0, k0, kc, X, ldx, n, si * 128, X, ldx, n, sj * 128);
        if (mine) pair_dot_chunk(lds, kc, ro, tr, co, tc, w);
    }
    double sl = 0.0;
    if (mine) {
        const double* ab = avec + b * vstride;
        const double* qb = qvec + b * gstride;
        const double* gb = gvec + b * gstride;
        double ak[8], qk[8], gk[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int gj = tj * 64 + R8(tc, q);
            ak[q] = ab[gj];
            qk[q] = qb[gj];
            gk[q] = gb[gj];
        }
        const double* Rt = Rn.base + b * Rn.cstride + tj * 64 + 4 * tc;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int gi = ti * 64 + R8(tr, p);
            const double* rr = Rt + (int64_t)gi * Rn.ld;
            const d2_t r0 = *reinterpret_cast<const d2_t*>(rr);
            const d2_t r1 = *reinterpret_cast<const d2_t*>(rr + 2);
            const d2_t r2 = *reinterpret_cast<const d2_t*>(rr + 32);
            const d2_t r3 = *reinterpret_cast<const d2_t*>(rr + 34);
            const double rv[8] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
            const double ai = ab[gi], qi = qb[gi], gg = gb[gi];
            double sp = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int gj = tj * 64 + R8(tc, q);
                const double m = 0.5 * (fma(ai, ak[q], rv[q]) + fma(qi, gk[q], gg * qk[q]));
                const double cnt = (gi > gj) ? 2.0 : 1.0;
                const bool in = gi < n && gj <= gi;  // (gj <= gi < n)
                sp += in ? cnt * (m * w[p][q]) : 0.0;
            }
            sl += sp;
        }
    }
    sl = wave_sum_d(sl);
    if (lane == 0) red[wv] = sl;
    __syncthreads();
    if (tid == 0)
        part[b * pstride + (int64_t)t * P + P - 1] =
            exp(th[P - 1]) * (((red[0] + red[1]) + red[2]) + red[3]);
}

void launch_grad_reduce(MatB K, MatB Rn, const double* X, int64_t ldx, int n, int d, int nb,
                        const double* theta, int64_t tstride, int kind, const double* a,
                        int64_t vstride, const double* q, const double* g, int64_t gstride,
                        double* part, int64_t pstride, int P, Live live, int nchains,
                        hipStream_t s) {
    const int ns = (nb + 1) / 2;
    const KernelKind kk = kernel_kind_of(kind);
    APM_FAMILY_DISPATCH(
        kk.family,
        APM_BIAS_DISPATCH(
            kk.bias,
            APM_LINEAR_DISPATCH(kk.linear, APM_LAUNCH((k_grad_reduce<FAM, BIAS, LIN>),
                                                      dim3(ns * (ns + 1) / 2, nchains), dim3(256),
                                                      0, s, K, Rn, X, ldx, n, d, nb, theta, tstride,
                                                      kk.iso ? 0 : 1, a, vstride, q, g, gstride,
                                                      part, pstride, P, live))));
    if (kk.linear)
        APM_LAUNCH(k_grad_lin, dim3(ns * (ns + 1) / 2, nchains), dim3(256), 0, s, Rn, X, ldx, n, d,
                   nb, theta, tstride, a, vstride, q, g, gstride, part, pstride, P, live);
}

// grad[b][p] = the nst super-tile partials of (chain b, parameter p) added in tile order
__global__ __launch_bounds__(256) void k_grad_sum(const double* __restrict__ part,
                                                  int64_t pstride, int nst, int P,
                                                  double* __restrict__ grad, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double* pb = part + b * pstride + p;
    double s = 0.0;
    for (int t = 0; t < nst; ++t) s += pb[(int64_t)t * P];
    grad[(int64_t)b * P + p] = s;
}

void launch_grad_sum(const double* part, int64_t pstride, int nst, int P, double* grad, Live live,
                     int nchains, hipStream_t s) {
    APM_LAUNCH(k_grad_sum, dim3((P + 255) / 256, nchains), dim3(256), 0, s, part, pstride, nst, P,
               grad, live);
}
