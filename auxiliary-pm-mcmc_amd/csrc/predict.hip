// Laplace predictive distribution at test inputs: the two kernels around the
// panel solves that host_laplace.cpp's predict_block borrows from the Cholesky (chol_solve_rows on the test
// rows only).
//
//   k*_c = s exp(-1/2 sum_k ((x*_k - x_ck)/tau_k)^2)   no epsilon: kernels.pyx adds it to the
//                                                       i == j entries of ONE point set only
//   mu*  = k*^T a,   v = L^-1 (W^1/2 . k*),   var* = s - v^T v   (prior variance k** = s)
//   (a biased kind, DESIGN.md §22: k*_c + beta and k** = s + beta)
//   pi*  = Phi(mu* / sqrt(1 + var*))
// with W, L, a of the last Newton iteration (latent_posterior_approximations.py:81-112).
#include "apm_internal.h"
#include "gh_table.h"
#include "pair_tile.h"

// Rectangular twin of k_gram: one workgroup of 4 waves per 128x128 super-tile (si over the test
// rows, sj over the training columns), wave w the 64x64 tile (2si + w/2, 2sj + w%2), 8x8 pairs per
// lane, the staging and the distance loop of pair_tile.h. s = exp(theta_0) comes from the host
// (sig[b], libm's exp, the same value in k* and in the prior variance k** of k_predict_reduce), so
// an uninformed test
// point returns bitwise the caller's exp(theta_0); K's own s is the device's exp and may differ
// from it in the last bit. Every (row, column) value depends on its own pair of points only, and
// the partial sums of mu* on the column position only: a chain's outputs do not depend on its
// batch nor a test point's on its block.
// FAM (APM_FAM_*) selects the epilogue (cov_S), ard the length scales, as in k_gram.
// BIAS: the constant term beta = bet[b] (the host's exp, as s is) is added to every k* of a test
// row r < ms and a training column c < n; the prior variance sig[b] that k_predict_reduce and
// k_is_rows read is then s + beta.
// LIN: the linear term: lambda = lam[b] (the host's exp, as s and beta are) times
// the dot product of the raw inputs is added to every k* of a test row r < ms and a training
// column c < n as k_gram does it: a sweep of its own sums the dot products (pair_dot_chunk), they
// are parked in the lane's own entries of the output, which it overwrites below, and the epilogue
// takes fma(lambda, x*_r . x_c, cov_S [+ beta]). The prior variance then differs by test row,
// k** = sig[b] + lam[b] |x*_r|^2 (k_predict_reduce, k_is_rows).
template <int FAM, bool BIAS, bool LIN>
__global__ __launch_bounds__(256, 2) void k_gram_cross(
    MatB out, int64_t row0, const double* __restrict__ Xs, int ms, int mb,
    const double* __restrict__ X, int64_t ldx, int n, int d, int nb,
    const double* __restrict__ theta, int64_t tstride, const double* __restrict__ sig,
    const double* __restrict__ bet, const double* __restrict__ lamv, int ard,
    const double* __restrict__ Ws, const double* __restrict__ avec, int64_t vstride,
    double* __restrict__ part, int64_t pstride, Live live, int plain) {
    const int b = blockIdx.y;
    if (live.active && !live_chain(live, b)) return;
    const int nsc = (nb + 1) / 2;
    const int si = blockIdx.x / nsc, sj = blockIdx.x % nsc;

    __shared__ PairTile lds;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tr = lane >> 3, tc = lane & 7;
    const int ti = 2 * si + (wv >> 1), tj = 2 * sj + (wv & 1);
    const bool mine = ti < mb && tj < nb;  // (wave-uniform)
    const int ro = 64 * (wv >> 1), co = 64 * (wv & 1);
    const double* th = theta + b * tstride;
    const double sigma = sig[b];
    double beta = 0.0;
    if constexpr (BIAS) beta = bet[b];
    double lam = 0.0;
    if constexpr (LIN) lam = lamv[b];

    double acc[8][8];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[p][q] = 0.0;

    if constexpr (LIN) {
        for (int k0 = 0; k0 < d; k0 += GK) {
            const int kc = min(GK, d - k0);
            pair_stage<true>(lds, th, ard, k0, kc, Xs, d, ms, si * 128, X, ldx, n, sj * 128);
            if (mine) pair_dot_chunk(lds, kc, ro, tr, co, tc, acc);
        }
        if (mine) {  // park the dot products where this lane's own results go
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                if (plain) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int gi = ti * 64 + R8(tr, p), gj = tj * 64 + R8(tc, q);
                        if (gi < ms && gj < n) out.base[(int64_t)gi * out.ld + gj] = acc[p][q];
                    }
                } else {
                    pair_store_row(out.base + b * out.cstride +
                                       (row0 + ti * 64 + R8(tr, p)) * out.ld + tj * 64 + 4 * tc,
                                   acc[p]);
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[p][q] = 0.0;
            }
        }
    }
    for (int k0 = 0; k0 < d; k0 += GK) {
        const int kc = min(GK, d - k0);
        pair_stage(lds, th, ard, k0, kc, Xs, d, ms, si * 128, X, ldx, n, sj * 128);
        if (mine) pair_r2_chunk(lds, kc, ro, tr, co, tc, acc);
    }
    if (!mine) return;  // (after the last barrier)

#pragma unroll
    for (int p = 0; p < 8; ++p) {
        double dt[8];  // (LIN: the row's parked dot products)
        if constexpr (LIN) {
            if (plain) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int gi = ti * 64 + R8(tr, p), gj = tj * 64 + R8(tc, q);
                    dt[q] = (gi < ms && gj < n) ? out.base[(int64_t)gi * out.ld + gj] : 0.0;
                }
            } else {
                pair_load_row(out.base + b * out.cstride +
                                  (row0 + ti * 64 + R8(tr, p)) * out.ld + tj * 64 + 4 * tc,
                              dt);
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int gi = ti * 64 + R8(tr, p), gj = tj * 64 + R8(tc, q);
            if constexpr (LIN)
                acc[p][q] = (gi < ms && gj < n)
                                ? fma(lam, dt[q], cov_S<FAM>(sigma, acc[p][q]) + beta)
                                : 0.0;
            else if constexpr (BIAS)
                acc[p][q] = (gi < ms && gj < n) ? cov_S<FAM>(sigma, acc[p][q]) + beta : 0.0;
            else
                acc[p][q] = (gi < ms && gj < n) ? cov_S<FAM>(sigma, acc[p][q]) : 0.0;
        }
    }

    if (plain) {  // apm_gram_cross: k* itself into an ms x n buffer (any ld: scalar stores)
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int gi = ti * 64 + R8(tr, p), gj = tj * 64 + R8(tc, q);
                if (gi < ms && gj < n) out.base[(int64_t)gi * out.ld + gj] = acc[p][q];
            }
        return;
    }

    // mu* partial of this tile: each lane its 8 columns in order, then the row's 8 lanes in a
    // fixed butterfly; the tile columns are summed in order by k_predict_reduce. Then W^1/2 . k*
    // into the work matrix (whole tiles: zeros beyond the data, the panel solves read them).
    const double* ab = avec + b * vstride + tj * 64;
    const double* wb = Ws + b * vstride + tj * 64;
    double av[8], wq[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        av[q] = ab[R8(tc, q)];
        wq[q] = wb[R8(tc, q)];
    }
    double* pb = part + b * pstride + (int64_t)tj * (64 * mb) + ti * 64;
    double* Ab = out.base + b * out.cstride;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            s = fma(acc[p][q], av[q], s);
            acc[p][q] *= wq[q];
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (tc == 0) pb[R8(tr, p)] = s;
        pair_store_row(Ab + (row0 + ti * 64 + R8(tr, p)) * out.ld + tj * 64 + 4 * tc, acc[p]);
    }
}

void launch_gram_cross(MatB out, int64_t row0, const double* Xs, int ms, int mb, const double* X,
                       int64_t ldx, int n, int d, int nb, const double* theta, int64_t tstride,
                       const double* sig, const double* bet, const double* lam, int kind,
                       const double* Ws, const double* a, int64_t vstride, double* part,
                       int64_t pstride, Live live, int plain, int nchains, hipStream_t s) {
    const int nsr = (mb + 1) / 2, nsc = (nb + 1) / 2;
    const KernelKind kk = kernel_kind_of(kind);
    APM_FAMILY_DISPATCH(
        kk.family,
        APM_BIAS_DISPATCH(
            kk.bias,
            APM_LINEAR_DISPATCH(kk.linear,
                                APM_LAUNCH((k_gram_cross<FAM, BIAS, LIN>), dim3(nsr * nsc, nchains),
                                           dim3(256), 0, s, out, row0, Xs, ms, mb, X, ldx, n, d, nb,
                                           theta, tstride, sig, bet, lam, kk.iso ? 0 : 1, Ws, a,
                                           vstride, part, pstride, live, plain))));
}

// One wave per (chain, test row): the squared norm of the row of V^T = (W^1/2 . k*)^T L^-T over
// the 64 nb columns (row_sqnorm_d2), mu* from the tile-column partials in order, and the probit
// average through erfc, whose lower tail keeps its relative accuracy (Phi(z) = erfc(-z/sqrt2)/2).
// The logit has no closed form: pi* = sum_q w_q sigma(mu* + sqrt(2 var*) x_q) over the
// Gauss-Hermite table (gh_table.h), one pair of nodes +-x_q per lane and the
// wave's butterfly, a fixed order. With a_q = sqrt(2 var*) x_q >= 0:
//   mu* <  0:  sum_q w_q [sigma(mu* + a_q) + sigma(mu* - a_q)]          (every term positive: the
//                                                                        lower tail stays relative)
//   mu* >= 0:  1/2 + sum_q w_q [sigma(mu* + a_q) - sigma(a_q - mu*)]    (sigma(u) = 1 - sigma(-u),
//                                                                        2 sum_q w_q = 1)
// so an uninformed test point (mu* = 0 exactly) returns 0.5 bitwise, whatever its variance. A
// variance <= 0 (nothing is clamped) takes a_q = 0: sigma(mu*).
template <int LIK>
__global__ __launch_bounds__(256) void k_predict_reduce(
    MatB A, int64_t row0, int ms, int mb, int nb, const double* __restrict__ sig,
    const double* __restrict__ lam, const double* __restrict__ xsn,
    const double* __restrict__ part, int64_t pstride, double* __restrict__ mean,
    double* __restrict__ var, double* __restrict__ prob, int64_t ostride, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= ms) return;
    // (every lane has the norm, mu* and v; the logit's wave stays whole)
    const double s = row_sqnorm_d2(A.base + b * A.cstride + (row0 + r) * A.ld, 64 * nb, lane);
    const double mu = sum_tile_partials(part + b * pstride + r, nb, 64 * mb);
    // (lam: null unless the kind has the linear term; xsn is then not read either)
    const double v = (lam ? fma(lam[b], xsn[r], sig[b]) : sig[b]) - s;
    if constexpr (LIK == APM_LIK_LOGIT) {
        const double sd = v > 0.0 ? sqrt(2.0 * v) : 0.0;
        double acc = 0.0;
        for (int q = lane; q < APM_GH_PAIRS; q += 64) {
            const double a = sd * APM_GH_X[q];
            const double up = sigmoid_d(mu + a);
            acc += APM_GH_W[q] * (mu < 0.0 ? up + sigmoid_d(mu - a) : up - sigmoid_d(a - mu));
        }
        acc = wave_sum_d(acc);
        if (lane != 0) return;
        mean[b * ostride + r] = mu;
        var[b * ostride + r] = v;
        prob[b * ostride + r] = mu < 0.0 ? acc : 0.5 + acc;
    } else {
        if (lane != 0) return;
        const double z = mu / sqrt(1.0 + v);
        mean[b * ostride + r] = mu;
        var[b * ostride + r] = v;
        prob[b * ostride + r] = 0.5 * erfc(-z * 0.70710678118654752440);
    }
}

void launch_predict_reduce(int lik, MatB A, int64_t row0, int ms, int mb, int nb,
                           const double* sig, const double* lam, const double* xsn,
                           const double* part, int64_t pstride, double* mean, double* var,
                           double* prob, int64_t ostride, Live live, int nchains, hipStream_t s) {
    APM_LIK_DISPATCH(lik, APM_LAUNCH(k_predict_reduce<LIK>, dim3((ms + 3) / 4, nchains), dim3(256),
                                     0, s, A, row0, ms, mb, nb, sig, lam, xsn, part, pstride, mean,
                                     var, prob, ostride, live));
}
