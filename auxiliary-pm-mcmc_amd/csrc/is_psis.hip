// Pareto-smoothed leave-one-out densities and the Pareto shape k-hat of the importance ratios
// (DESIGN.md §24): the kernels that host_is_psis.cpp runs after the u-path of apm_u_eval and
// k_is_logw.
//
// §23's product f = f_post + C_chol U once more, with an epilogue that stores every log ratio
//   t_si = log wbar_s - log p(y_i | f_si)
// instead of reducing it (is_loo.hip's k_is_row_gemm pair with its storing epilogue), and one
// workgroup per (chain, row) that sorts the row in LDS, fits the generalised Pareto distribution to
// its upper tail (Zhang & Stephens 2009 with the priors of the `loo` package) and sums the row with
// the tail replaced by the fitted quantiles (k_psis_rows; include/apm.h has the steps). The same
// fit on the row log wbar gives the tail shape of the weights themselves.
#include <cfloat>

#include "apm_internal.h"

// ------------------------------------------------------------------------------- the rows
// The largest tail: M <= ceil(3 sqrt(APM_PSIS_MAX_SAMPLES)) = 192, so the fit's grid has
// m = 30 + floor(sqrt(M)) <= 43 points.
#define PSIS_MAX_TAIL 192
#define PSIS_MAX_GRID 64

// One workgroup of 256 threads per (chain, row): blockIdx.x < n is a row of T, blockIdx.x == n the
// chain's row log wbar (khat_w; its sum is not kept). LDS (dynamic): the row padded with -inf to P,
// the power of two >= S, then the tail's excesses x (PSIS_MAX_TAIL), the grid's b_j, L_j and
// b_j omega_j (PSIS_MAX_GRID each) and the block reductions' four words.
//
// Every sum has a shape that depends on (S, P, M) alone: a thread adds its elements in ascending
// order with stride 256 (the grid: a lane with stride 64), a wave by butterfly, the four waves in
// order (block_sum_d); the grid's row j belongs to wave j mod 4. So a row's result does not depend
// on where it runs. Every branch below is taken by the whole workgroup.
__global__ __launch_bounds__(256) void k_psis_rows(const double* __restrict__ T, int64_t tstride,
                                                   int sp, const double* __restrict__ logw, int S,
                                                   int P, int n, double* __restrict__ out,
                                                   int64_t npr, int64_t qstride,
                                                   double* __restrict__ khat_w,
                                                   const int* __restrict__ status) {
    const int b = blockIdx.y;
    if (status[b] != 0) return;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double* row = r < n ? T + b * tstride + (int64_t)r * sp : logw + (int64_t)b * sp;
    extern __shared__ double psis_lds[];
    double* a = psis_lds;
    double* xs = a + P;
    double* gb = xs + PSIS_MAX_TAIL;
    double* gl = gb + PSIS_MAX_GRID;
    double* gw = gl + PSIS_MAX_GRID;
    double* red = gw + PSIS_MAX_GRID;

    // 1. the finite entries, their maximum, the shifted row and its raw sum
    double mx = -INFINITY, cnt = 0.0;
    for (int s = tid; s < P; s += 256) {
        const double v = s < S ? row[s] : -INFINITY;
        a[s] = v;
        mx = fmax(mx, v);
        cnt += v != -INFINITY ? 1.0 : 0.0;
    }
    mx = block_max_d(mx, red);
    const int Sf = (int)block_sum_d(cnt, red);
    double raw = 0.0;
    for (int s = tid; s < P; s += 256) {
        const double v = a[s] == -INFINITY ? a[s] : a[s] - mx;
        a[s] = v;
        raw += v == -INFINITY ? 0.0 : exp(v);
    }
    raw = block_sum_d(raw, red);  // (its barriers also publish a[])
    int M = (int)ceil(3.0 * sqrt((double)Sf));  // ceil(3 sqrt(S')), made exact in integers
    while (M > 0 && (M - 1) * (M - 1) >= 9 * Sf) --M;
    while (M * M < 9 * Sf) ++M;
    M = min(Sf / 5, M);

    double khat = NAN, res = -(mx + log(raw));
    if (M >= 5) {
        // bitonic sort, ascending: -inf first, the tail in a[P - M .. P)
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = tid; e < P / 2; e += 256) {
                    const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
                    const double u = a[lo], v = a[hi];
                    if ((u > v) == ((lo & k) == 0)) {
                        a[lo] = v;
                        a[hi] = u;
                    }
                }
                __syncthreads();
            }
        // 3. the excesses over the cut
        const double ec = exp(fmax(a[P - M - 1], log(DBL_MIN)));
        if (tid < M) xs[tid] = exp(a[P - M + tid]) - ec;
        __syncthreads();
        const double x1 = xs[0], xM = xs[M - 1];
        if (x1 > 0.0 && xM > x1) {
            // 4. the profile likelihood on the grid b_j
            int m = 30;
            while ((m - 29) * (m - 29) <= M) ++m;  // 30 + floor(sqrt(M))
            const double xq = xs[(M + 2) / 4 - 1];
            for (int j = w; j < m; j += 4) {
                const double bj = 1.0 / xM + (1.0 - sqrt((double)m / (j + 0.5))) / (3.0 * xq);
                double sum = 0.0;
                for (int z = lane; z < M; z += 64) sum += log1p(-bj * xs[z]);
                const double kj = wave_sum_d(sum) / M;
                if (lane == 0) {
                    gb[j] = bj;
                    gl[j] = M * (log(-bj / kj) - kj - 1.0);
                }
            }
            __syncthreads();
            if (tid < m) {
                double den = 0.0;
                for (int l = 0; l < m; ++l) den += exp(gl[l] - gl[tid]);
                gw[tid] = gb[tid] * (1.0 / den);
            }
            __syncthreads();
            double bh = 0.0;
            for (int j = 0; j < m; ++j) bh += gw[j];
            const double k = block_sum_d(tid < M ? log1p(-bh * xs[tid]) : 0.0, red) / M;
            const double sigma = -k / bh;
            khat = (M * k + 5.0) / (M + 10.0);
            if (isfinite(khat) && isfinite(sigma)) {
                // 5. the tail's quantiles, capped at the largest raw ratio; 6. the sum
                double q = 0.0;
                if (tid < M) {
                    const double l1 = log1p(-(tid + 0.5) / M);
                    q = khat == 0.0 ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
                    q = fmin(q + ec, 1.0);
                }
                for (int s = P - Sf + tid; s < P - M; s += 256) q += exp(a[s]);
                res = -(mx + log(block_sum_d(q, red)));
            }
        }
    }
    if (tid == 0) {
        if (r < n) {
            out[b * npr + r] = res;
            out[qstride + b * npr + r] = khat;
        } else {
            khat_w[b] = khat;
        }
    }
}

void launch_psis_rows(const double* T, int64_t tstride, int sp, const double* logw, int S, int n,
                      double* out, int64_t npr, int64_t qstride, double* khat_w,
                      const int* status, int nchains, hipStream_t s) {
    int P = 2;
    while (P < S) P <<= 1;
    const size_t lds = sizeof(double) * (P + PSIS_MAX_TAIL + 3 * PSIS_MAX_GRID + 4);
    APM_LAUNCH(k_psis_rows, dim3(n + 1, nchains), dim3(256), lds, s, T, tstride, sp, logw, S, P, n,
               out, npr, qstride, khat_w, status);
}
