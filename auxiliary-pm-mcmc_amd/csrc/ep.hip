// Parallel expectation propagation for the probit: the three kernels of a sweep
// that are EP's own. The posterior from the current sites is the fp64 Newton iteration's algebra
// with W := tau~ and b := nu~ (newton.hip, chol.hip) and the rows of V^T = (K S^1/2) L^-T are
// grad_block's first pass (k_form_aug, chol_solve_rows); host_ep.cpp runs the sweep loop.
//
//   sigma2_i = K_ii - |V_i|^2,  tau_- = 1/sigma2 - tau~,  nu_- = mu/sigma2 - nu~,
//   mu_- = nu_-/tau_-,  s_- = 1/tau_-,  z = y mu_- / sqrt(1 + s_-),  r = phi(z)/Phi(z),
//   mu^ = mu_- + y s_- r / sqrt(1 + s_-),  s^ = s_- - s_-^2 r (z + r)/(1 + s_-),
//   tau~_new = max(1/s^ - tau_-, 0),  nu~_new = mu^/s^ - nu_-,  damped by delta;
//   log Z_EP = sum_i [log Phi(z) + 1/2 log(1 + tau~/tau_-) + 1/2 nu~ mu - 1/2 nu~^2 sigma2
//              + 1/2 mu_- tau_- (tau~ mu_- - 2 nu~) sigma2] - sum_i log L_ii
// (R&W eqs. 3.65, 3.73-3.74 with tau_- + tau~ = 1/sigma2). Probit only: the logit's tilted
// moments need quadrature.
#include "apm_internal.h"

// S^1/2 and nu~ into the Newton vectors (Ws, W, b); rows >= n have tau~ = nu~ = 0 throughout
__global__ __launch_bounds__(256) void k_ep_prep(EpVecs e, NewtonVecs v, int np, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const double t = e.tau[b * e.stride + i];
    const int64_t o = b * v.vstride + i;
    v.W[o] = t;
    v.Ws[o] = sqrt(t);
    v.b[o] = e.nu[b * e.stride + i];
}

void launch_ep_prep(EpVecs e, NewtonVecs v, int np, Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_ep_prep, dim3((np + 255) / 256, nchains), dim3(256), 0, s, e, v, np, live);
}

// One wave per (chain, training row r): the squared norm of row np + r of the work matrix over
// its first 64 nb columns (row_sqnorm_d2, as k_grad_rows), then on lane 0 the marginal
// variance, the cavity, the tilted moments, the damped candidate sites and the row's terms of
// log Z_EP and of the stop measure. Rows >= n get exact zeros and enter no sum.
__global__ __launch_bounds__(256) void k_ep_sites(MatB A, MatB K, int n, int nb, NewtonVecs v,
                                                  const double* __restrict__ y, EpVecs e,
                                                  double damping, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int np = 64 * nb;
    if (r >= np) return;
    const int64_t o = b * e.stride + r;
    if (r >= n) {  // (wave-uniform)
        if (lane == 0) {
            e.var[o] = e.ctau[o] = e.cnu[o] = e.lz[o] = e.dm[o] = 0.0;
            e.bad[o] = 0;
        }
        return;
    }
    const double s = row_sqnorm_d2(A.base + b * A.cstride + (int64_t)(np + r) * A.ld, np, lane);
    if (lane != 0) return;
    const double var = K.base[b * K.cstride + (int64_t)r * K.ld + r] - s;
    const double tau = e.tau[o], nu = e.nu[o], yi = y[r];
    const double mu = v.fnew[b * v.vstride + r], dmu = mu - v.f[b * v.vstride + r];
    const double tc = 1.0 / var - tau, nc = mu / var - nu;
    const double muc = nc / tc, vc = 1.0 / tc;
    const double den = 1.0 + vc, sq = sqrt(den);
    const double z = yi * muc / sq;
    const double lp = log_ndtr_d(z);
    const double rr = exp(-0.5 * z * z - lp - 0.91893853320467274178);
    const double muh = muc + yi * vc * rr / sq;
    const double vh = vc - vc * vc * rr * (z + rr) / den;
    const double tn = fmax(1.0 / vh - tc, 0.0), nn = muh / vh - nc;
    e.var[o] = var;
    e.ctau[o] = (1.0 - damping) * tau + damping * tn;
    e.cnu[o] = (1.0 - damping) * nu + damping * nn;
    e.lz[o] = lp + 0.5 * log1p(tau / tc) + 0.5 * nu * mu - 0.5 * nu * nu * var +
              0.5 * muc * tc * (tau * muc - 2.0 * nu) * var;
    e.dm[o] = dmu * dmu;
    e.bad[o] = (tc > 0.0 && tc < INFINITY) ? 0 : 1;  // (a NaN fails both comparisons)
}

void launch_ep_sites(MatB A, MatB K, int n, int nb, NewtonVecs v, const double* y, EpVecs e,
                     double damping, Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_ep_sites, dim3((64 * nb + 3) / 4, nchains), dim3(256), 0, s, A, K, n, nb, v, y,
               e, damping, live);
}

// Per chain: the rows' terms summed in a fixed order (block_sum_d: each thread its rows in
// order, the wave's butterfly, the waves in order), sum log L_ii from ldet, the cavity check and
// the stop rule. A chain that goes on takes the candidate sites; a converged one keeps the sites
// its posterior was built from, so every output is the state of one sweep. mu_prev <- mu.
__global__ __launch_bounds__(256) void k_ep_chain(EpVecs e, NewtonVecs v, int n, int np,
                                                  const double* __restrict__ ldet,
                                                  int64_t lstride, int nb, double diff_tol,
                                                  int fail_code, int* active, int* status,
                                                  int* n_iter) {
    const int b = blockIdx.x;
    if (active[b] == 0 || status[b] != 0) return;
    __shared__ double red[4];
    const int64_t eo = b * e.stride, vo = b * v.vstride;
    double lz = 0.0, dm = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        lz += e.lz[eo + i];
        dm += e.dm[eo + i];
        bad += (double)e.bad[eo + i];
    }
    lz = block_sum_d(lz, red);
    __syncthreads();
    dm = block_sum_d(dm, red);
    __syncthreads();
    bad = block_sum_d(bad, red);
    const int sweep = n_iter[b] + 1;  // (uniform: read before thread 0 writes it, below the
    __syncthreads();                  //  barrier)
    const bool failed = bad != 0.0;
    const bool done = !failed && sweep >= 2 && dm / n < diff_tol;
    if (!failed && !done)
        for (int i = threadIdx.x; i < np; i += 256) {
            e.tau[eo + i] = e.ctau[eo + i];
            e.nu[eo + i] = e.cnu[eo + i];
        }
    for (int i = threadIdx.x; i < np; i += 256) v.f[vo + i] = v.fnew[vo + i];
    if (threadIdx.x == 0) {
        n_iter[b] = sweep;
        if (failed) {
            status[b] = fail_code;
        } else if (done) {
            double ld = 0.0;
            for (int k = 0; k < nb; ++k) ld += ldet[b * lstride + k];
            e.logz[b] = lz - ld;
            active[b] = 0;
        }
    }
}

void launch_ep_chain(EpVecs e, NewtonVecs v, int n, int np, const double* ldet, int64_t lstride,
                     int nb, double diff_tol, int fail_code, int* active, int* status,
                     int* n_iter, int nchains, hipStream_t s) {
    APM_LAUNCH(k_ep_chain, dim3(nchains), dim3(256), 0, s, e, v, n, np, ldet, lstride, nb,
               diff_tol, fail_code, active, status, n_iter);
}

// The hand-over of a converged fit to the posterior-factor and slot code of the IS theta-call
// (host_theta.cpp), once per call after the stop sweep, live chains only. That
// code reads the Newton vectors: f_post from v.f (post_cov_lk's right-hand side, the slot, the
// guard's row residuals), W from v.W (the slot's z = a + W f_post = nu~), W^1/2 from v.Ws
// (k_form_y2_rev, icm_check) and a from v.a. The stop sweep left tau~, S^1/2 and its a there, which
// stay; mu of that sweep (v.fnew = K a) is written into v.f, so the state handed over does not rest
// on k_ep_chain's mu_prev <- mu, and rows >= n of the four vectors are set to exact zeros, as the
// factor's right-hand side row and the padded rows of Y2 = S^1/2 L_K expect them. Two rows per
// thread, one 16-byte access per vector (vstride and np are multiples of 64).
__global__ __launch_bounds__(256) void k_ep_handoff(NewtonVecs v, int n, int np, Live live) {
    const int b = blockIdx.y;
    if (!live_chain(live, b)) return;
    const int i = 2 * (blockIdx.x * 256 + threadIdx.x);
    if (i >= np) return;
    const int64_t o = b * v.vstride + i;
    if (i + 1 < n) {
        *reinterpret_cast<d2_t*>(v.f + o) = *reinterpret_cast<const d2_t*>(v.fnew + o);
        return;
    }
    const d2_t zero = d2_t{0.0, 0.0};
    if (i >= n) {
        *reinterpret_cast<d2_t*>(v.f + o) = zero;
        *reinterpret_cast<d2_t*>(v.W + o) = zero;
        *reinterpret_cast<d2_t*>(v.Ws + o) = zero;
        *reinterpret_cast<d2_t*>(v.a + o) = zero;
        return;
    }
    // i = n - 1 (n odd): row i is the last training row, row i + 1 the first padded one
    *reinterpret_cast<d2_t*>(v.f + o) = d2_t{v.fnew[o], 0.0};
    *reinterpret_cast<d2_t*>(v.W + o) = d2_t{v.W[o], 0.0};
    *reinterpret_cast<d2_t*>(v.Ws + o) = d2_t{v.Ws[o], 0.0};
    *reinterpret_cast<d2_t*>(v.a + o) = d2_t{v.a[o], 0.0};
}

void launch_ep_handoff(NewtonVecs v, int n, int np, Live live, int nchains, hipStream_t s) {
    APM_LAUNCH(k_ep_handoff, dim3((np / 2 + 255) / 256, nchains), dim3(256), 0, s, v, n, np, live);
}
