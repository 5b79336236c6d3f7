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
// (R&W eqs. 3.65, 3.73-3.74 with tau_- + tau~ = 1/sigma2). These closed-form moments are the
// probit's; k_ep_sites_q takes them by quadrature for either likelihood.
#include "apm_internal.h"
#include "ep_quad.h"

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

// The tilted moments of p(y f) N(f | mu_-, s_-) by quadrature, on a whole wave:
// the sums S_k of p(t) (t - m)^k N(t | m, s_-) over t = y f, m = y mu_-, k = 0, 1, 2, with the
// largest exponent E of their terms taken out, so every lane returns log Z^ = E + log S_0,
// e1 = S_1/S_0 and e2 = S_2/S_0 (mu^ = mu_- + y e1, s^ = e2 - e1^2). Two nodes per lane, the three
// sums by the wave's butterfly, every loop of fixed length; the tables are ep_quad.h's.
//   s_- <= v0: the 128-node Gauss-Hermite rule on the cavity, t_k = m + sqrt(2 s_-) x_k.
//   s_- >  v0: p = H + r with H the unit step and r(t) = -sign(t) p(-|t|), which decays like
//     e^-|t| (logit) or faster. The step's moments about m are closed form in alpha = m/sd:
//     Phi, sd phi, s_- (Phi - alpha phi). The correction is the integral over u of
//     p(-u) [(-u - m)^k N(-u | m, s_-) - (u - m)^k N(u | m, s_-)] by 8-node Gauss-Legendre on 8
//     panels of [0, T_in] and 8 of [T_in, T]. The logit's part at -u is a Gaussian of deviation
//     sd about c = -m - s_- times 1/(1 + e^-u), and [T_in, T] follows that Gaussian down by
//     e^-36 from its peak (c > 0: T = c + 8.5 sd) or from its value at 0 (T = c + sqrt(c^2 +
//     72.25 s_-)), T >= 2 T_in. The probit's T is 2 T_in: its r is below 1e-23 past T_in.
// The covered region (include/apm.h states it): the logit while an outer panel is no wider than
// 2 sd, which is c <= 7.5 sd + 20, and, where c < 0, while alpha >= -30 (there the step dominates
// and the moments about m cancel like alpha^4); the probit while the product's peak is inside
// the nodes (narrow: x* <= 8; wide: -m <= min(5 (1 + s_-), 300), the second bound because the
// moments about m cancel like (m / sd^)^2). A site outside is reported through `covered` and
// fails its chain (APM_STATUS_EP_CAVITY): the rule is never silently wrong.
struct EpMoments {
    double lz, e1, e2;
    bool covered;
};
template <int LIK>
__device__ __forceinline__ EpMoments ep_quad_moments(double m, double vc, int lane) {
    static_assert(APM_EPQ_GH_N == 128 && APM_EPQ_GL_N == 8 && APM_EPQ_PANELS == 16,
                  "two nodes per lane of a wave");
    const double sd = sqrt(vc);
    double E, s0, s1, s2;
    if (vc <= APM_EPQ_V0) {  // (wave-uniform)
        const double sc = 1.4142135623730951 * sd;
        const double d0 = sc * APM_EPQ_GH_X[lane], d1 = sc * APM_EPQ_GH_X[lane + 64];
        const double l0 = lik_logp<LIK>(m + d0) + APM_EPQ_GH_LW[lane];
        const double l1 = lik_logp<LIK>(m + d1) + APM_EPQ_GH_LW[lane + 64];
        E = wave_max_d(fmax(l0, l1));
        const double a0 = exp(l0 - E), a1 = exp(l1 - E);
        s0 = wave_sum_d(a0 + a1);
        s1 = wave_sum_d(a0 * d0 + a1 * d1);
        s2 = wave_sum_d(a0 * d0 * d0 + a1 * d1 * d1);
        // (the probit's integrand peaks at x* = -m sd / (sqrt2 (1 + s_-)) in the rule's variable)
        const bool covered = LIK == APM_LIK_LOGIT ||
                             -m * sd <= APM_EPQ_X_MAX * 1.4142135623730951 * (1.0 + sd * sd);
        return EpMoments{E + log(s0), s1 / s0, s2 / s0, covered};
    }
    constexpr double t_in = LIK == APM_LIK_LOGIT ? APM_EPQ_T_IN_LOGIT : APM_EPQ_T_IN_PROBIT;
    double t_end = 2.0 * t_in;
    bool covered;
    if constexpr (LIK == APM_LIK_LOGIT) {
        const double c = -m - sd * sd, ts = APM_EPQ_TAIL * sd;
        t_end = fmax(t_end, c + (c > 0.0 ? ts : sqrt(c * c + ts * ts)));
        covered = t_end - t_in <= 8.0 * APM_EPQ_H_MAX * sd &&
                  (c >= 0.0 || m >= -APM_EPQ_A_MAX * sd);
    } else {
        covered = -m <= fmin(APM_EPQ_PEAK_MAX * (1.0 + sd * sd), APM_EPQ_M_MAX);
    }
    // lane l: node l & 7 of panel l >> 3 of [0, T_in] (u[0]) and of [T_in, T] (u[1])
    const double frac = ((double)(lane >> 3) + APM_EPQ_GL_XI[lane & 7]) / 8.0;
    const double lwn = APM_EPQ_GL_LW[lane & 7] - 2.0794415416798357;  // (log 8)
    const double u[2] = {t_in * frac, t_in + (t_end - t_in) * frac};
    const double lW[2] = {log(t_in) + lwn, log(t_end - t_in) + lwn};
    const double alpha = m / sd, lsd = log(sd), i2v = 2.0 * sd * sd;
    double lm[2], lp[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double base = lik_logp<LIK>(-u[k]) + lW[k] - lsd - 0.91893853320467274178;
        lm[k] = base - (u[k] + m) * (u[k] + m) / i2v;  // the node at t = -u
        lp[k] = base - (u[k] - m) * (u[k] - m) / i2v;  // the node at t = +u
    }
    const double lP = log_ndtr_d(alpha);
    E = fmax(lP, wave_max_d(fmax(fmax(lm[0], lp[0]), fmax(lm[1], lp[1]))));
    s0 = s1 = s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double am = exp(lm[k] - E), ap = exp(lp[k] - E);
        const double dm = -(u[k] + m), dp = u[k] - m;
        s0 += am - ap;
        s1 += dm * am - dp * ap;
        s2 += dm * dm * am - dp * dp * ap;
    }
    s0 = wave_sum_d(s0);
    s1 = wave_sum_d(s1);
    s2 = wave_sum_d(s2);
    const double P = exp(lP - E), ph = exp(-0.5 * alpha * alpha - 0.91893853320467274178 - E);
    const double z = P + s0;
    return EpMoments{E + log(z), (sd * ph + s1) / z, (sd * sd * (P - alpha * ph) + s2) / z,
                     covered};
}

// k_ep_sites with the tilted moments by quadrature, for either likelihood (apm_set_ep_quadrature):
// the same grid, row norm and outputs; every lane of the wave forms the cavity (the loads are
// wave-uniform), the wave evaluates the rule, and lane 0 finishes the damped sites. The row's
// term of log Z_EP carries log Z^ in the place of log Phi(z); a site outside the rule's covered
// region counts as a bad cavity.
template <int LIK>
__global__ __launch_bounds__(256) void k_ep_sites_q(MatB A, MatB K, int n, int nb, NewtonVecs v,
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
    const double var = K.base[b * K.cstride + (int64_t)r * K.ld + r] - s;
    const double tau = e.tau[o], nu = e.nu[o], yi = y[r];
    const double mu = v.fnew[b * v.vstride + r], dmu = mu - v.f[b * v.vstride + r];
    const double tc = 1.0 / var - tau, nc = mu / var - nu;
    const double muc = nc / tc, vc = 1.0 / tc;
    const EpMoments q = ep_quad_moments<LIK>(yi * muc, vc, lane);
    if (lane != 0) return;
    const double muh = muc + yi * q.e1;
    const double vh = q.e2 - q.e1 * q.e1;
    const double tn = fmax(1.0 / vh - tc, 0.0), nn = muh / vh - nc;
    e.var[o] = var;
    e.ctau[o] = (1.0 - damping) * tau + damping * tn;
    e.cnu[o] = (1.0 - damping) * nu + damping * nn;
    e.lz[o] = q.lz + 0.5 * log1p(tau / tc) + 0.5 * nu * mu - 0.5 * nu * nu * var +
              0.5 * muc * tc * (tau * muc - 2.0 * nu) * var;
    e.dm[o] = dmu * dmu;
    e.bad[o] = (tc > 0.0 && tc < INFINITY && q.covered) ? 0 : 1;  // (a NaN fails the comparisons)
}

void launch_ep_sites_q(int lik, MatB A, MatB K, int n, int nb, NewtonVecs v, const double* y,
                       EpVecs e, double damping, Live live, int nchains, hipStream_t s) {
    APM_LIK_DISPATCH(lik, APM_LAUNCH(k_ep_sites_q<LIK>, dim3((64 * nb + 3) / 4, nchains),
                                     dim3(256), 0, s, A, K, n, nb, v, y, e, damping, live));
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
