/*
 * apm.h — C-ABI of the MI355X-native auxiliary-pseudo-marginal GP-classification hot path
 * (libapm.so, built from auxiliary-pm-mcmc_amd/csrc/). Plain pointers and sizes only.
 *
 * Every entry point replaces a reference interface on the per-step log-pseudo-marginal path
 * (matt-graham/auxiliary-pm-mcmc, paths relative to the reference root):
 *
 *   apm_gram           <- gpdemo/kernels.pyx:12-49  isotropic_squared_exponential_kernel(K, X, theta, epsilon)
 *                         gpdemo/kernels.pyx:52-90  diagonal_squared_exponential_kernel(K, X, theta, epsilon)
 *   apm_gram_cross     <- the same two kernels between two point sets (their i != j entries)
 *   apm_predict        <- no reference counterpart: the Laplace predictive distribution at test
 *                         inputs from the Newton quantities of laplace_approximation (:81-112)
 *   apm_laplace_grad   <- no reference counterpart: the gradient of the Laplace log marginal
 *                         likelihood (:103-106) with respect to theta
 *   apm_ep_eval        <- no reference counterpart: expectation propagation for the probit (the
 *   apm_ep_predict        fit, log Z_EP, the marginals and the predictive distribution; R&W §3.6)
 *   apm_ep                with the sweeps' factorisations and solves on the device; the logit by
 *   apm_ep_lik            quadrature of the tilted moments (apm_set_ep_quadrature, opt-in)
 *   apm_ep_grad        <- no reference counterpart: the gradient of log Z_EP with respect to theta
 *   apm_u_eval_diag    <- no reference counterpart: the cached u-call cut into blocks of samples, with
 *   apm_is_spread         each block's weight ESS, over independent redraws of u on the device
 *   apm_laplace        <- gpdemo/latent_posterior_approximations.py:22-124  laplace_approximation(K, y, ...)
 *   apm_theta_eval     <- gpdemo/estimators.py:201-217 (+ :221-241)  ApproxPosteriorIS.__call__(ns, theta)
 *                         gpdemo/estimators.py:317-325               PriorMC.__call__(ns, theta)
 *                         gpdemo/estimators.py:65-82                 Laplace.__call__(theta)
 *   apm_u_eval         <- gpdemo/estimators.py:218-241  ApproxPosteriorIS.__call__(ns, cached_results=...)
 *                         gpdemo/estimators.py:323-325  PriorMC.__call__(ns, K_chol=...)
 *   apm_u_*            <- the u_sampler / elliptical-slice proposal of auxpm/samplers.py:780-788 and
 *                         auxpm/mcmc_updates.py:382 kept on the device (batched driver)
 *
 * The estimator's cached_results tuple (K_chol, C_chol, f_post) (estimators.py:166-176) becomes an
 * opaque, context-owned cache SLOT; draws u become context-owned device U BUFFERS.
 * Batched entry points evaluate `count` independent chains per call (one chain per index).
 *
 * All calls are synchronous with respect to the host (results are in host memory on return).
 * Return value: 0 on success, a negative APM_E_* code on an API/HIP failure (message via
 * apm_last_error / apm_global_error). Per-chain numerical failures are reported in status[]
 * (APM_STATUS_*), which the Python layer maps onto the reference's exceptions.
 */
#ifndef APM_H
#define APM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APM_SUCCESS 0
#define APM_E_INVALID (-1)
#define APM_E_HIP (-2)
#define APM_E_NOMEM (-3)

/* per-chain status */
#define APM_STATUS_OK 0
#define APM_STATUS_CHOL_K 1   /* chol(K) not PD        -> numpy.linalg.LinAlgError (estimators.py:321) */
#define APM_STATUS_CHOL_B 2   /* chol(B) not PD        -> numpy.linalg.LinAlgError (lpa.py:92) */
#define APM_STATUS_CHOL_C 3   /* chol(C) not PD        -> InvalidCovarianceMatrixError (estimators.py:208-215) */
#define APM_STATUS_MAXITER 4  /* Newton not converged  -> MaximumIterationsExceededError (lpa.py:100-102) */
#define APM_STATUS_GUARD 5    /* a device-side invariant of the theta-call failed (apm_guard_read;
                                 DESIGN.md §11): the value is withheld -> DeviceInvariantError
                                 (no reference counterpart: the reference has no device) */
#define APM_STATUS_EP_CAVITY 6 /* an EP cavity precision 1/sigma_i^2 - tau~_i was <= 0 or not finite,
                                  or (moments by quadrature) a site left the rule's covered region
                                  -> InvalidCavityError (no reference counterpart: the reference has
                                  no EP) */

/* covariance kernels */
#define APM_KERNEL_ISO 0         /* kernels.pyx:12-49, theta = (log sigma, log tau) */
#define APM_KERNEL_ARD 1         /* kernels.pyx:52-90, theta = (log sigma, log tau_1..tau_D) */
#define APM_KERNEL_PRECOMPUTED 2 /* K supplied by the caller (apm_theta_eval_K) */
/* Matern covariance functions, built on the device like the two SE kernels (no reference
 * counterpart: kernels.pyx has the SE family only). Same theta layout as ISO / ARD: s =
 * exp(theta_0), tau_k = exp(theta_{k+1}) (ARD, d + 1 entries) or exp(theta_1) for every k (ISO, 2
 * entries), r = sqrt(sum_k ((x_ik - x_jk)/tau_k)^2):
 *   Matern 3/2  S = s (1 + sqrt3 r) exp(-sqrt3 r)
 *   Matern 5/2  S = s (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)
 * with the SE kernels' epsilon rule: K = S + epsilon I on one point set's Gram only, none on
 * apm_gram_cross / k*, prior variance k** = s. Accepted wherever ISO / ARD are: apm_create,
 * apm_gram, apm_gram_cross, apm_theta_eval (all estimators), apm_predict, apm_laplace_grad. */
#define APM_KERNEL_M32_ISO 3
#define APM_KERNEL_M32_ARD 4
#define APM_KERNEL_M52_ISO 5
#define APM_KERNEL_M52_ARD 6
/* Constant (bias) term, a flag OR-ed onto one of the six kinds above (kinds 16, 17, 19 .. 22; not
 * onto APM_KERNEL_PRECOMPUTED): K = S + beta 1 1^T + epsilon I, a N(0, beta) prior on a constant
 * offset of the latent function, integrated out. theta gains one entry, the last one:
 * beta = exp(theta[P - 1]) with P = apm_theta_len = the base kind's length + 1. beta is added to
 * every pair of data points (K_ii = s + beta + epsilon), to the cross-covariance k* (no epsilon)
 * and to the prior variance k** = s + beta; dK/dtheta_{P-1} = beta on every data pair. Accepted
 * wherever the base kinds are; gradients have P entries. */
#define APM_COV_BIAS 16
/* Linear (dot-product) term, a flag OR-ed onto APM_KERNEL_ISO or APM_KERNEL_ARD, with or without
 * APM_COV_BIAS (kinds 64, 65, 80, 81; refused on a Matern kind and on APM_KERNEL_PRECOMPUTED):
 * K = S [+ beta 1 1^T] + lambda X X^T + epsilon I, a N(0, lambda I) prior on the weights of a
 * linear function of the raw (unscaled) inputs, integrated out. theta gains one entry, the last
 * one: lambda = exp(theta[P - 1]) with P = apm_theta_len = the base kind's length [+ 1] + 1; with
 * both flags beta = exp(theta[P - 2]). K_ii = s [+ beta] + lambda |x_i|^2 + epsilon, the
 * cross-covariance gains lambda x*_i . x_j (no epsilon) and the prior variance at a test point is
 * s [+ beta] + lambda |x*_i|^2; dK/dtheta_{P-1} = lambda x_i . x_j on every data pair. Accepted
 * wherever the base kinds are; gradients have P entries. A caller detects the feature by this
 * macro (apm_version() is unchanged). */
#define APM_COV_LINEAR 64

/* estimators */
#define APM_EST_IS 0       /* LogMarginalLikelihoodApproxPosteriorISEstimator */
#define APM_EST_PRIORMC 1  /* LogMarginalLikelihoodPriorMCEstimator */
#define APM_EST_LAPLACE 2  /* LogMarginalLikelihoodLaplaceEstimator */
/* APM_EST_IS with the importance distribution N(mu, (K^-1 + diag tau~)^-1) of the converged
 * expectation-propagation fit (apm_set_ep settings) in place of the Laplace
 * posterior. APM_E_INVALID on an APM_LIK_LOGIT context unless apm_set_ep_quadrature is on.
 * The cache slot holds the same state as an APM_EST_IS slot (f_post = mu, W = tau~, z = nu~,
 * cst = 1/2 mu^T nu~ - 1/2 log|B|), so apm_u_eval, apm_slot_read, apm_guard_read and the apm_cache_* calls serve it
 * unchanged. status[i]: APM_STATUS_CHOL_B, APM_STATUS_EP_CAVITY or APM_STATUS_MAXITER of the fit,
 * APM_STATUS_CHOL_K, APM_STATUS_CHOL_C or APM_STATUS_GUARD as for APM_EST_IS; a failed chain is
 * treated as a failed APM_EST_IS chain. n_cubic_ops[i] = 2 n_sweeps + 1 + 2 (two per sweep,
 * DESIGN.md §16, plus APM_EST_IS's own). apm_version() is unchanged: detect it by this macro. */
#define APM_EST_IS_EP 3

/* likelihoods p(y | f) of a label y in {-1, +1} (R&W §3.4; the reference has the probit only):
 *   PROBIT  Phi(y f)     the default of every context and of apm_laplace
 *   LOGIT   sigma(y f) = 1 / (1 + exp(-y f)); with t = y f:
 *           log p = -log1p(exp(-t)) (t >= 0), t - log1p(exp(t)) (t < 0),
 *           grad = d log p/df = y sigma(-t), W = -d^2 log p/df^2 = sigma(t) sigma(-t) in (0, 1/4],
 *           d3 = d^3 log p/df^3 = -y W (1 - 2 sigma(t)); sigma(-t) is formed as 1/(1 + exp(t)),
 *           never as 1 - sigma(t). */
#define APM_LIK_PROBIT 0
#define APM_LIK_LOGIT 1

typedef struct apm_ctx apm_ctx;

/* 3: the likelihoods APM_LIK_* (apm_set_likelihood, apm_laplace_lik); 2: the Matern kinds
 * APM_KERNEL_M32_* / APM_KERNEL_M52_* (1: SE and PRECOMPUTED only) */
int apm_version(void);
int apm_device_count(void);
const char *apm_global_error(void);

/* ---- context: data (X, y) resident on `device`, workspaces for max_batch chains ------------- */
apm_ctx *apm_create(int device, int kernel_kind, const double *X, int64_t n, int64_t d,
                    int64_t ldx, const double *y, double epsilon, int64_t n_imp,
                    int64_t max_batch, int64_t n_slots, int64_t n_ubufs);
void apm_destroy(apm_ctx *ctx);
const char *apm_last_error(const apm_ctx *ctx);
int64_t apm_padded_n(const apm_ctx *ctx);
int64_t apm_theta_len(const apm_ctx *ctx);
/* Newton settings of laplace_approximation (diff_f_tol, max_iters); defaults 1e-4, 1000 */
int apm_set_newton(apm_ctx *ctx, double diff_f_tol, int64_t max_iters);
/* The likelihood (APM_LIK_*; default APM_LIK_PROBIT) of every later call on the context:
 * apm_theta_eval (all three estimators), apm_theta_eval_K, apm_u_eval, apm_predict and
 * apm_laplace_grad. APM_E_INVALID for an unknown value. A cache slot holds the state of the
 * likelihood it was written under (W, z and cst of that likelihood's Laplace fit): reading it
 * with apm_u_eval under the other one is the caller's error and is not detected. The IS estimate
 * log w_s = sum_n [log p(y_n|f_sn) + 1/2 W_n f_sn^2 - z_n f_sn] + cst holds for either likelihood
 * (W the one the proposal was built from); PriorMC is the same with W = z = 0. */
int apm_set_likelihood(apm_ctx *ctx, int lik);
/* the context's likelihood (negative on a null context) */
int apm_likelihood(const apm_ctx *ctx);
/* hipStream_t the context launches on (for device-side timing by the caller) */
void *apm_stream(apm_ctx *ctx);

/* ---- U buffers (n x n_imp standard-normal draws, fp32 on device) ----------------------------- */
int apm_u_upload(apm_ctx *ctx, int64_t ubuf, const double *U, int64_t ldu);
int apm_u_download(apm_ctx *ctx, int64_t ubuf, double *U, int64_t ldu);
/* Philox4x32-10 normals: buffer ubufs[i] <- N(0,1) stream (seeds[i], counters[i]) */
int apm_u_normal(apm_ctx *ctx, int64_t count, const int64_t *ubufs, const uint64_t *seeds,
                 const uint64_t *counters);
/* dst[i] <- ca[i] * a[i] + cb[i] * b[i]  (elliptical-slice proposal u cos(phi) + nu sin(phi)) */
int apm_u_combine(apm_ctx *ctx, int64_t count, const int64_t *dst, const int64_t *a,
                  const int64_t *b, const double *ca, const double *cb);

/* ---- estimator calls ------------------------------------------------------------------------- */
/* theta-call for `count` chains: thetas row i (ldt stride) -> log-estimate out_logf[i]; the
 * per-theta state is written to cache slot slots[i]. ubufs/slots are ignored for APM_EST_LAPLACE.
 * n_cubic_ops[i] follows the reference's accounting (estimators.py:81,217,322). out_logf[i] is
 * NaN where status[i] != 0. */
int apm_theta_eval(apm_ctx *ctx, int estimator, int64_t count, const double *thetas, int64_t ldt,
                   const int64_t *ubufs, const int64_t *slots, double *out_logf, int *status,
                   int64_t *n_cubic_ops);
/* the same for one chain with K (n x n, ldk) computed by the caller (any kernel_func) */
int apm_theta_eval_K(apm_ctx *ctx, int estimator, const double *K, int64_t ldk, int64_t ubuf,
                     int64_t slot, double *out_logf, int *status, int64_t *n_cubic_ops);
/* Laplace predictive at m test inputs Xs (m x d, ldxs) for `count` thetas (count <= max_batch):
 * Gram -> fp64 Newton (apm_set_newton settings) -> mean/var/prob, each count x m with row stride
 * ldo (any of the three may be NULL). status[i]: APM_STATUS_* of chain i (outputs of a failed
 * chain are NaN); n_iter[i] (may be NULL): Newton iterations. Needs an ISO or ARD context of
 * any family (SE, Matern 3/2, Matern 5/2), not a PRECOMPUTED one.
 * mean = k*^T a, var = s - |L^-1 (W^1/2 . k*)|^2 with s = exp(theta_0) (no epsilon on k* or k**:
 * kernels.pyx adds it to the diagonal of one point set's Gram only), prob = Phi(mean /
 * sqrt(1 + var)); W, L, a of the last Newton iteration (lpa.py:81-112). Nothing is clamped.
 * Under APM_LIK_LOGIT mean and var are the same expressions (with the logit's W, L, a) and prob
 * = int sigma(x) N(x | mean, var) dx has no closed form: it is the Gauss-Hermite average
 * sum_q w_q sigma(mean + sqrt(2 var) x_q) over the 400-node rule (its 128 central nodes; the
 * others carry 3e-24 of the weight), summed in pairs +-x_q in a fixed order, so that mean = 0
 * gives 0.5 bitwise. The rule is exact to 1e-12 for var <= 20 and to 2e-6 for var <= 100; at var
 * = e^6 it is 4e-4 off. var <= 0 is returned as computed, and prob is then
 * sigma(mean).
 * Uses the context's work matrix like every theta-call; cache slots are not touched. */
int apm_predict(apm_ctx *ctx, int64_t count, const double *thetas, int64_t ldt,
                const double *Xs, int64_t m, int64_t ldxs, double *mean, double *var,
                double *prob, int64_t ldo, int *status, int64_t *n_iter);
/* Importance-sampling predictive at m test inputs Xs (m x d, ldxs) for `count` chains (count <=
 * max_batch), estimator APM_EST_IS or APM_EST_IS_EP. The call first IS apm_theta_eval(estimator,
 * ...) on the same thetas, ubufs and slots: the slots are written, out_logf[i], status[i] and the
 * failure handling are that call's, out_logf[i] bitwise. Then, for the chains that are OK, with
 * the importance samples f_s = f_post + C_chol u_s of U buffer ubufs[i] and their self-normalised
 * weights wbar_s (the summands of the estimate, exp(log w_s - max) / sum over the S real samples;
 * padded sample columns weigh exactly 0):
 *   p_j = L_K^-1 k*_j (k* = k(X, x*_j), no epsilon), v*_j = s - |p_j|^2, s = exp(theta_0),
 *   h_j = U_M^-1 p_j (M = I + L_K^T W L_K = U_M U_M^T), c_j = k*_j^T a, a = K^-1 f_post,
 *   m_sj = E[f*_j | f_s] = c_j + h_j^T u_s,
 *   prob_j = sum_s wbar_s Phi(m_sj / sqrt(1 + v*_j))      (APM_LIK_PROBIT)
 *          = sum_s wbar_s GH(m_sj, v*_j)                   (APM_LIK_LOGIT: apm_predict's rule)
 *   mean_j = sum_s wbar_s m_sj,  var_j = v*_j + sum_s wbar_s m_sj^2 - mean_j^2,
 *   ess = 1 / sum_s wbar_s^2,
 * prob / mean / var count x m with row stride ldo >= m, ess count; any of the four may be NULL.
 * Averaged over the iterations of a pseudo-marginal chain whose state is (theta, u), prob is a
 * consistent estimate of the exact posterior predictive at any fixed number of samples. Nothing
 * is clamped; the tail is fp64 throughout and never applies K^-1 to a computed f_s (DESIGN.md
 * §19). The outputs of a chain that is not OK are NaN. n_cubic_ops[i] (may be NULL) is the
 * theta-call's own plus 2 for an OK chain: the tail factors K and J M J again in fp64; the two n x m
 * row solves are not counted, as apm_predict does not count its own. APM_E_INVALID for any other
 * estimator, a PRECOMPUTED context, APM_EST_IS_EP under APM_LIK_LOGIT and count > max_batch. A
 * chain's outputs do not depend on its position in the batch nor on the other chains; the U
 * buffers are not modified. apm_version() is unchanged: detect the entry point by its symbol. */
int apm_is_predict(apm_ctx *ctx, int estimator, int64_t count, const double *thetas, int64_t ldt,
                   const int64_t *ubufs, const int64_t *slots, const double *Xs, int64_t m,
                   int64_t ldxs, double *out_logf, double *prob, double *mean, double *var,
                   int64_t ldo, double *ess, int *status, int64_t *n_cubic_ops);
/* Gradient of the Laplace log marginal likelihood with respect to theta for `count` thetas
 * (count <= max_batch): Gram -> fp64 Newton (apm_set_newton settings) -> lml[i] (may be NULL) and
 * grad row i (count x P, row stride ldg >= P = apm_theta_len). status[i]: APM_STATUS_* of chain i
 * (lml and the grad row of a failed chain are NaN); n_iter[i] (may be NULL): Newton iterations.
 * Needs an ISO or ARD context of any family, not a PRECOMPUTED one. No reference counterpart. With W, W^1/2, L = chol(I + W^1/2 K
 * W^1/2), a of the last Newton iteration and the mode f = K a (lpa.py:81-106):
 *   v = phi(f)/Phi(y f), g = y v, d3 = -[(2v + y f)(-f v - y v^2) + y v],
 *   R = Z^T Z with Z = L^-1 diag(W^1/2), dS_i = K_ii - |L^-1 (W^1/2 . K[:, i])|^2,
 *   s2 = 1/2 dS . d3, q = s2 - R (K s2), M = 1/2 a a^T - 1/2 R + 1/2 (q g^T + g q^T),
 *   grad_j = sum_ik M_ik (dK/dtheta_j)_ik,
 * dK/dtheta_0 = S, the covariance function WITHOUT epsilon (its diagonal is exp(theta_0): the
 * jitter kernels.pyx adds does not depend on theta), dK/dtheta_{k+1} = S_ik ((x_ik - x_jk) /
 * tau_k)^2 (ARD) or the sum over k of these (ISO); K = S + epsilon I everywhere else. For a
 * Matern kind the length-scale derivative is G_ik ((x_ik - x_jk) / tau_k)^2 with G = 3 s
 * exp(-sqrt3 r) (3/2) or G = 5/3 s (1 + sqrt5 r) exp(-sqrt5 r) (5/2): finite at r = 0, zero
 * diagonal; dK/dtheta_0 = S as for SE. Under APM_LIK_LOGIT the same formulas hold with the
 * logit's g = y sigma(-y f) and d3 = -y W (1 - 2 sigma(y f)), W = sigma(y f) sigma(-y f) (and
 * the logit's W, L, a, f). This is the
 * derivative at the exact mode: at a loose diff_f_tol it is approximate.
 * lml[i] is bitwise the value apm_theta_eval(APM_EST_LAPLACE) returns for the same theta and
 * Newton settings: that call always takes this fp64 Newton path, so no setting is needed.
 * A chain's outputs do not depend on its position in the batch nor on the other chains. Uses the
 * context's work matrix like every theta-call; cache slots and U buffers are not touched. */
int apm_laplace_grad(apm_ctx *ctx, int64_t count, const double *thetas, int64_t ldt, double *lml,
                     double *grad, int64_t ldg, int *status, int64_t *n_iter);
/* ---- expectation propagation (no reference counterpart) ----------------------
 * Parallel EP for the probit likelihood, labels y in {-1, +1}. From tau~ = nu~ = 0, sweep t = 1,
 * 2, ...:
 *   1. S^1/2 = sqrt(tau~), L = chol(I + S^1/2 K S^1/2) (failure: APM_STATUS_CHOL_B),
 *      a = nu~ - S^1/2 B^-1 S^1/2 K nu~, mu = K a, V = L^-1 (S^1/2 K), sigma2_i = K_ii - sum_r V_ri^2;
 *   2. tau_- = 1/sigma2 - tau~, nu_- = mu/sigma2 - nu~, mu_- = nu_-/tau_-, s_- = 1/tau_-; a tau_-
 *      that is <= 0 or not finite fails the chain with APM_STATUS_EP_CAVITY;
 *      z = y mu_- / sqrt(1 + s_-);
 *   3. for t >= 2: mean_i (mu_i - mu_i of sweep t - 1)^2 < diff_tol stops the chain with no site
 *      update, so sites, L, a, mu and sigma2 returned are those of one sweep, n_sweeps = t; a
 *      chain not stopped after sweep max_sweeps fails with APM_STATUS_MAXITER;
 *   4. r = phi(z)/Phi(z), mu^ = mu_- + y s_- r / sqrt(1 + s_-), s^ = s_- - s_-^2 r (z + r)/(1 + s_-);
 *   5. tau~_new = max(1/s^ - tau_-, 0), nu~_new = mu^/s^ - nu_-, tau~ <- (1 - damping) tau~ +
 *      damping tau~_new and nu~ likewise (the clamp removes rounding only: tau~_new >= 0 holds
 *      exactly for the probit).
 *   log Z_EP = sum log Phi(z_i) + 1/2 sum log(1 + tau~_i/tau_-i) - sum log L_ii + 1/2 nu~^T mu
 *              - 1/2 sum nu~_i^2 sigma2_i + 1/2 sum mu_-i tau_-i (tau~_i mu_-i - 2 nu~_i) sigma2_i
 * (R&W eqs. 3.65, 3.73-3.74), every sum over the n data rows in a fixed order. Everything is
 * fp64. These closed-form moments are the default, and with them every EP entry point returns
 * APM_E_INVALID on a context whose likelihood is APM_LIK_LOGIT (its tilted moments have no closed
 * form and need quadrature).
 *
 * Moments by quadrature (apm_set_ep_quadrature(ctx, 1)) replace step 4 for either
 * likelihood p, and open every EP entry point, APM_EST_IS_EP included, to the logit. With t = y f,
 * m = y mu_-, sd = sqrt(s_-), the rule forms S_k = int p(t) (t - m)^k N(t | m, s_-) dt, k = 0, 1,
 * 2, with the largest exponent of its terms taken out, and
 *   log Z^ = log S_0,  mu^ = mu_- + y S_1/S_0,  s^ = S_2/S_0 - (S_1/S_0)^2;
 * log Z_EP carries sum log Z^_i in the place of sum log Phi(z_i) (the same number for the probit).
 *   s_- <= 5: the 128-node Gauss-Hermite rule on the cavity, t_k = m + sqrt(2) sd x_k.
 *   s_- >  5: p = H + r, H the unit step, r(t) = -sign(t) p(-|t|). The step's moments about m are
 *     closed form (alpha = m/sd: Phi(alpha), sd phi(alpha), s_- (Phi(alpha) - alpha phi(alpha)));
 *     the correction int_0^T p(-u) [(-u - m)^k N(-u | m, s_-) - (u - m)^k N(u | m, s_-)] du is
 *     composite 8-node Gauss-Legendre, 8 panels on [0, T_in] and 8 on [T_in, T]. Logit: T_in = 20,
 *     and with c = -m - s_-, T = max(40, c + 8.5 sd) for c > 0, max(40, c + sqrt(c^2 + 72.25 s_-))
 *     otherwise. Probit: T_in = 10, T = 20.
 * Against 30-digit quadrature the rule is within 4e-11 in log Z^, (mu^ error)/sqrt(s^) and
 * (s^ error)/s^ for s_- from 1e-2 to e^10 and |alpha| <= 8. Its covered region is
 *   logit:  s_- <= 5 everywhere; s_- > 5 while -m <= s_- + 7.5 sd + 20 and, where -m < s_-,
 *           alpha >= -30 (together they admit every alpha >= -16.4);
 *   probit: s_- <= 5 while -m sd <= 8 sqrt(2) (1 + s_-); s_- > 5 while -m <= min(5 (1 + s_-), 300).
 * A site outside it fails its chain with APM_STATUS_EP_CAVITY, as a bad tau_- does: the label
 * lies so many cavity deviations on the wrong side that the nodes no longer reach the tilted
 * mass. The clamp of step 5 still removes rounding only (both likelihoods are log-concave).
 * apm_version() is unchanged: a caller detects EP by the presence of these symbols. */
/* on = 1: every later EP fit on the context (apm_ep_eval, apm_ep_predict, apm_ep_grad, the
 * APM_EST_IS_EP theta-calls and what reads their slots) takes its tilted moments by the rule
 * above, under either likelihood, and apm_set_ep and those calls accept an APM_LIK_LOGIT context.
 * on = 0 (the default): the closed-form probit moments and the refusals of the logit, exactly as
 * before the switch existed. Any other value, or a NULL context: APM_E_INVALID. Host state only;
 * nothing else on the context depends on it. */
int apm_set_ep_quadrature(apm_ctx *ctx, int on);
/* the switch (0 or 1); negative on a NULL context */
int apm_ep_quadrature(const apm_ctx *ctx);
/* damping in (0, 1], diff_tol >= 0, max_sweeps >= 1 (APM_E_INVALID otherwise); defaults 0.8,
 * 1e-8, 100 (DESIGN.md §16 has the study they come from) */
int apm_set_ep(apm_ctx *ctx, double damping, double diff_tol, int64_t max_sweeps);
/* The EP fit for `count` thetas (count <= max_batch): Gram -> sweeps (apm_set_ep settings) ->
 * logz[i] and rows i of mu, var (sigma2), tau (tau~), nu (nu~), each count x n with row stride
 * ldo; any of the five may be NULL. status[i]: APM_STATUS_* of chain i (the outputs of a failed
 * chain are NaN); n_sweeps[i] (may be NULL). Needs an ISO or ARD context of any family, not a
 * PRECOMPUTED one. A chain's outputs do not depend on its position in the batch nor on the other
 * chains. Uses the context's work matrix like every theta-call; cache slots and U buffers are
 * not touched. */
int apm_ep_eval(apm_ctx *ctx, int64_t count, const double *thetas, int64_t ldt, double *logz,
                double *mu, double *var, double *tau, double *nu, int64_t ldo, int *status,
                int64_t *n_sweeps);
/* The EP fit, then apm_predict's pass on the final S^1/2, a and L at the m test inputs Xs (m x d,
 * ldxs), in blocks of at most apm_padded_n rows: mean = k*^T a, var = s - |L^-1 (S^1/2 . k*)|^2
 * with s = exp(theta_0), prob = Phi(mean / sqrt(1 + var)) (a logit context: apm_predict's
 * Gauss-Hermite average of sigma); each count x m with row stride ldo,
 * any of the three may be NULL, NaN rows for a failed chain. Nothing is clamped. */
int apm_ep_predict(apm_ctx *ctx, int64_t count, const double *thetas, int64_t ldt,
                   const double *Xs, int64_t m, int64_t ldxs, double *mean, double *var,
                   double *prob, int64_t ldo, int *status, int64_t *n_sweeps);
/* The EP fit (Gram -> sweeps with the apm_set_ep settings), then the gradient of log Z_EP with
 * respect to theta into row i of grad (count x P, row stride ldg >= P = apm_theta_len). With
 * S^1/2, L and a of the sweep the fit stopped at (R&W eq. 5.27 / Alg. 5.2; a is their b):
 *   Z = L^-1 diag(S^1/2), R = Z^T Z = S^1/2 B^-1 S^1/2, M = 1/2 a a^T - 1/2 R,
 *   grad_j = sum_ik M_ik (dK/dtheta_j)_ik,
 * dK/dtheta_j exactly apm_laplace_grad's (dK/dtheta_0 = S WITHOUT epsilon, the G-weighted
 * squared scaled differences for the length scales): apm_laplace_grad's M without its implicit
 * term, because at the EP fixed point the derivative through the sites vanishes. The gradient is
 * therefore only as exact as the fit is converged: at the default diff_tol = 1e-8 it is off by
 * up to a few 1e-4 of max(1, max|grad|), at 1e-16 by a few 1e-8 (DESIGN.md §18 has the table);
 * set a tight diff_tol (and max_sweeps to match) before fitting theta with it.
 * logz[i] (may be NULL) is bitwise the value apm_ep_eval returns for the same theta and
 * settings; status[i] is the fit's (APM_STATUS_CHOL_B, _EP_CAVITY, _MAXITER; a failed chain has
 * NaN logz and a NaN row); n_sweeps[i] (may be NULL). Probit only unless apm_set_ep_quadrature is
 * on (the expression has no likelihood in it), ISO or ARD context of any
 * family, count <= max_batch (APM_E_INVALID otherwise). A chain's outputs do not depend on its
 * position in the batch nor on the other chains. Uses the context's work matrix like every
 * theta-call; cache slots and U buffers are not touched. apm_version() is unchanged: a caller
 * detects this entry point by its symbol. */
int apm_ep_grad(apm_ctx *ctx, int64_t count, const double *thetas, int64_t ldt, double *logz,
                double *grad, int64_t ldg, int *status, int64_t *n_sweeps);
/* ---- joint Laplace / EP predictive at test inputs (no reference counterpart) --
 * The fit of apm_predict (approx = APM_JOINT_LAPLACE) or apm_ep_predict (APM_JOINT_EP) with its
 * settings, statuses and refusals, then for each chain that is OK, at the m test inputs Xs (m x d,
 * ldxs) taken as ONE block, 1 <= m <= apm_padded_n (a joint covariance cannot be split):
 *   mean_j = k*_j^T a                       bitwise apm_predict's / apm_ep_predict's mean
 *   Sigma  = K**(Xs, Xs) - V V^T,  V_j = L^-1 (W^1/2 . k*_j)   (S^1/2 for EP)
 * K** the context's covariance function between the test points with its bias and linear terms and
 * no epsilon (as k* and k** carry none). cov: count blocks of m rows, row stride ldc >= m, both
 * triangles, one the exact mirror of the other; nothing is clamped. mean: count x m, row stride
 * ldo >= m.
 * n_draws > 0: L_S = chol(Sigma + epsilon I) with the context's epsilon (the reference's rule of
 * adding epsilon to one point set's own Gram; cov stays Sigma without it); a factor that fails
 * gives that chain APM_STATUS_CHOL_C. Then
 *   f*_r = mean + L_S xi_r,  r < n_draws,
 * xi_r column r of the m x n_draws matrix that the Philox normal stream of apm_u_normal fills in
 * row-major order from (seeds[i], counters[i]): xi_rj is element j n_draws + r of the stream, so
 * every draw can be reproduced on the host. draws: count x n_draws x m. And with labels ys (m
 * values in {-1, +1}, the same for every chain)
 *   joint_lpd[i] = logsumexp_r sum_j log p(ys_j | f*_rj) - log n_draws
 * under the context's likelihood, in log space throughout: the joint log predictive density of the
 * labels, which does not factorise over the test points.
 * Any of mean, cov, draws and joint_lpd may be NULL; n_draws = 0 asks for neither of the last two
 * (seeds, counters and ys may then be NULL too). The outputs of a chain that is not OK are NaN.
 * n_iter[i] (may be NULL): the fit's Newton iterations or EP sweeps. APM_E_INVALID for another
 * approx, a PRECOMPUTED context, APM_JOINT_EP on an APM_LIK_LOGIT context without
 * apm_set_ep_quadrature, count > max_batch, m outside [1, apm_padded_n], n_draws outside [0,
 * APM_JOINT_MAX_DRAWS], and draws or joint_lpd asked for with n_draws = 0. A chain's outputs do
 * not depend on its position in the batch nor on the other chains. Uses the context's work matrix
 * like every theta-call; cache slots and U buffers are not touched. The first call that draws
 * allocates device scratch that grows with the largest n_draws asked for so far and is kept for
 * the context's lifetime: max_batch x 64 ceil(n_draws / 64) x apm_padded_n doubles for the normals
 * and as many again at the first call that wants the draws back (about 1 GiB each at max_batch
 * 8, apm_padded_n 4096 and 4096 draws). apm_version() is unchanged: a caller detects this entry
 * point by its symbol. */
#define APM_JOINT_LAPLACE 0
#define APM_JOINT_EP 1
#define APM_JOINT_MAX_DRAWS 4096
int apm_predict_joint(apm_ctx *ctx, int approx, int64_t count, const double *thetas, int64_t ldt,
                      const double *Xs, int64_t m, int64_t ldxs,
                      double *mean, int64_t ldo,            /* count x m, may be NULL */
                      double *cov, int64_t ldc,             /* count blocks of m x ldc, may be NULL */
                      int64_t n_draws, const uint64_t *seeds, const uint64_t *counters,
                      double *draws,                        /* count x n_draws x m, may be NULL */
                      const double *ys, double *joint_lpd,  /* m labels in {-1,+1}; count; may be NULL */
                      int *status, int64_t *n_iter);
/* cached u-call: reuse slots[i]'s per-theta state with draws ubufs[i]; out_logf[i] is NaN where
 * status[i] != 0 or the slot's last theta-call failed (such a slot holds no state) */
int apm_u_eval(apm_ctx *ctx, int64_t count, const int64_t *slots, const int64_t *ubufs,
               double *out_logf, int *status);
/* ---- replicate spread and weight diagnostics of the IS estimate (no reference counterpart;
 * DESIGN.md §20) -------------------------------------------------------------------------------
 * For one chain, with slot state and a U buffer of S = n_imp real columns, log w_s is the summand
 * of the estimate exactly as apm_u_eval forms it. For a block length 1 <= block <= n_imp the
 * samples are cut into nblk = floor(n_imp / block) blocks, block j being samples [j block,
 * (j + 1) block); leftover samples are ignored. Per block:
 *   logf_j = logsumexp_{s in j} log w_s - log(block)     (an estimate from `block` samples)
 *   ess_j  = (sum w)^2 / sum w^2,  wmax_j = max w / sum w (w = exp(log w_s - block maximum))
 * and, where the block maximum is not finite, logf_j = max - log(block), ess_j = wmax_j = 0. With
 * block = n_imp, logf_0 is bitwise apm_u_eval's value. A chain's outputs do not depend on its
 * position in the batch nor on the other chains. APM_E_INVALID, with nothing written, for block < 1
 * or > n_imp, n_rep < 1, n_rep nblk > APM_SPREAD_MAX_BLOCKS, ldo < n_rep nblk, count outside [1,
 * max_batch], null slots / ubufs / status (apm_is_spread: seeds / counters) and indices out of
 * range. Any of logf, ess, wmax may be NULL. A chain whose slot's last theta-call failed (status
 * != 0 there: the slot was not written, or its value is withheld) gets apm_u_eval's status and NaN
 * in all three outputs. Works for slots written by APM_EST_IS, APM_EST_IS_EP and APM_EST_PRIORMC
 * under both likelihoods. apm_version() is unchanged: detect the entry points by their symbols. */
#define APM_SPREAD_MAX_BLOCKS 4096
/* apm_u_eval (the same checks, launches and status) followed by the block reduction: nblk values
 * per chain into row i of logf / ess / wmax (row stride ldo). Slots and U buffers are only read. */
int apm_u_eval_diag(apm_ctx *ctx, int64_t count, const int64_t *slots, const int64_t *ubufs,
                    int64_t block, double *logf, double *ess, double *wmax, int64_t ldo,
                    int *status);
/* n_rep independent replicates of the estimate at fixed slot state: for r = 0 .. n_rep - 1 U
 * buffer ubufs[i] is redrawn as apm_u_normal(seeds[i], counters[i] + r) draws it and the u-path
 * and the block reduction run on it; replicate r's block j goes to [i ldo + r nblk + j]. All
 * replicates are enqueued without a host synchronisation; one read-back ends the call. ubufs[i] is
 * scratch: at return it holds the last replicate's draws. The slots are only read. */
int apm_is_spread(apm_ctx *ctx, int64_t count, const int64_t *slots, const int64_t *ubufs,
                  const uint64_t *seeds, const uint64_t *counters, int64_t n_rep, int64_t block,
                  double *logf, double *ess, double *wmax, int64_t ldo, int *status);
/* ---- leave-one-out predictive densities from the IS samples (no reference counterpart;
 * DESIGN.md §23) -------------------------------------------------------------------------------
 * For one chain, with slot state (f_post, W, z = C^-1 f_post, the factor C_chol and its squared row
 * norms C_ii) and a U buffer of S = n_imp real columns: f_si = f_post_i + (C_chol U)_is are the
 * importance samples, wbar_s their self-normalised weights (log w_s the summand of the estimate
 * exactly as apm_u_eval forms it; padded columns weigh exactly 0) and p_si = p(y_i | f_si) the
 * context's likelihood, the same function of the same f_si as in the weights. Per training point
 * i < n:
 *   loo_i     = -log sum_s wbar_s / p_si     (log p(y_i | y_-i): 1 / E[1 / p(y_i | f_i) | y])
 *   lpd_i     =  log sum_s wbar_s p_si       (the in-sample density; lpd_i >= loo_i)
 *   ess_loo_i = (sum_s rho_si)^2 / sum_s rho_si^2, rho_si = wbar_s / p_si   (in [1, n_imp])
 *   gauss_i   = log int p(y_i | f) N(f | nu / tau, 1 / tau) df,
 *               tau = 1 / C_ii - W_i, nu = f_post_i / C_ii - z_i
 * and per chain ess = 1 / sum_s wbar_s^2. gauss is the Gaussian (cavity) leave-one-out density of
 * the slot's N(f_post, C) with site i removed (EP's own cavity for an APM_EST_IS_EP slot; probit:
 * log Phi(y_i m / sqrt(1 + v)), logit: the log of the Gauss-Hermite average of apm_predict); a
 * computed tau <= 0 gives NaN for that point's gauss only. All sums over s are formed in log
 * space. Averaged over the states (theta, u) of a pseudo-marginal chain, exp(-loo_i) and
 * exp(lpd_i) estimate E[1 / p(y_i | f_i) | y] and E[p(y_i | f_i) | y]: no Gaussian approximation
 * of p(f | theta, y) is left in them.
 * apm_u_eval (the same checks, launches and status: out_logf is bitwise its value) followed by
 * the tail; chain i's rows are at [i ldo], n values each. Any output pointer except status may be
 * NULL. APM_E_INVALID, with nothing written, for count outside [1, max_batch], null slots / ubufs
 * / status, indices out of range and ldo < n with any row output non-NULL. A chain whose slot's
 * last theta-call failed gets apm_u_eval's status and NaN in every output. Works for slots written
 * by APM_EST_IS, APM_EST_IS_EP and APM_EST_PRIORMC (W = z = 0: loo is the prior-proposal
 * estimate, gauss the prior predictive) under both likelihoods. A chain's outputs do not depend on
 * its position in the batch nor on the other chains. Slots and U buffers are only read.
 * apm_version() is unchanged: detect the entry point by its symbol. */
int apm_is_loo(apm_ctx *ctx, int64_t count, const int64_t *slots, const int64_t *ubufs,
               double *out_logf, double *loo, double *lpd, double *ess_loo, double *gauss,
               int64_t ldo, double *ess, int *status);
/* ---- Pareto-smoothed leave-one-out densities and the Pareto k-hat of the importance ratios (PSIS:
 * Vehtari, Simpson, Gelman, Yao, Gabry; no reference counterpart) -----------------
 * ess_loo_i is blind to a ratio whose variance is infinite; the shape k-hat of the ratios' upper
 * tail is not. Per chain and per training point i < n, with t_s = log wbar_s - log p(y_i | f_si),
 * exactly apm_is_loo's t. Padded columns, and real columns whose log wbar_s = -inf, have no t; S'
 * is the number of finite t_s.
 *  1. M = min(floor(0.2 S'), ceil(3 sqrt(S'))) and mx = max_s t_s; work with t_s - mx, sorted
 *     ascending t_(1) <= .. <= t_(S').
 *  2. If M < 5: khat_i = NaN and loo_psis_i = -(mx + log sum_s e^(t_s - mx)), the raw value.
 *  3. cut = max(t_(S'-M), log DBL_MIN), e_c = e^cut, x_z = e^(t_(S'-M+z)) - e_c for z = 1..M,
 *     ascending. If x_1 <= 0 or x_M <= x_1: the same fallback as in 2.
 *  4. The generalised-Pareto fit of Zhang & Stephens (2009) with the `loo` package's priors:
 *     m = 30 + floor(sqrt(M)), q = x_(floor(M/4 + 0.5)) (1-based); for j = 1..m
 *       b_j = 1 / x_M + (1 - sqrt(m / (j - 0.5))) / (3 q),  k_j = (1/M) sum_z log1p(-b_j x_z),
 *       L_j = M (log(-b_j / k_j) - k_j - 1),  omega_j = 1 / sum_l e^(L_l - L_j);
 *     b = sum_j b_j omega_j, k = (1/M) sum_z log1p(-b x_z), sigma = -k / b and
 *     khat = (M k + 5) / (M + 10) (prior_k = 10 pulling towards 0.5). A non-finite khat or sigma
 *     gives the fallback, with khat_i as computed.
 *  5. p_z = (z - 0.5) / M, q_z = sigma expm1(-khat log1p(-p_z)) / khat (-sigma log1p(-p_z) when
 *     khat == 0), r_z = min(q_z + e_c, 1): the cap is truncation at the largest raw ratio.
 *  6. loo_psis_i = -(mx + log(sum_{z <= S'-M} e^(t_(z)) + sum_z r_z)). Only the sum is needed, so
 *     no rank-to-sample map is formed and ties cannot matter.
 * loo_psis keeps the form -log sum_s r_si, so it drops into the same average over a chain's states
 * as loo (1 / E[1 / p]). Per chain, steps 1-4 on the row log wbar_s give khat_w, the tail shape of
 * the importance weights: a diagnostic only (the pseudo-marginal estimate itself is never
 * smoothed, which would bias it). k-hat above 0.7 marks a value not to be trusted.
 * apm_u_eval (the same checks, launches and status: out_logf is bitwise its value) followed by
 * the tail; chain i's rows loo_psis and khat are at [i ldo], n values each, khat_w has count
 * entries. logratio, if given, receives the t_si themselves, chain i's at [i ldr + r n_imp + s] for
 * row r < n and the real columns s < n_imp (ldr >= n n_imp), for a caller who pools states and
 * smooths offline. Any output pointer except status may be NULL. APM_E_INVALID, with nothing
 * written, for apm_is_loo's own conditions, for n_imp > APM_PSIS_MAX_SAMPLES and for
 * ldr < n n_imp with logratio non-NULL. A chain whose slot's last theta-call failed gets
 * apm_u_eval's status and NaN in every output. Works for slots written by APM_EST_IS,
 * APM_EST_IS_EP and APM_EST_PRIORMC under both likelihoods. A chain's outputs do not depend on its
 * position in the batch nor on the other chains. Slots and U buffers are only read; apm_is_loo's
 * results are not disturbed. apm_version() is unchanged: detect the entry point by its symbol. */
#define APM_PSIS_MAX_SAMPLES 4096
int apm_is_loo_psis(apm_ctx *ctx, int64_t count, const int64_t *slots, const int64_t *ubufs,
                    double *out_logf, double *loo_psis, double *khat, int64_t ldo,
                    double *khat_w, double *logratio, int64_t ldr, int *status);
/* cache-slot lifetimes (samplers.py:563-584: an MH sampler keeps the current state's cache and the
 * proposal's alive at once). acquire: a free slot, one owner (APM_E_NOMEM when all are owned);
 * copy: one more owner of the same (immutable) state - the handle copy of the reference's tuple;
 * release: one owner fewer, the slot is free again at zero (APM_E_INVALID if not acquired);
 * refcount: owners of a slot (negative on a bad argument). Host bookkeeping, no device work.
 * apm_theta_eval / apm_u_eval take any slot index; the Python layer allocates through these. */
int apm_cache_acquire(apm_ctx *ctx, int64_t *slot);
int apm_cache_copy(apm_ctx *ctx, int64_t slot);
int apm_cache_release(apm_ctx *ctx, int64_t slot);
int64_t apm_cache_refcount(const apm_ctx *ctx, int64_t slot);
/* read a slot back (any pointer may be NULL): factor (n x n lower, fp32 rounded), f_post, g, cst */
int apm_slot_read(apm_ctx *ctx, int64_t slot, double *L, int64_t ldl, double *f_post, double *g,
                  double *cst);

/* ---- stand-alone building blocks (host in / host out) ---------------------------------------- */
int apm_gram(int device, int kernel_kind, const double *X, int64_t n, int64_t d, int64_t ldx,
             const double *theta, int64_t n_theta, double epsilon, double *K, int64_t ldk);
/* stand-alone building block, as apm_gram: Ks (m x n, ldk) = k(Xs_i, X_j), no epsilon (both
 * point sets with row stride ldx) */
int apm_gram_cross(int device, int kernel_kind, const double *Xs, int64_t m, const double *X,
                   int64_t n, int64_t d, int64_t ldx, const double *theta, int64_t n_theta,
                   double *Ks, int64_t ldk);
/* laplace_approximation(K, y, calc_cov, calc_lml, diff_f_tol, max_iters): f_out (n), C_out
 * (n x n, ldc; if calc_cov), lml_out (if calc_lml), n_iter_out = Newton iterations */
int apm_laplace(int device, const double *K, int64_t n, int64_t ldk, const double *y,
                int calc_cov, int calc_lml, double diff_f_tol, int64_t max_iters, double *f_out,
                double *C_out, int64_t ldc, double *lml_out, int64_t *n_iter_out, int *status);
/* the same under likelihood lik (APM_LIK_*); apm_laplace is apm_laplace_lik(APM_LIK_PROBIT) */
int apm_laplace_lik(int device, int lik, const double *K, int64_t n, int64_t ldk, const double *y,
                    int calc_cov, int calc_lml, double diff_f_tol, int64_t max_iters,
                    double *f_out, double *C_out, int64_t ldc, double *lml_out,
                    int64_t *n_iter_out, int *status);

/* EP's stand-alone twin of apm_laplace (no reference counterpart): the caller supplies K (n x n,
 * ldk) and the settings; mu_out, var_out, tau_out, nu_out (n each), logz_out and n_sweeps_out
 * may be NULL; calc_cov: C_out (n x n, ldc) = K - V^T V, the posterior covariance, formed as
 * apm_laplace's. Probit, by the closed-form moments. On a failed fit (*status != 0) the outputs
 * are NaN and C_out is left alone. */
int apm_ep(int device, const double *K, int64_t n, int64_t ldk, const double *y, int calc_cov,
           double damping, double diff_tol, int64_t max_sweeps, double *mu_out, double *var_out,
           double *tau_out, double *nu_out, double *C_out, int64_t ldc, double *logz_out,
           int64_t *n_sweeps_out, int *status);
/* the same under likelihood lik (APM_LIK_*); apm_ep is apm_ep_lik(APM_LIK_PROBIT). The probit
 * takes the closed-form moments, the logit the quadrature rule of apm_set_ep_quadrature. */
int apm_ep_lik(int device, int lik, const double *K, int64_t n, int64_t ldk, const double *y,
               int calc_cov, double damping, double diff_tol, int64_t max_sweeps, double *mu_out,
               double *var_out, double *tau_out, double *nu_out, double *C_out, int64_t ldc,
               double *logz_out, int64_t *n_sweeps_out, int *status);

/* ---- device-time accounting of the hot kernels (HIP events on the context stream) ------------ */
#define APM_PROF_GRAM 0
#define APM_PROF_CHOL_UPDATE 1
#define APM_PROF_UGEMM 2
#define APM_PROF_CHOL_UPDATE32 3
#define APM_PROF_STATS 4 /* not a kernel: launches = chains whose mixed-precision Newton solve was
                            rerun in fp64, work = refinement steps launched, total_ms = 0 */
#define APM_PROF_CHOL_UPDATE32_OUTER 5 /* the rank-64*OUTER launches among CHOL_UPDATE32 */
#define APM_PROF_CHOL_UPDATE_OUTER 6   /* the rank-64*OUTER launches among CHOL_UPDATE */
#define APM_PROF_DF_TIMEOUTS 7 /* not a kernel: launches = bounded-spin timeouts of the Newton
                                 factorisation's dataflow panel launches (each fails its chain,
                                 which the Newton loop reruns in fp64; apart from breakdowns of
                                 the fp32 factor, which are not counted here) */
#define APM_PROF_POST32_OUTER 8 /* the rank-64*OUTER trailing updates of the posterior factor's
                                   bottom block in fp32 (postcov.hip, APM_POST32) */
#define APM_PROF_POST64_RERUNS 9 /* not a kernel: launches = chains whose posterior bottom block was
                                    recomputed in fp64 (trace of C above the fp32 bound) */
#define APM_PROF_TRSV_TIMEOUTS 10 /* not a kernel: launches = bounded-spin timeouts of the Newton
                                    solves' multi-workgroup TRSV (each fails its chain, which the
                                    Newton loop reruns in fp64) */
#define APM_PROF_ICM_CHECKS 11 /* not a kernel: launches = chains whose chol(C) was also formed the
                                 reference's way (the InvalidCovarianceMatrixError check) */
#define APM_PROF_GUARD 12 /* not a kernel: launches = chains failed by the guard (APM_STATUS_GUARD) */
#define APM_PROF_GRAD_REDUCE 13 /* k_grad_reduce of apm_laplace_grad and apm_ep_grad; work = bytes
                                   (the lower triangles of R and K it reads) */
#define APM_PROF_EP_SITES 14 /* k_ep_sites of the EP sweeps; work = bytes (the solved rows of V^T
                                it reads) */
#define APM_PROF_NKINDS 15
/* on = 0 off; 1 the roofline kinds (GRAM, UGEMM and the two *_OUTER kinds: one event pair per
 * launch of those kernels only, so that the timing adds little to a timed region); 2 every kind
 * (CHOL_UPDATE / CHOL_UPDATE32 add an event pair around every in-panel update launch) */
int apm_prof_enable(apm_ctx *ctx, int on);
/* total device milliseconds and launch count per tracked kernel since the last reset; also the
 * algorithmic work: bytes (GRAM) or flops (CHOL_UPDATE, CHOL_UPDATE32 = the fp32 Newton
 * factorisation, UGEMM) those launches performed */
int apm_prof_read(apm_ctx *ctx, int kind, double *total_ms, int64_t *launches, double *work,
                  int reset);
/* launches the empty kernel k_apm_marker<id> (id 0..3) on the context stream: brackets a region
 * in a rocprofv3 kernel trace (tools/prof_window.py); no reference counterpart */
int apm_prof_marker(apm_ctx *ctx, int id);

/* The guard of the last IS theta-call: per chain i < count, r[4i..4i+3] =
 * |1/2 log|B| of the last Newton factor - 1/2 log|M| of the posterior factor| (the same
 * eigenvalues), | |g|^2 - f_post^T z | / max(1, |f_post^T z|) (g = chol(C)^-1 f_post from the
 * posterior factors, z = a + W f_post from the Newton vectors), |sum log diag chol(C) -
 * (1/2 log|K| - 1/2 log|M|)| (C_chol's diagonal from the slot) and max_r |(C_chol g)_r -
 * f_post_r| / max(1, max |f_post|) (every row of the slot's fp32 factor). A chain past a bound
 * fails with APM_STATUS_GUARD. */
int apm_guard_read(apm_ctx *ctx, int64_t count, double *r);

/* ---- self-test ------------------------------------------------------------------------------- */
/* C = C + A * B^T for 64x64 row-major fp64 host matrices through the f64 MFMA tile routine that
 * every Cholesky panel / trailing update uses (pins the v_mfma_f64_16x16x4 operand maps) */
int apm_selftest_tile(int device, const double *A, const double *B, double *C);
/* out[4i..4i+3] = Philox4x32-10(counter in[6i..6i+3], key in[6i+4..6i+5]) for i < n, through
 * the device round function of apm_u_normal (Salmon et al., SC'11; checked against the
 * published known-answer vectors in tests/test_gpu_kernels.py) */
int apm_selftest_philox(int device, int64_t n, const uint32_t *in, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* APM_H */
