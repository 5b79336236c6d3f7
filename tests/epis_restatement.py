"""float64 numpy/scipy restatement of the importance-sampling estimator with the EP posterior as
its importance distribution (APM_EST_IS_EP), shared by test_epis_host.py and
test_gpu_epis.py. A plain module. The state is ep_restatement.ep_fit's converged sweep put into
the slots of the consistent form of DESIGN.md §3.2: f_post = mu, W = tau~, a (so that
z = a + W f_post = nu~) and log|B| of B = I + S^1/2 K S^1/2."""
import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr, logsumexp

import ep_restatement as ep


def state(K, y, **ep_settings):
    """The EP fit and chol(C) of C = (K^-1 + diag tau~)^-1 = L_K M^-1 L_K^T with
    M = I + L_K^T diag(tau~) L_K = U U^T: the push-through route of logit_restatement.is_state with
    W = tau~."""
    fit = ep.ep_fit(K, y, **ep_settings)
    Lk = la.cholesky(K, lower=True)
    M = np.eye(K.shape[0]) + (Lk.T * fit['tau'][None]).dot(Lk)
    Lp = la.cholesky(M[::-1, ::-1], lower=True)
    U = Lp[::-1, ::-1]
    C_chol = la.solve_triangular(U, Lk.T, lower=False).T
    return dict(fit, f=fit['mu'], W=fit['tau'], Ws=fit['s'], K_chol=Lk, C_chol=C_chol,
                logdet_B=2.0 * np.log(fit['L'].diagonal()).sum())


def cst(st):
    """1/2 mu^T nu~ - 1/2 log|B|: the constant a cache slot keeps."""
    return 0.5 * st['mu'].dot(st['nu']) - 0.5 * st['logdet_B']


def is_consistent(y, st, ns):
    """log w_s = sum_n [log Phi(y_n f_sn) + 1/2 W_n f_sn^2 - z_n f_sn] + 1/2 f_post^T z - 1/2 log|B|
    with z = a + W f_post (include/apm.h), f_s = f_post + C_chol u_s, log-mean-exp over the
    samples. Takes any state with f, W, a, C_chol and logdet_B: the EP one or a Laplace one."""
    f_post, W = st['f'], st['W']
    z = st['a'] + W * f_post
    f_s = f_post[:, None] + st['C_chol'].dot(ns)
    t = log_ndtr(y[:, None] * f_s) + (0.5 * W[:, None] * f_s - z[:, None]) * f_s
    lw = t.sum(0) + 0.5 * f_post.dot(z) - 0.5 * st['logdet_B']
    return logsumexp(lw) - np.log(ns.shape[1])


def is_direct(K, y, st, ns):
    """The reference's form (estimators.py:221-241): log p(y|f) + log N(f|0, K) - log N(f|mu, Sigma)
    at f_s = mu + chol(Sigma) u_s with Sigma = K - V^T V, V = L^-1 S^1/2 K (the 2 pi terms
    cancel)."""
    V = la.solve_triangular(st['L'], st['s'][:, None] * K, lower=True)
    S_chol = la.cholesky(K - V.T.dot(V), lower=True)
    f_s = st['mu'][None] + S_chol.dot(ns).T
    q_K = (la.cho_solve((st['K_chol'], True), f_s.T) * f_s.T).sum(0)
    log_p_f = -0.5 * q_K - np.log(st['K_chol'].diagonal()).sum()
    f_zm = f_s - st['mu'][None]
    q_S = (la.cho_solve((S_chol, True), f_zm.T) * f_zm.T).sum(0)
    log_q = -0.5 * q_S - np.log(S_chol.diagonal()).sum()
    lw = log_ndtr(f_s * y[None]).sum(-1) + log_p_f - log_q
    return logsumexp(lw) - np.log(ns.shape[1])


def laplace_state(K, y):
    """The probit Laplace state of the oracle in the keys is_consistent reads."""
    import apm_oracle as orc
    st = orc.theta_state_pushthrough(K, y)
    return dict(f=st['f_post'], W=st['W'], a=st['a'], C_chol=st['C_chol'],
                logdet_B=st['logdet_B'])
