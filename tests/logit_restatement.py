"""float64 numpy/scipy restatement of the logistic likelihood's paths, shared by
test_logit_host.py and test_gpu_logit.py. A plain module. The oracle is probit-only, so this is
the logit's yardstick: grad_restatement's Newton loop (latent_posterior_approximations.py:85-99)
with the logit's grad / W (same f0 = 0, same stopping rule, W / L / a of the LAST iteration kept
beside the updated f), the LML, the consistent importance-sampling form of DESIGN.md §3.2 and PriorMC, the
predictive with pi* from a 400-node Gauss-Hermite rule, and grad_restatement's gradient formula
with the logit's g and d3. K and k* come from the caller (cov_restatement).

With t = y f, sigma(u) = 1/(1 + e^-u):
    log p = log sigma(t),  grad = y sigma(-t),  W = sigma(t) sigma(-t),
    d3 = d^3 log p / df^3 = -y W (1 - 2 sigma(t))
"""
import numpy as np
import scipy.linalg as la
from scipy.special import expit, logsumexp, roots_hermite

import grad_restatement as gr

GH_NODES = 400
# the grid the committed table is pinned on (test_logit_host) and its bound
GH_BOUND = 1e-7


def log_lik(t):
    """log sigma(t): -log1p(e^-t) for t >= 0, t - log1p(e^t) for t < 0."""
    t = np.asarray(t, dtype=np.float64)
    return np.where(t >= 0, -np.log1p(np.exp(-np.abs(t))), t - np.log1p(np.exp(-np.abs(t))))


def grad_W(f, y):
    t = y * f
    sm = expit(-t)
    return y * sm, expit(t) * sm


def d3(f, y):
    t = y * f
    sp, sm = expit(t), expit(-t)
    return -y * (sp * sm) * (sm - sp)  # (sm - sp = 1 - 2 sigma(t))


LOGIT = gr.Likelihood(log_lik, grad_W, d3)


def newton(K, y, tol=1e-4, max_iters=1000):
    """grad_restatement's Newton loop with the logit's grad / W and log p."""
    return gr.newton(K, y, tol, max_iters, LOGIT)


def lml(K, y, tol=1e-24):
    return newton(K, y, tol)['lml']


def covariance(K, nw):
    """C = K - V^T V, V = L^-1 W^1/2 K (lpa.py:107-112)."""
    V = la.solve_triangular(nw['L'], nw['Ws'][:, None] * K, lower=True)
    return K - V.T.dot(V)


def is_state(K, y, tol=1e-4):
    """Per-theta state of the consistent form: the Newton quantities and chol(C) with
    C = (K^-1 + W)^-1 = L_K M^-1 L_K^T, M = I + L_K^T W L_K = U U^T (the device's route,
    apm_oracle.theta_state_pushthrough)."""
    nw = newton(K, y, tol)
    Lk = la.cholesky(K, lower=True)
    M = np.eye(K.shape[0]) + (Lk.T * nw['W'][None]).dot(Lk)
    Lp = la.cholesky(M[::-1, ::-1], lower=True)
    U = Lp[::-1, ::-1]
    C_chol = la.solve_triangular(U, Lk.T, lower=False).T
    return dict(nw, K_chol=Lk, C_chol=C_chol, logdet_B=2.0 * np.log(nw['L'].diagonal()).sum())


def is_consistent(y, st, ns, C_chol=None):
    """log w_s = sum_n [log p(y_n|f_sn) + 1/2 W_n f_sn^2 - z_n f_sn] + 1/2 f_post^T z - 1/2 log|B|,
    z = a + W f_post, log-mean-exp over the samples."""
    L = st['C_chol'] if C_chol is None else C_chol
    f_post, W = st['f'], st['W']
    z = st['a'] + W * f_post
    f_s = f_post[:, None] + L.dot(ns)
    t = log_lik(y[:, None] * f_s) + (0.5 * W[:, None] * f_s - z[:, None]) * f_s
    lw = t.sum(0) + 0.5 * f_post.dot(z) - 0.5 * st['logdet_B']
    return logsumexp(lw) - np.log(ns.shape[1])


def is_direct(K, y, st, ns):
    """The reference's form (estimators.py:221-241) with the logit: log p(y|f) + log N(f|0, K)
    - log N(f|f_post, C) at f_s = f_post + chol(C) u_s, C = K - V^T V (the 2 pi terms cancel)."""
    C_chol = la.cholesky(covariance(K, st), lower=True)
    f_s = st['f'][None] + C_chol.dot(ns).T
    q_K = (la.cho_solve((st['K_chol'], True), f_s.T) * f_s.T).sum(0)
    log_p_f = -0.5 * q_K - np.log(st['K_chol'].diagonal()).sum()
    f_zm = f_s - st['f'][None]
    q_C = (la.cho_solve((C_chol, True), f_zm.T) * f_zm.T).sum(0)
    log_q = -0.5 * q_C - np.log(C_chol.diagonal()).sum()
    lw = log_lik(f_s * y[None]).sum(-1) + log_p_f - log_q
    return logsumexp(lw) - np.log(ns.shape[1]), C_chol


def priormc(K, y, ns):
    f_s = la.cholesky(K, lower=True).dot(ns)
    return logsumexp(log_lik(y[:, None] * f_s).sum(0)) - np.log(ns.shape[1])


_RULES = {}


def gauss_hermite(q=GH_NODES):
    """Nodes and weights / sqrt(pi) of the q-node rule (scipy: numpy's hermgauss overflows to NaN
    weights at 400 nodes)."""
    if q not in _RULES:
        x, w = roots_hermite(q)
        _RULES[q] = (x, w / np.sqrt(np.pi))
    return _RULES[q]


def logistic_normal(mu, var, q=GH_NODES):
    """int sigma(x) N(x | mu, var) dx by the q-node rule, elementwise."""
    x, w = gauss_hermite(q)
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    return (expit(mu[..., None] + np.sqrt(2.0 * var)[..., None] * x) * w).sum(-1)


def predictive(K, Ks, y, sigma, tol=1e-4, max_iters=1000):
    """mean = Ks a, var = sigma - |L^-1 (W^1/2 . ks)|^2 from the last iteration's W, L, a, and
    prob by the 400-node rule."""
    nw = newton(K, y, tol, max_iters)
    mu = Ks.dot(nw['a'])
    V = la.solve_triangular(nw['L'], (Ks * nw['Ws'][None, :]).T, lower=True)
    var = sigma - (V * V).sum(0)
    return dict(n_iter=nw['n_iter'], f=nw['f'], a=nw['a'], diffs=nw['diffs'], mean=mu, var=var,
                prob=logistic_normal(mu, var))


def laplace_grad(K, dKs, y, tol=1e-14, max_iters=1000):
    """dict(lml, grad (P,), n_iter, diffs, f): grad_restatement.laplace_grad's algebra with the
    logit's g and d3; dKs the P matrices dK/dtheta_j (cov_restatement's Cov.dK)."""
    return gr.laplace_grad(K, dKs, y, tol, max_iters, LOGIT)


central_differences = gr.central_differences


def committed_table():
    """(x, w) of auxiliary-pm-mcmc_amd/csrc/gh_table.h, the literals k_predict_reduce sums."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    txt = open(os.path.join(here, '..', 'auxiliary-pm-mcmc_amd', 'csrc', 'gh_table.h')).read()
    out = []
    for name in ('APM_GH_X', 'APM_GH_W'):
        body = re.search(name + r'\[APM_GH_PAIRS\] = \{(.*?)\};', txt, re.S).group(1)
        out.append(np.array([float(t) for t in body.replace('\n', ' ').split(',') if t.strip()]))
    pairs = int(re.search(r'#define APM_GH_PAIRS (\d+)', txt).group(1))
    assert out[0].shape == out[1].shape == (pairs,)
    return out[0], out[1]


def table_average(mu, var, x, w):
    """k_predict_reduce<LOGIT>'s arithmetic on the table's pairs +-x_q (numpy's sum order):
    mu < 0: sum w [sigma(mu + a) + sigma(mu - a)]; mu >= 0: 1/2 + sum w [sigma(mu + a) -
    sigma(a - mu)]; a = sqrt(2 var) x, var <= 0 -> a = 0."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    a = np.sqrt(2.0 * np.maximum(var, 0.0))[..., None] * x
    m = mu[..., None]
    lo = (w * (expit(m + a) + expit(m - a))).sum(-1)
    hi = 0.5 + (w * (expit(m + a) - expit(a - m))).sum(-1)
    return np.where(mu < 0, lo, hi)
