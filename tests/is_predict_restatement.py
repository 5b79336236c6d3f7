"""numpy statement of the importance-sampling predictive at test inputs (DESIGN.md §19;
apm_is_predict), shared by test_is_predict_host.py and test_gpu_is_predict.py. A plain module.

Inputs: K (n x n, with epsilon), Ks (m x n, k* without epsilon), s = exp(theta_0), the labels y,
the draws U (n x S), the likelihood and the proposal fit: a dict with f (f_post), W, a = K^-1 f_post
and logdet_B, as epis_restatement.laplace_state / .state and logit_restatement.is_state return
them (the fits themselves and the Gauss-Hermite rule are those modules')."""
import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr, ndtr

import logit_restatement as lr


def _chol(A):
    """Lower Cholesky factor in A's own dtype (scipy has no long double)."""
    if A.dtype == np.float64:
        return la.cholesky(A, lower=True)
    n = A.shape[0]
    L = np.tril(A).astype(A.dtype)
    for j in range(n):
        L[j:, j] -= L[j:, :j].dot(L[j, :j])
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return L


def _solve_lower(L, B):
    """L^-1 B in L's dtype."""
    if L.dtype == np.float64:
        return la.solve_triangular(L, B, lower=True)
    X = np.array(B, dtype=L.dtype)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i].dot(X[:i])) / L[i, i]
    return X


def h_route(K, Ks, s, W, a, U, dtype=np.float64):
    """c_j = k*_j . a, v*_j = s - |p_j|^2 with p_j = L_K^-1 k*_j, and m_sj = c_j + h_j^T u_s with
    J h_j = L'^-1 J p_j, L' = chol(J M J), M = I + L_K^T W L_K: dict(c (m,), vstar (m,), m (m, S)),
    every operation in `dtype` (float64, or numpy.longdouble for the rounding yardstick)."""
    K, Ks, W, a, U = (np.asarray(x, dtype=dtype) for x in (K, Ks, W, a, U))
    Lk = _chol(K)
    P = _solve_lower(Lk, Ks.T)                                   # (n, m): the p_j as columns
    vstar = dtype(s) - (P * P).sum(0)
    M = np.eye(K.shape[0], dtype=dtype) + (Lk.T * W[None]).dot(Lk)
    Lp = _chol(np.ascontiguousarray(M[::-1, ::-1]))
    Hrev = _solve_lower(Lp, np.ascontiguousarray(P[::-1]))       # J h_j as columns
    c = Ks.dot(a)
    return dict(c=c, vstar=vstar, m=c[:, None] + Hrev.T.dot(U[::-1]), Lk=Lk, Lp=Lp)


def naive_route(K, Ks, f_s):
    """m_sj = k*_j^T K^-1 f_s on given samples f_s (n, S): the route the device does NOT take."""
    return Ks.dot(la.cho_solve((la.cholesky(K, lower=True), True), f_s))


def samples(hr, f_post, U):
    """f_s = f_post + C_chol u_s with chol(C) = L_K U_M^-T, U_M = J L' J (n, S)."""
    Um = hr['Lp'][::-1, ::-1]
    C_chol = la.solve_triangular(Um, hr['Lk'].T, lower=False).T
    return f_post[:, None] + C_chol.dot(U)


def log_weights(y, fit, f_s, likelihood='probit'):
    """log w_s of DESIGN.md §3.2 at the samples f_s (n, S)."""
    f_post, W = fit['f'], fit['W']
    z = fit['a'] + W * f_post
    ll = lr.log_lik if likelihood == 'logit' else log_ndtr
    t = ll(y[:, None] * f_s) + (0.5 * W[:, None] * f_s - z[:, None]) * f_s
    return t.sum(0) + 0.5 * f_post.dot(z) - 0.5 * fit['logdet_B']


def link(m, vstar, likelihood='probit'):
    """p(y* = 1 | f_s): Phi(m / sqrt(1 + v*)) or the 400-node Gauss-Hermite average of sigma."""
    v = np.broadcast_to(np.asarray(vstar)[:, None], m.shape)
    if likelihood == 'logit':
        return lr.logistic_normal(m, np.maximum(v, 0.0))
    return ndtr(m / np.sqrt(1.0 + v))


def predictive(K, Ks, s, y, U, fit, likelihood='probit', n_real=None):
    """dict(prob, mean, var (m,), ess, logf, wbar (S,), m (m, S), c, vstar, lw): the section
    'Mathematics' of the feature. The first n_real columns of U (default: all) are the real
    samples; the others are padding and weigh exactly 0."""
    S = U.shape[1] if n_real is None else int(n_real)
    hr = h_route(K, Ks, s, fit['W'], fit['a'], U)
    lw = log_weights(y, fit, samples(hr, fit['f'], U), likelihood)
    e = np.where(np.arange(U.shape[1]) < S, np.exp(lw - lw[:S].max()), 0.0)
    wbar = e / e.sum()
    m = hr['m']
    mean = m.dot(wbar)
    return dict(prob=link(m, hr['vstar'], likelihood).dot(wbar), mean=mean,
                var=hr['vstar'] + (m * m).dot(wbar) - mean ** 2, ess=1.0 / (wbar ** 2).sum(),
                logf=lw[:S].max() + np.log(e.sum()) - np.log(S), wbar=wbar, m=m, c=hr['c'],
                vstar=hr['vstar'], lw=lw)


def prob_stderr(h, lw):
    """Standard error of the self-normalised estimate sum_s wbar_s h_s by the delta method for a
    ratio of means: sqrt(sum_s wbar_s^2 (h_s - est)^2)."""
    e = np.exp(lw - lw.max())
    wbar = e / e.sum()
    est = wbar.dot(h)
    return est, np.sqrt(((wbar * (h - est)) ** 2).sum())
