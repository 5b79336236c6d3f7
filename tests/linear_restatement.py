"""numpy restatement of the linear (dot-product) covariance term, shared by
test_linear_host.py and test_gpu_linear.py. A plain module that wraps bias_restatement's pieces.

For an SE base kind ('iso' | 'ard') with theta-length P0 (2 for iso, d + 1 for ARD) the kind with
the linear term, with (bias=True) or without the constant term, takes theta of length
P = P0 + bias + 1; theta[:P0] keep their meaning, lambda = exp(theta[P - 1]) and, with both,
beta = exp(theta[P - 2]). The dot products are on the raw inputs:

    K_ij  = S_ij [+ beta] + lambda x_i . x_j      data pairs
    K_ii  = (s [+ beta]) + lambda |x_i|^2 + eps   s = exp(theta_0)
    k*_ij = S*_ij [+ beta] + lambda x*_i . x_j    the cross-Gram, no epsilon
    k**_i = s [+ beta] + lambda |x*_i|^2          the prior variance, per test row
    dK/dtheta_{P-1} = lambda x_i . x_j            every data pair, the diagonal included, no epsilon

The other derivatives are the base kind's (theta_0's is S with s on the diagonal; beta's is beta on
every pair). The Newton loop, the M formula, the EP fit and the predictive formulas are the
imported restatements', run with this module's K, k*, k** and dK.
"""
import contextlib
import math

import numpy as np
import scipy.linalg as la

import bias_restatement as br
import ep_restatement as ep
import grad_restatement as gr
import predict_restatement as pr

COV_LINEAR = 64
KINDS = [('iso', False), ('ard', False), ('iso', True), ('ard', True)]  # (kind, bias)


def native_kind(kind, bias, linear=True):
    """The C-ABI's value: APM_KERNEL_ISO | _ARD [| APM_COV_BIAS] [| APM_COV_LINEAR]."""
    return br.native_kind('se', kind, bias) | (COV_LINEAR if linear else 0)


def theta_len(kind, bias, d):
    return br.n_base(kind, d) + (1 if bias else 0) + 1


def split(kind, bias, theta, d):
    """(the base kind's theta, beta (0.0 without the constant term), lambda); a theta shorter than
    P is an IndexError."""
    theta = np.asarray(theta, dtype=np.float64)
    p0 = br.n_base(kind, d)
    if theta.shape[0] < theta_len(kind, bias, d):
        raise IndexError('theta too short')
    beta = math.exp(theta[p0]) if bias else 0.0
    return theta[:p0], beta, math.exp(theta[p0 + (1 if bias else 0)])


def without_linear(kind, bias, theta, d):
    """theta of the same kind without the linear flag (the last entry dropped)."""
    return np.asarray(theta, dtype=np.float64)[:theta_len(kind, bias, d) - 1]


def gram(kind, bias, X, theta, eps):
    th0, beta, lam = split(kind, bias, theta, X.shape[1])
    G = X.dot(X.T)
    K = br.base_S('se', kind, X, th0) + beta + lam * G
    K[np.diag_indices_from(K)] = (math.exp(th0[0]) + beta) + lam * G.diagonal() + eps
    return K


def gram_cross(kind, bias, Xs, X, theta):
    th0, beta, lam = split(kind, bias, theta, X.shape[1])
    return br.base_cross('se', kind, Xs, X, th0) + beta + lam * Xs.dot(X.T)


def prior_var(kind, bias, Xs, theta):
    """k** of every test row (m,)."""
    th0, beta, lam = split(kind, bias, theta, Xs.shape[1])
    return (math.exp(th0[0]) + beta) + lam * (Xs * Xs).sum(axis=1)


def dK(kind, bias, X, theta, eps=0.0):
    """The P dense matrices dK/dtheta_j."""
    n, d = X.shape
    th0, beta, lam = split(kind, bias, theta, d)
    S = br.base_S('se', kind, X, th0)
    out = [np.array(D) for D in br._SE_DK(kind, X, th0, S, 0.0)]
    if bias:
        out.append(np.full((n, n), beta))
    out.append(lam * X.dot(X.T))
    return out


def kernel_func(kind, bias, eps):
    """``kernel_func(K, X, theta)`` for the oracle's estimators."""
    def fn(K, X, theta):
        K[...] = gram(kind, bias, X, theta, eps)
    return fn


@contextlib.contextmanager
def _substituted(bias):
    """grad_restatement with this module's K and dK in place of its SE ones."""
    old = gr.gram, gr.dK
    gr.gram = lambda kind, X, theta, eps: gram(kind, bias, X, theta, eps)
    gr.dK = lambda kind, X, theta, K, eps, eps_in_dk0=False: dK(kind, bias, X, theta, eps)
    try:
        yield
    finally:
        gr.gram, gr.dK = old


def lml(kind, bias, X, y, theta, eps, tol=1e-24):
    return gr.newton(gram(kind, bias, X, theta, eps), y, tol)['lml']


def laplace_grad(kind, bias, X, y, theta, eps, tol=1e-14):
    """dict(lml, grad (P,), n_iter, diffs): grad_restatement.laplace_grad (Newton loop, M)."""
    with _substituted(bias):
        return gr.laplace_grad(kind, X, y, np.asarray(theta, dtype=np.float64), eps, tol=tol)


def predictive(kind, bias, X, y, Xs, theta, eps, tol=1e-4):
    """predict_restatement.predictive with this module's K, k* and the per-row k**."""
    return pr.predictive(gram(kind, bias, X, theta, eps), gram_cross(kind, bias, Xs, X, theta), y,
                         prior_var(kind, bias, Xs, theta), tol=tol)


def ep_logz(kind, bias, X, y, theta, eps, **ep_settings):
    return ep.ep_fit(gram(kind, bias, X, theta, eps), y, **ep_settings)['logz']


def ep_grad(kind, bias, X, y, theta, eps, **ep_settings):
    """ep_grad_restatement.ep_grad's algebra with this module's K and dK."""
    fit = ep.ep_fit(gram(kind, bias, X, theta, eps), y, **ep_settings)
    Z = la.solve_triangular(fit['L'], np.diag(fit['s']), lower=True)
    M = 0.5 * np.outer(fit['a'], fit['a']) - 0.5 * Z.T.dot(Z)
    grad = np.array([float((M * D).sum()) for D in dK(kind, bias, X, theta)])
    return dict(logz=fit['logz'], grad=grad, n_sweeps=fit['n_sweeps'], fit=fit)


def ep_predictive(kind, bias, X, y, Xs, theta, eps, **ep_settings):
    fit = ep.ep_fit(gram(kind, bias, X, theta, eps), y, **ep_settings)
    out = ep.at_test_inputs(gram_cross(kind, bias, Xs, X, theta),
                            prior_var(kind, bias, Xs, theta), fit)
    out['n_sweeps'] = fit['n_sweeps']
    return out


def gram_bound(kind, bias, A, B, theta, Kref):
    """Per-entry bound on |K - Kref| of a device Gram or cross-Gram (u = 2^-53): the base kind's
    bound on S (test_gpu_kernels' rule relative to the exponent, 2e-15 max(1, |log S|) |S|) plus
    3 u |Kref| plus (d + 2) u lambda sum_k |a_ik b_jk|, the forward bound of the chain of d fmas
    with the product's and lambda's roundings."""
    u = 2.0 ** -53
    d = A.shape[1]
    th0, beta, lam = split(kind, bias, theta, d)
    Sref = br.base_cross('se', kind, A, B, th0)
    base = 2e-15 * np.maximum(1.0, np.abs(np.log(np.maximum(Sref, 1e-300)))) * np.abs(Sref)
    return base + 3.0 * u * np.abs(Kref) + (d + 2) * u * lam * np.abs(A).dot(np.abs(B).T)


def make_case(n, d, kind, bias, seed, pairs=((0.3, -2.0), (0.3, 1.0), (3.0, 1.0), (-1.0, -2.0)),
              log_beta=1.5, offset=0.0):
    """grad_restatement.make_case-style inputs and length scales, the labels from a linear trend in
    the first feature, and one theta per (theta_0, log lambda) pair (log beta = 1.5 where biased)."""
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) + offset > 0, 1.0, -1.0)
    nl = d if kind == 'ard' else 1
    thetas = np.array([np.r_[s0, 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=nl),
                             [log_beta] if bias else [], ll] for s0, ll in pairs])
    return dict(n=n, d=d, kind=kind, bias=bias, X=X, y=y, thetas=thetas)


symmetric_ulp_noise = br.symmetric_ulp_noise
