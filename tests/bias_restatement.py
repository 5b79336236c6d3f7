"""numpy restatement of the constant (bias) covariance term, shared by
test_bias_host.py and test_gpu_bias.py. A plain module that wraps the existing restatements.

For a base kind (family 'se' | '32' | '52', kind 'iso' | 'ard') with theta-length P0 (2 for iso,
d + 1 for ARD) the biased kind takes theta of length P = P0 + 1; theta[:P0] keep their meaning and
beta = exp(theta[P - 1]):

    K_ij  = S_ij + beta                 data pairs; K_ii = s + beta + epsilon, s = exp(theta_0)
    k*_ij = S*_ij + beta                the cross-Gram, no epsilon
    k**   = s + beta                    the prior variance at a test point
    dK/dtheta_{P-1} = beta              every data pair, the diagonal included, no epsilon
    dK/dtheta_0 = S (s on the diagonal); the length-scale derivatives are the base kind's

S is the C oracle's Gram for the SE family (grad_restatement.gram) and matern_restatement's for
'32' / '52'. The Newton loop, the M formula, the EP fit and the predictive formulas are the
imported restatements', run with this module's K, k*, k** and dK.
"""
import contextlib
import math

import numpy as np
import scipy.linalg as la

import ep_restatement as ep
import grad_restatement as gr
import matern_restatement as mr
import predict_restatement as pr

_SE_GRAM, _SE_DK = gr.gram, gr.dK  # (grad_restatement's own: _substituted() replaces the names)
FAMILIES = ('se', '32', '52')
FAMILY_KINDS = [(f, k) for f in FAMILIES for k in ('iso', 'ard')]
COV_BIAS = 16
_BASE = {('se', 'iso'): 0, ('se', 'ard'): 1, ('32', 'iso'): 3, ('32', 'ard'): 4, ('52', 'iso'): 5,
         ('52', 'ard'): 6}


def native_kind(family, kind, bias=True):
    """The C-ABI's value: APM_KERNEL_* | APM_COV_BIAS."""
    return _BASE[family, kind] | (COV_BIAS if bias else 0)


def name(family, kind):
    """The name gpdemo.kernels.make_kernel_func and the batched samplers know the base kind by."""
    return kind if family == 'se' else 'matern{0}_{1}'.format(family, kind)


def n_base(kind, d):
    return d + 1 if kind == 'ard' else 2


def split(kind, theta, d):
    """(the base kind's theta, beta); a theta shorter than P0 + 1 is an IndexError."""
    theta = np.asarray(theta, dtype=np.float64)
    p0 = n_base(kind, d)
    if theta.shape[0] < p0 + 1:
        raise IndexError('theta too short')
    return theta[:p0], math.exp(theta[p0])


def base_S(family, kind, X, th0):
    """S of the base kind on one point set: no epsilon, s = exp(theta_0) on the diagonal."""
    if family == 'se':
        S = _SE_GRAM(kind, X, th0, 0.0)
    else:
        S = mr.gram(family, kind, X, th0, 0.0)
    S[np.diag_indices_from(S)] = math.exp(th0[0])
    return S


def base_cross(family, kind, Xs, X, th0):
    if family == 'se':
        return math.exp(th0[0]) * np.exp(-0.5 * mr.r2(kind, Xs, X, th0))
    return mr.gram_cross(family, kind, Xs, X, th0)


def gram(family, kind, X, theta, eps):
    th0, beta = split(kind, theta, X.shape[1])
    K = base_S(family, kind, X, th0) + beta
    K[np.diag_indices_from(K)] = math.exp(th0[0]) + beta + eps
    return K


def gram_cross(family, kind, Xs, X, theta):
    th0, beta = split(kind, theta, X.shape[1])
    return base_cross(family, kind, Xs, X, th0) + beta


def prior_var(kind, theta, d):
    th0, beta = split(kind, theta, d)
    return math.exp(th0[0]) + beta


def dK(family, kind, X, theta, eps=0.0, minus_beta=True):
    """The P dense matrices dK/dtheta_j. ``minus_beta=False`` is the wrong reading (theta_0's
    weight taken from K's own entries, S + beta) that the gradient test must tell apart."""
    n, d = X.shape
    th0, beta = split(kind, theta, d)
    if family == 'se':
        S = base_S(family, kind, X, th0)
        out = _SE_DK(kind, X, th0, S, 0.0)
    else:
        out = mr.dK(family, kind, X, th0, 0.0)
    out = [np.array(D) for D in out]
    if not minus_beta:
        out[0] = out[0] + beta
    out.append(np.full((n, n), beta))
    return out


def kernel_func(family, kind, eps):
    """``kernel_func(K, X, theta)`` for the oracle's estimators."""
    def fn(K, X, theta):
        K[...] = gram(family, kind, X, theta, eps)
    return fn


@contextlib.contextmanager
def _substituted(family, minus_beta=True):
    """grad_restatement with this module's K and dK in place of its SE ones."""
    old = gr.gram, gr.dK
    gr.gram = lambda kind, X, theta, eps: gram(family, kind, X, theta, eps)
    gr.dK = lambda kind, X, theta, K, eps, eps_in_dk0=False: dK(family, kind, X, theta, eps,
                                                               minus_beta)
    try:
        yield
    finally:
        gr.gram, gr.dK = old


def lml(family, kind, X, y, theta, eps, tol=1e-24):
    return gr.newton(gram(family, kind, X, theta, eps), y, tol)['lml']


def laplace_grad(family, kind, X, y, theta, eps, tol=1e-14, minus_beta=True):
    """dict(lml, grad (P,), n_iter, diffs): grad_restatement.laplace_grad (Newton loop, M)."""
    with _substituted(family, minus_beta):
        return gr.laplace_grad(kind, X, y, np.asarray(theta, dtype=np.float64), eps, tol=tol)


def predictive(family, kind, X, y, Xs, theta, eps, tol=1e-4):
    """predict_restatement.predictive with the biased K, k* and k** = s + beta."""
    return pr.predictive(gram(family, kind, X, theta, eps), gram_cross(family, kind, Xs, X, theta),
                         y, prior_var(kind, theta, X.shape[1]), tol=tol)


def ep_logz(family, kind, X, y, theta, eps, **ep_settings):
    return ep.ep_fit(gram(family, kind, X, theta, eps), y, **ep_settings)['logz']


def ep_grad(family, kind, X, y, theta, eps, **ep_settings):
    """ep_grad_restatement.ep_grad's algebra (M = 1/2 a a^T - 1/2 R at the sweep the fit stopped
    at) with the biased K and dK: dict(logz, grad (P,), n_sweeps, fit)."""
    fit = ep.ep_fit(gram(family, kind, X, theta, eps), y, **ep_settings)
    Z = la.solve_triangular(fit['L'], np.diag(fit['s']), lower=True)
    M = 0.5 * np.outer(fit['a'], fit['a']) - 0.5 * Z.T.dot(Z)
    grad = np.array([float((M * D).sum()) for D in dK(family, kind, X, theta)])
    return dict(logz=fit['logz'], grad=grad, n_sweeps=fit['n_sweeps'], fit=fit)


def ep_predictive(family, kind, X, y, Xs, theta, eps, **ep_settings):
    fit = ep.ep_fit(gram(family, kind, X, theta, eps), y, **ep_settings)
    out = ep.at_test_inputs(gram_cross(family, kind, Xs, X, theta),
                            prior_var(kind, theta, X.shape[1]), fit)
    out['n_sweeps'] = fit['n_sweeps']
    return out


def gram_bound(family, kind, A, B, theta, Kref):
    """Per-entry bound on |K - Kref| of a device Gram or cross-Gram (u = 2^-53): the base kind's
    bound on S - for SE test_gpu_kernels' rule relative to the exponent, 2e-15 max(1, |log S|) |S|;
    for Matern matern_restatement.gram_bound - plus 3 u |Kref| for the exp of theta_{P-1}, the
    sum S + beta and the epsilon."""
    u = 2.0 ** -53
    th0, beta = split(kind, theta, A.shape[1])
    Sref = base_cross(family, kind, A, B, th0)
    if family == 'se':
        base = 2e-15 * np.maximum(1.0, np.abs(np.log(np.maximum(Sref, 1e-300)))) * np.abs(Sref)
    else:
        base = mr.gram_bound(kind, A, B, th0, Sref)
    return base + 3.0 * u * np.abs(Kref)


def make_case(n, d, kind, seed, log_betas=(-2.0, 1.5), sigmas=(0.3, 3.0, -1.0), offset=1.0):
    """grad_restatement.make_case's inputs and length scales, the labels drawn with `offset`
    added to the latent so that the classes are uneven, and one theta per (theta_0, log beta)."""
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) + offset > 0, 1.0, -1.0)
    nl = d if kind == 'ard' else 1
    thetas = np.array([np.r_[s0, 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=nl), lb]
                       for s0 in sigmas for lb in log_betas])
    return dict(n=n, d=d, kind=kind, X=X, y=y, thetas=thetas)


def symmetric_ulp_noise(K, seed):
    """K with 1-ulp symmetric relative noise: K_ij (1 + 2^-52 e_ij), e symmetric in {-1, 0, 1}."""
    rng = np.random.RandomState(seed)
    e = np.tril(rng.randint(-1, 2, size=K.shape).astype(np.float64))
    e = e + np.tril(e, -1).T
    return K * (1.0 + 2.0 ** -52 * e)
