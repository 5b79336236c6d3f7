"""numpy restatement of the Matérn 3/2 and 5/2 covariance functions, iso and ARD,
shared by test_matern_host.py and test_gpu_matern.py. A plain module. The oracle's C Gram knows
the SE family only, so these tests bring their own: with s = exp(theta_0), tau_k = exp(theta_{k+1})
(ARD) or exp(theta_1) for every k (iso) and r^2 = sum_k ((x_ik - x_jk)/tau_k)^2, summed over k in
a plain loop in order,

    family '32':  S = s (1 + sqrt3 r) exp(-sqrt3 r)               G = 3 s exp(-sqrt3 r)
    family '52':  S = s (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)     G = 5/3 s (1 + sqrt5 r) exp(-sqrt5 r)

K = S + epsilon I on one point set's Gram only (no epsilon on the cross-Gram), dK/dtheta_0 = S and
dK/dtheta_{k+1} = G_ij ((x_ik - x_jk)/tau_k)^2 (ARD; iso: the sum over k).

The Laplace quantities are grad_restatement's: its Newton loop and its M formula are imported and
run with this module's K and dK in place of the SE ones.
"""
import contextlib
import math

import numpy as np

import grad_restatement as gr

FAMILIES = ('32', '52')
SQRT3, SQRT5 = math.sqrt(3.0), math.sqrt(5.0)


def n_theta(kind, d):
    return d + 1 if kind == 'ard' else 2


def _tau(kind, theta, d):
    theta = np.asarray(theta, dtype=np.float64)
    if theta.shape[0] < n_theta(kind, d):
        raise IndexError('theta too short')
    return np.exp(theta[1:d + 1]) if kind == 'ard' else np.full(d, math.exp(theta[1]))


def r2(kind, A, B, theta):
    """(len(A), len(B)) scaled squared distances, the sum over k in order."""
    tau = _tau(kind, theta, A.shape[1])
    out = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        out += ((A[:, None, k] - B[None, :, k]) / tau[k]) ** 2
    return out


def cov_S(family, sigma, q):
    """The covariance function of the scaled squared distance q = r^2."""
    r = np.sqrt(q)
    if family == '32':
        return sigma * ((1.0 + SQRT3 * r) * np.exp(-SQRT3 * r))
    if family == '52':
        return sigma * ((1.0 + SQRT5 * r + (5.0 / 3.0) * q) * np.exp(-SQRT5 * r))
    raise ValueError('family must be one of {0}'.format(FAMILIES))


def cov_G(family, sigma, q):
    """The weight of the length-scale derivatives."""
    r = np.sqrt(q)
    if family == '32':
        return 3.0 * sigma * np.exp(-SQRT3 * r)
    if family == '52':
        return (5.0 / 3.0) * sigma * ((1.0 + SQRT5 * r) * np.exp(-SQRT5 * r))
    raise ValueError('family must be one of {0}'.format(FAMILIES))


def gram_cross(family, kind, Xs, X, theta):
    """(m, n) cross-covariance, no epsilon (also where two points coincide)."""
    return cov_S(family, math.exp(theta[0]), r2(kind, Xs, X, theta))


def gram(family, kind, X, theta, eps):
    """K = S + eps I; the diagonal is exp(theta_0) + eps exactly."""
    K = gram_cross(family, kind, X, X, theta)
    K[np.diag_indices_from(K)] = math.exp(theta[0]) + eps
    return K


def dK(family, kind, X, theta, eps):
    """The P dense matrices dK/dtheta_j (eps is not part of any of them)."""
    n, d = X.shape
    sigma = math.exp(theta[0])
    q = r2(kind, X, X, theta)
    S = cov_S(family, sigma, q)
    S[np.diag_indices_from(S)] = sigma
    G = cov_G(family, sigma, q)
    tau = _tau(kind, theta, d)
    sq = [((X[:, None, k] - X[None, :, k]) / tau[k]) ** 2 for k in range(d)]
    out = [S]
    if kind == 'ard':
        out.extend(G * s for s in sq)
    else:
        out.append(G * sum(sq))
    return out


def kernel_func(family, kind, eps):
    """``kernel_func(K, X, theta)`` for the oracle's is_estimate / priormc_estimate /
    laplace_estimate."""
    def fn(K, X, theta):
        K[...] = gram(family, kind, X, theta, eps)
    return fn


@contextlib.contextmanager
def _substituted(family):
    """grad_restatement with this module's K and dK in place of its SE ones."""
    old = gr.gram, gr.dK
    gr.gram = lambda kind, X, theta, eps: gram(family, kind, X, theta, eps)
    gr.dK = lambda kind, X, theta, K, eps, eps_in_dk0=False: dK(family, kind, X, theta, eps)
    try:
        yield
    finally:
        gr.gram, gr.dK = old


def lml(family, kind, X, y, theta, eps, tol=1e-24):
    return gr.newton(gram(family, kind, X, theta, eps), y, tol)['lml']


def laplace_grad(family, kind, X, y, theta, eps, tol=1e-14):
    """dict(lml, grad (P,), n_iter, diffs): grad_restatement.laplace_grad (Newton loop, M)."""
    with _substituted(family):
        return gr.laplace_grad(kind, X, y, np.asarray(theta, dtype=np.float64), eps, tol=tol)


def gram_bound(kind, A, B, theta, Kref):
    """Per-entry bound on |K - Kref| for a device Gram in the direct form on pre-scaled
    coordinates a_k = x_ik / tau_k, c_k = x_jk / tau_k, with u = 2^-53:

        delta(r^2) = 4 u sum_k (|a_k| + |c_k|) |a_k - c_k| + (D + 2) u r^2
        |K - Kref| <= |Kref| (8 u + 2 delta(r^2))

    (|d log S / d r^2| <= 3/2 for both families.)"""
    u = 2.0 ** -53
    tau = _tau(kind, theta, A.shape[1])
    D = A.shape[1]
    s1 = np.zeros((A.shape[0], B.shape[0]))
    q = np.zeros_like(s1)
    for k in range(D):
        a, c = A[:, None, k] / tau[k], B[None, :, k] / tau[k]
        s1 += (np.abs(a) + np.abs(c)) * np.abs(a - c)
        q += (a - c) ** 2
    delta = 4.0 * u * s1 + (D + 2) * u * q
    return np.abs(Kref) * (8.0 * u + 2.0 * delta)
