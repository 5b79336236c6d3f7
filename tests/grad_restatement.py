"""numpy/scipy restatement of the gradient of the Laplace log marginal likelihood with respect to
theta (apm_laplace_grad), shared by test_grad_host.py and test_gpu_grad.py. A plain
module: the Newton loop of latent_posterior_approximations.py:81-99, then dense algebra with the
W, L, a of the LAST iteration and the returned mode f = K a, as the device holds them.

    v = phi(f)/Phi(y f),  g = y v,  d3 = -[(2v + y f)(-f v - y v^2) + y v]
    Z = L^-1 diag(W^1/2),  R = Z^T Z,  dS_i = K_ii - |L^-1 (W^1/2 . K[:, i])|^2
    s2 = +1/2 dS . d3,  q = s2 - R (K s2)
    M = 1/2 a a^T - 1/2 R + 1/2 (q g^T + g q^T)
    dLML/dtheta_j = sum_ik M_ik (dK/dtheta_j)_ik

dK/dtheta_0 = S = K - epsilon I (the jitter does not depend on theta); the length-scale
derivatives S_ij ((x_ik - x_jk)/tau_k)^2 have a zero diagonal.
"""
import math

import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr

import apm_oracle as orc


def gram(kind, X, theta, eps):
    n = X.shape[0]
    K = np.empty((n, n))
    orc.c_gram(kind, K, X, np.asarray(theta, dtype=np.float64), eps)
    return K


def newton(K, y, tol, max_iters=1000):
    """The Newton loop; ``diffs`` keeps every iteration's mean((f_new - f)^2)."""
    n = y.shape[0]
    f, diffs = np.zeros(n), []
    while True:
        v = np.exp(-0.5 * f ** 2 - log_ndtr(y * f) - 0.5 * np.log(2 * np.pi))
        grad = v * y
        W = v ** 2 + grad * f
        Ws = np.sqrt(W)
        L = la.cholesky(np.eye(n) + Ws[:, None] * K * Ws[None, :], lower=True)
        b = W * f + grad
        a = b - Ws * la.cho_solve((L, True), Ws * K.dot(b))
        f_new = K.dot(a)
        diffs.append(np.mean((f_new - f) ** 2))
        f = f_new
        if diffs[-1] < tol or len(diffs) >= max_iters:
            break
    lml = -0.5 * a.dot(f) + log_ndtr(y * f).sum() - np.log(L.diagonal()).sum()
    return dict(f=f, a=a, W=W, Ws=Ws, L=L, lml=lml, n_iter=len(diffs), diffs=diffs)


def lml(kind, X, y, theta, eps, tol=1e-24):
    return newton(gram(kind, X, theta, eps), y, tol)['lml']


def dK(kind, X, theta, K, eps, eps_in_dk0=False):
    """The P matrices dK/dtheta_j. ``eps_in_dk0`` is the wrong reading (epsilon kept on the
    diagonal of dK/dtheta_0) that the epsilon-rule test must tell apart."""
    n, d = X.shape
    S = K - eps * np.eye(n)
    out = [K.copy() if eps_in_dk0 else S]
    tau = np.exp(np.asarray(theta, dtype=np.float64)[1:])
    sq = [((X[:, None, k] - X[None, :, k]) / tau[k if kind == 'ard' else 0]) ** 2
          for k in range(d)]
    if kind == 'ard':
        out.extend(S * s for s in sq)
    else:
        out.append(S * sum(sq))
    return out


def laplace_grad(kind, X, y, theta, eps, tol=1e-14, max_iters=1000, eps_in_dk0=False):
    """dict(lml, grad (P,), n_iter, diffs) at theta."""
    K = gram(kind, X, theta, eps)
    nw = newton(K, y, tol, max_iters)
    f, a, Ws, L = nw['f'], nw['a'], nw['Ws'], nw['L']
    v = np.exp(-0.5 * f ** 2 - log_ndtr(y * f) - 0.5 * np.log(2 * np.pi))
    g = y * v
    d3 = -((2.0 * v + y * f) * (-f * v - y * v ** 2) + y * v)
    Z = la.solve_triangular(L, np.diag(Ws), lower=True)
    R = Z.T.dot(Z)
    V = la.solve_triangular(L, Ws[:, None] * K, lower=True)
    dS = K.diagonal() - (V * V).sum(0)
    s2 = 0.5 * dS * d3
    q = s2 - R.dot(K.dot(s2))
    M = 0.5 * np.outer(a, a) - 0.5 * R + 0.5 * (np.outer(q, g) + np.outer(g, q))
    grad = np.array([float((M * D).sum()) for D in dK(kind, X, theta, K, eps, eps_in_dk0)])
    return dict(lml=nw['lml'], grad=grad, n_iter=nw['n_iter'], diffs=nw['diffs'])


def central_differences(fun, theta, h=1e-5):
    theta = np.asarray(theta, dtype=np.float64)
    out = np.empty(theta.shape[0])
    for j in range(theta.shape[0]):
        e = np.zeros_like(theta)
        e[j] = h
        out[j] = (fun(theta + e) - fun(theta - e)) / (2.0 * h)
    return out


def make_case(n, d, kind, seed, sigmas=(0.3, 3.0, -1.0)):
    """The generator of test_gpu_predict._make_case without the test inputs: length scales around
    sqrt(d), log tau = 1/2 log d + U(-0.3, 0.1)."""
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) > 0, 1.0, -1.0)
    nl = d if kind == 'ard' else 1
    thetas = np.array([np.r_[s0, 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=nl)]
                       for s0 in sigmas])
    return dict(n=n, d=d, kind=kind, X=X, y=y, thetas=thetas)
