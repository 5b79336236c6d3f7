"""numpy/scipy restatement of the Laplace approximation's Newton loop and of the gradient of the
Laplace log marginal likelihood with respect to theta (apm_laplace_grad): the
one copy of each, for either likelihood and any covariance kind (K and the dK/dtheta_j come from
the caller: cov_restatement). A plain module: the Newton loop of
latent_posterior_approximations.py:81-99, then dense algebra with the W, L, a of the LAST
iteration and the returned mode f = K a, as the device holds them. With g = d log p / df and
d3 = d^3 log p / df^3 of the likelihood (probit: v = phi(f)/Phi(y f), g = y v,
d3 = -[(2v + y f)(-f v - y v^2) + y v]):

    Z = L^-1 diag(W^1/2),  R = Z^T Z,  dS_i = K_ii - |L^-1 (W^1/2 . K[:, i])|^2
    s2 = +1/2 dS . d3,  q = s2 - R (K s2)
    M = 1/2 a a^T - 1/2 R + 1/2 (q g^T + g q^T)
    dLML/dtheta_j = sum_ik M_ik (dK/dtheta_j)_ik
"""
import collections
import math

import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr

# What differs between the likelihoods: log p(y | f) as a function of t = y f, (grad, W) and d3
# as functions of (f, y). logit_restatement has the logit's record.
Likelihood = collections.namedtuple('Likelihood', 'log_lik grad_W d3')


def _probit_v(f, y):
    return np.exp(-0.5 * f ** 2 - log_ndtr(y * f) - 0.5 * np.log(2 * np.pi))


def _probit_grad_W(f, y):
    v = _probit_v(f, y)
    grad = v * y
    return grad, v ** 2 + grad * f


def _probit_d3(f, y):
    v = _probit_v(f, y)
    return -((2.0 * v + y * f) * (-f * v - y * v ** 2) + y * v)


PROBIT = Likelihood(log_ndtr, _probit_grad_W, _probit_d3)


def newton(K, y, tol, max_iters=1000, lik=PROBIT):
    """The Newton loop; ``diffs`` keeps every iteration's mean((f_new - f)^2)."""
    n = y.shape[0]
    f, diffs = np.zeros(n), []
    while True:
        grad, W = lik.grad_W(f, y)
        Ws = np.sqrt(W)
        L = la.cholesky(np.eye(n) + Ws[:, None] * K * Ws[None, :], lower=True)
        b = W * f + grad
        a = b - Ws * la.cho_solve((L, True), Ws * K.dot(b))
        f_new = K.dot(a)
        diffs.append(np.mean((f_new - f) ** 2))
        f = f_new
        if diffs[-1] < tol or len(diffs) >= max_iters:
            break
    lml = -0.5 * a.dot(f) + lik.log_lik(y * f).sum() - np.log(L.diagonal()).sum()
    return dict(f=f, a=a, W=W, Ws=Ws, L=L, lml=lml, n_iter=len(diffs), diffs=diffs)


def laplace_grad(K, dKs, y, tol=1e-14, max_iters=1000, lik=PROBIT):
    """dict(lml, grad (P,), n_iter, diffs, f); dKs the P matrices dK/dtheta_j."""
    nw = newton(K, y, tol, max_iters, lik)
    f, a, Ws, L = nw['f'], nw['a'], nw['Ws'], nw['L']
    g = lik.grad_W(f, y)[0]
    Z = la.solve_triangular(L, np.diag(Ws), lower=True)
    R = Z.T.dot(Z)
    V = la.solve_triangular(L, Ws[:, None] * K, lower=True)
    dS = K.diagonal() - (V * V).sum(0)
    s2 = 0.5 * dS * lik.d3(f, y)
    q = s2 - R.dot(K.dot(s2))
    M = 0.5 * np.outer(a, a) - 0.5 * R + 0.5 * (np.outer(q, g) + np.outer(g, q))
    grad = np.array([float((M * D).sum()) for D in dKs])
    return dict(lml=nw['lml'], grad=grad, n_iter=nw['n_iter'], diffs=nw['diffs'], f=f)


def central_differences(fun, theta, h=1e-5):
    theta = np.asarray(theta, dtype=np.float64)
    out = np.empty(theta.shape[0])
    for j in range(theta.shape[0]):
        e = np.zeros_like(theta)
        e[j] = h
        out[j] = (fun(theta + e) - fun(theta - e)) / (2.0 * h)
    return out


def make_case(n, d, kind, seed, rows=(0.3, 3.0, -1.0), offset=0.0):
    """Inputs, labels and one theta per row. A row is theta_0, or (theta_0, trailing
    log-parameters ...) for a kind with a constant or a linear term; the length scales are drawn
    around sqrt(d), log tau = 1/2 log d + U(-0.3, 0.1), one draw per row after X and the label
    noise. The labels follow the first feature plus ``offset`` (uneven classes)."""
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) + offset > 0, 1.0, -1.0)
    nl = d if kind == 'ard' else 1
    rows = [np.atleast_1d(np.asarray(row, dtype=np.float64)) for row in rows]
    thetas = np.array([np.r_[row[0], 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=nl), row[1:]]
                       for row in rows])
    return dict(n=n, d=d, kind=kind, X=X, y=y, thetas=thetas)
