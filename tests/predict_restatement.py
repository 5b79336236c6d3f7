"""numpy/scipy restatement of the Laplace predictive distribution at test inputs (DESIGN.md §12;
apm_predict), shared by test_gpu_predict.py and test_gpu_laplace_edges.py. A plain module."""
import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr, ndtr


def predictive(K, Ks, y, sigma, tol=1e-4, max_iters=1000):
    """Newton loop of latent_posterior_approximations.py:81-99, then the predictive from the
    last iteration's W, L, a: mu = Ks a, var = sigma - |L^-1 (W^1/2 . ks)|^2,
    Phi(mu / sqrt(1 + var))."""
    n = y.shape[0]
    f, it = np.zeros(n), 0
    while True:
        v = np.exp(-0.5 * f ** 2 - log_ndtr(y * f) - 0.5 * np.log(2 * np.pi))
        grad = v * y
        W = v ** 2 + grad * f
        Ws = np.sqrt(W)
        L = la.cholesky(np.eye(n) + Ws[:, None] * K * Ws[None, :], lower=True)
        b = W * f + grad
        a = b - Ws * la.cho_solve((L, True), Ws * K.dot(b))
        f_new = K.dot(a)
        it += 1
        done = np.mean((f_new - f) ** 2) < tol
        f = f_new
        if done or it >= max_iters:
            break
    return dict(n_iter=it, f=f, a=a, **at_test_inputs(Ks, sigma, L, Ws, a))


def at_test_inputs(Ks, sigma, L, Ws, a):
    """mean, var and prob at the rows of Ks from one Newton state (L, W^1/2, a)."""
    mu = Ks.dot(a)
    V = la.solve_triangular(L, (Ks * Ws[None, :]).T, lower=True)
    var = sigma - (V * V).sum(0)
    return dict(mean=mu, var=var, prob=ndtr(mu / np.sqrt(1.0 + var)))
