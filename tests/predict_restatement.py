"""numpy/scipy restatement of the Laplace predictive distribution at test inputs (DESIGN.md §12;
apm_predict), shared by test_gpu_predict.py and test_gpu_laplace_edges.py. A plain module."""
import numpy as np
import scipy.linalg as la
from scipy.special import ndtr

import grad_restatement as gr


def predictive(K, Ks, y, sigma, tol=1e-4, max_iters=1000):
    """grad_restatement's Newton loop, then the predictive from the last iteration's W, L, a:
    mu = Ks a, var = sigma - |L^-1 (W^1/2 . ks)|^2, Phi(mu / sqrt(1 + var))."""
    nw = gr.newton(K, y, tol, max_iters)
    return dict(n_iter=nw['n_iter'], f=nw['f'], a=nw['a'],
                **at_test_inputs(Ks, sigma, nw['L'], nw['Ws'], nw['a']))


def at_test_inputs(Ks, sigma, L, Ws, a):
    """mean, var and prob at the rows of Ks from one Newton state (L, W^1/2, a)."""
    mu = Ks.dot(a)
    V = la.solve_triangular(L, (Ks * Ws[None, :]).T, lower=True)
    var = sigma - (V * V).sum(0)
    return dict(mean=mu, var=var, prob=ndtr(mu / np.sqrt(1.0 + var)))
