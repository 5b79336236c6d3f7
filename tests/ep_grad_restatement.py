"""numpy/scipy restatement of the gradient of log Z_EP with respect to theta (DESIGN.md §18;
apm_ep_grad), shared by test_ep_grad_host.py and test_gpu_ep_grad.py. A plain module: the parallel
EP fit of ep_restatement, then dense algebra with S^1/2, L and a of the sweep the fit stopped at,
as the device holds them (Rasmussen & Williams eq. 5.27 / Alg. 5.2; a is their b):

    Z = L^-1 diag(S^1/2),  R = Z^T Z = S^1/2 B^-1 S^1/2,  M = 1/2 a a^T - 1/2 R
    d log Z_EP / d theta_j = sum_ik M_ik (dK/dtheta_j)_ik

with the dK/dtheta_j of grad_restatement (SE) or matern_restatement ('32' / '52'): dK/dtheta_0 = S
without epsilon. This is the explicit derivative only; the one through the sites vanishes at the
EP fixed point, so the result is as exact as the fit is converged.
"""
import numpy as np
import scipy.linalg as la

import ep_restatement as ep
import grad_restatement as gr
import matern_restatement as mr


def gram(kind, X, theta, eps, family='se'):
    """K of the family: the C oracle's Gram for SE (the kinds it builds), matern_restatement's
    numpy Gram for '32' / '52'."""
    theta = np.asarray(theta, dtype=np.float64)
    if family == 'se':
        return gr.gram(kind, X, theta, eps)
    return mr.gram(family, kind, X, theta, eps)


def dK(kind, X, theta, K, eps, family='se', eps_in_dk0=False):
    if family == 'se':
        return gr.dK(kind, X, theta, K, eps, eps_in_dk0)
    out = mr.dK(family, kind, X, theta, eps)
    if eps_in_dk0:
        out[0] = out[0] + eps * np.eye(X.shape[0])
    return out


def logz(kind, X, y, theta, eps, family='se', **ep_settings):
    return ep.ep_fit(gram(kind, X, theta, eps, family), y, **ep_settings)['logz']


def ep_grad(kind, X, y, theta, eps, family='se', eps_in_dk0=False, K=None, **ep_settings):
    """dict(logz, grad (P,), n_sweeps, m_hist) at theta; ep_settings are ep_fit's (damping,
    diff_tol, max_sweeps). K: the Gram to fit on instead of building it from theta (it must be
    theta's: the iso / ARD identity puts both sides on one set of bits)."""
    theta = np.asarray(theta, dtype=np.float64)
    if K is None:
        K = gram(kind, X, theta, eps, family)
    fit = ep.ep_fit(K, y, **ep_settings)
    Z = la.solve_triangular(fit['L'], np.diag(fit['s']), lower=True)
    M = 0.5 * np.outer(fit['a'], fit['a']) - 0.5 * Z.T.dot(Z)
    grad = np.array([float((M * D).sum())
                     for D in dK(kind, X, theta, K, eps, family, eps_in_dk0)])
    return dict(logz=fit['logz'], grad=grad, n_sweeps=fit['n_sweeps'], m_hist=fit['m_hist'])
