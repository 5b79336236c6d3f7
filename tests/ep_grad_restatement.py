"""numpy/scipy restatement of the gradient of log Z_EP with respect to theta (DESIGN.md §18;
apm_ep_grad), shared by test_ep_grad_host.py and test_gpu_ep_grad.py. A plain module: the parallel
EP fit of ep_restatement, then dense algebra with S^1/2, L and a of the sweep the fit stopped at,
as the device holds them (Rasmussen & Williams eq. 5.27 / Alg. 5.2; a is their b):

    Z = L^-1 diag(S^1/2),  R = Z^T Z = S^1/2 B^-1 S^1/2,  M = 1/2 a a^T - 1/2 R
    d log Z_EP / d theta_j = sum_ik M_ik (dK/dtheta_j)_ik

with the dK/dtheta_j of the caller's covariance kind (cov_restatement's Cov.dK): dK/dtheta_0 = S
without epsilon. This is the explicit derivative only; the one through the sites vanishes at the
EP fixed point, so the result is as exact as the fit is converged.
"""
import numpy as np
import scipy.linalg as la

import ep_restatement as ep


def grad_of_fit(fit, dKs):
    """(P,) from an EP state (a, L, s of ep_restatement.ep_fit or ep_quad_restatement.ep_fit)."""
    Z = la.solve_triangular(fit['L'], np.diag(fit['s']), lower=True)
    M = 0.5 * np.outer(fit['a'], fit['a']) - 0.5 * Z.T.dot(Z)
    return np.array([float((M * D).sum()) for D in dKs])


def ep_grad(K, dKs, y, **ep_settings):
    """dict(logz, grad (P,), n_sweeps, m_hist, fit); ep_settings are ep_fit's (damping, diff_tol,
    max_sweeps)."""
    fit = ep.ep_fit(K, y, **ep_settings)
    return dict(logz=fit['logz'], grad=grad_of_fit(fit, dKs), n_sweeps=fit['n_sweeps'],
                m_hist=fit['m_hist'], fit=fit)
