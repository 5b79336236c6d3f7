# -*- coding: utf-8 -*-
"""Laplace approximation of the latent posterior p(f | y, theta, X) for probit (or, with
``likelihood='logit'``, logistic) GP classification, computed on the GPU (reference
latent_posterior_approximations.py:22-124).

Same signature, return tuples, convergence rule (mean squared change of f below
``diff_f_tol``), iteration cap and exception as the reference. The covariance C and the LML
use the Newton quantities of the last iteration together with the updated f, as the
reference does (:107-110).
"""
import numpy as np

from . import _native

__all__ = ['MaximumIterationsExceededError', 'InvalidCavityError', 'laplace_approximation',
           'ep_approximation']


class MaximumIterationsExceededError(Exception):
    """Raised when Newton's method fails to converge by the iteration limit."""


class InvalidCavityError(Exception):
    """Raised when an expectation-propagation cavity precision is not positive and finite."""


def laplace_approximation(K, y, calc_cov=True, calc_lml=False, diff_f_tol=1e-4, max_iters=1000,
                          likelihood='probit'):
    """Returns ``(f, C, lml, n_ops)``, ``(f, lml, n_ops)``, ``(f, C, n_ops)`` or ``(f, n_ops)``
    depending on the flags, with ``n_ops`` the reference's count of O(N^3) operations.
    ``likelihood``: ``'probit'`` (the reference's) or ``'logit'``; a ``ValueError`` otherwise."""
    f, C, lml, n_iter, status = _native.laplace(K, y, calc_cov, calc_lml, diff_f_tol, max_iters,
                                                likelihood=likelihood)
    if status == _native.STATUS_MAXITER:
        raise MaximumIterationsExceededError(
            'Failed to converge in {0} iterations'.format(n_iter))
    if status != _native.STATUS_OK:
        raise np.linalg.LinAlgError('Cholesky factorisation of B failed (not positive definite)')
    if calc_cov and calc_lml:
        return f, C, lml, n_iter + 1
    if calc_lml:
        return f, lml, n_iter
    if calc_cov:
        return f, C, n_iter + 1
    return f, n_iter


# the estimators run this approximation fused on the device when they are handed this function
laplace_approximation.apm_fused = True


def ep_approximation(K, y, calc_cov=True, calc_lml=False, damping=0.8, diff_tol=1e-8,
                     max_sweeps=100, return_sites=False, likelihood='probit'):
    """Expectation-propagation approximation of the latent posterior (Rasmussen & Williams §3.6;
    parallel EP with damped site updates), computed on the GPU. ``likelihood``:
    ``'probit'`` (closed-form tilted moments) or ``'logit'`` (moments by the quadrature rule of
    DESIGN.md §27); a ``ValueError`` otherwise. No reference counterpart. The return shape is
    ``laplace_approximation``'s:
    ``(mu, C, lml, n_ops)``, ``(mu, lml, n_ops)``, ``(mu, C, n_ops)`` or ``(mu, n_ops)`` with
    ``mu`` the posterior mean, ``C`` the posterior covariance, ``lml = log Z_EP`` and ``n_ops``
    the project's own count of O(N^3) operations, two per sweep (one factorisation and one matrix
    triangular solve) plus one for ``C``. With ``return_sites=True`` a dict with the site
    parameters ``tau`` and ``nu``, the marginal variances ``var`` and ``n_sweeps`` is appended.
    Raises ``MaximumIterationsExceededError`` (no convergence in ``max_sweeps``),
    ``numpy.linalg.LinAlgError`` (a factorisation failed) or ``InvalidCavityError`` (a cavity
    precision was not positive, or a site left the quadrature rule's covered region)."""
    mu, var, tau, nu, C, logz, n_sweeps, status = _native.ep(K, y, calc_cov, damping, diff_tol,
                                                             max_sweeps, likelihood=likelihood)
    raise_for_ep_status(status, max_sweeps)
    n_ops = 2 * n_sweeps + (1 if calc_cov else 0)
    out = (mu,) + ((C,) if calc_cov else ()) + ((logz,) if calc_lml else ()) + (n_ops,)
    if return_sites:
        out += (dict(tau=tau, nu=nu, var=var, n_sweeps=n_sweeps),)
    return out


# the IS estimator runs this approximation fused on the device (EST_IS_EP theta-calls) when it
# is handed this function
ep_approximation.apm_fused = True


def raise_for_ep_status(status, max_sweeps):
    """The exception of an EP chain's status (include/apm.h), nothing for APM_STATUS_OK."""
    if status == _native.STATUS_OK:
        return
    if status == _native.STATUS_MAXITER:
        raise MaximumIterationsExceededError(
            'Failed to converge in {0} sweeps'.format(max_sweeps))
    if status == _native.STATUS_EP_CAVITY:
        raise InvalidCavityError('a cavity precision was not positive and finite')
    raise np.linalg.LinAlgError('Cholesky factorisation of B failed (not positive definite)')
