# -*- coding: utf-8 -*-
"""Gradient of the Laplace log marginal likelihood of the probit (or, with
``likelihood='logit'``, logistic) GP classifier with respect to the kernel hyperparameters
``theta``, on the GPU.

``LogMarginalLikelihoodLaplaceEstimator`` gives the Laplace approximation's log marginal
likelihood at a ``theta``; :class:`LaplaceGradient` also says which way to move ``theta``: the
analytic derivative at the mode (Rasmussen & Williams, Alg. 5.1 in the ``B = I + W^1/2 K W^1/2``
form of ``latent_posterior_approximations``), at the cost of about nine Newton iterations whatever
the number of length scales. The jitter ``epsilon`` the kernels add to K's diagonal does not
depend on ``theta`` and has no share in it. The reference has no such function; everything runs
in libapm.so (``apm_laplace_grad``) and nothing but theta crosses the host
boundary.

The derivative is that of the converged fit: the class defaults to a tight Newton tolerance
(``diff_f_tol=1e-14``, a few iterations more than the estimators' ``1e-4``), because at the loose
one the gradient is off by about 1e-2 on entries of size 10. ``maximise`` runs L-BFGS-B on the
(negative) Laplace log posterior for type-II maximum likelihood / MAP starts of the chains; the
log-prior arithmetic is in the module-level function, which needs no device.
"""
import numpy as np

from . import _native
from .estimators import _kernel_spec, _raise_for_status

__all__ = ['LaplaceGradient', 'add_gaussian_log_prior']


def add_gaussian_log_prior(thetas, lml, grad, prior_mean, prior_std):
    """``(lml + log N(theta; m, s^2), grad - (theta - m) / s^2)`` for thetas (T, P), lml (T,) and
    grad (T, P), with an independent Gaussian prior on every component (``prior_mean`` /
    ``prior_std`` scalars or (P,) arrays, ``prior_std > 0``)."""
    th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    lml = np.asarray(lml, dtype=np.float64)
    grad = np.asarray(grad, dtype=np.float64)
    if lml.shape != (th.shape[0],) or grad.shape != th.shape:
        raise ValueError('lml {0} / grad {1} do not match thetas {2}'
                         .format(lml.shape, grad.shape, th.shape))
    m = np.broadcast_to(np.asarray(prior_mean, dtype=np.float64), (th.shape[1],))
    s = np.broadcast_to(np.asarray(prior_std, dtype=np.float64), (th.shape[1],))
    if not np.all(s > 0.0):
        raise ValueError('prior_std must be positive')
    z = (th - m[None, :]) / s[None, :]
    log_prior = (-0.5 * z ** 2 - np.log(s)[None, :] - 0.5 * np.log(2.0 * np.pi)).sum(1)
    return lml + log_prior, grad - z / s[None, :]


class LaplaceGradient(object):
    """Laplace log marginal likelihood and its gradient with respect to ``theta`` for the probit
    (``likelihood='logit'``: logistic) GP classifier trained on ``(X, y)``, for batches of
    hyperparameter vectors.

    ``kernel_func`` must be one of the two device kernels (``gpdemo.kernels.make_kernel_func``):
    the kernel's derivatives are built on the device, so a foreign callable raises
    ``NotImplementedError``. ``diff_f_tol`` / ``max_iters`` are the Newton settings of
    ``laplace_approximation``; ``max_batch`` thetas are fitted per device call.
    """

    def __init__(self, X, y, kernel_func, diff_f_tol=1e-14, max_iters=1000, max_batch=8,
                 device=None, likelihood='probit'):
        _native.likelihood_code(likelihood)
        self.likelihood = likelihood
        kind, eps = _kernel_spec(kernel_func)
        if kind == _native.KERNEL_PRECOMPUTED:
            raise NotImplementedError(
                'the device gradient builds the kernel derivatives itself and needs one of '
                'gpdemo.kernels.make_kernel_func("iso" | "ard"); got {0!r}'.format(kernel_func))
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.kernel_func = kernel_func
        self.max_iters = int(max_iters)
        # the gradient uses neither cache slots nor U buffers: one of each, one draw
        self._ctx = _native.Context(self.X, self.y, kind, eps, 1, max_batch=int(max_batch),
                                    n_slots=1, n_ubufs=1, device=device, likelihood=likelihood)
        self._ctx.set_newton(diff_f_tol, max_iters)
        self.n_iter = None
        self.status = None

    def __call__(self, thetas, on_error='raise'):
        """``(lml (T,), grad (T, P))`` for thetas of shape (T, P) or (P,). A theta whose Laplace
        fit fails raises the estimators' exception (``LinAlgError``,
        ``MaximumIterationsExceededError``); with ``on_error='nan'`` its row is NaN instead.
        ``self.n_iter`` keeps the Newton iteration counts and ``self.status`` the status codes."""
        if on_error not in ('raise', 'nan'):
            raise ValueError("on_error must be 'raise' or 'nan'")
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        lml, grad, st, nit = self._ctx.laplace_grad(th)
        self.n_iter, self.status = nit, st
        if on_error == 'raise':
            for s in st:
                _raise_for_status(int(s), self._ctx, self.max_iters)
        return lml, grad

    def log_posterior(self, thetas, prior_mean, prior_std, on_error='raise'):
        """``(value (T,), grad (T, P))`` of the Laplace log marginal likelihood plus an
        independent Gaussian log prior N(prior_mean, prior_std^2) on theta."""
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        lml, grad = self(th, on_error)
        return add_gaussian_log_prior(th, lml, grad, prior_mean, prior_std)

    def maximise(self, theta0, prior_mean=None, prior_std=None, gtol=1e-5, maxiter=100):
        """L-BFGS-B ascent of the Laplace log marginal likelihood (type-II maximum likelihood)
        or, with ``prior_mean`` and ``prior_std``, of the log posterior (MAP) from the one start
        ``theta0`` (P,). Returns scipy's result object (``x``, ``success``, ``nfev``, ...; ``fun``
        and ``jac`` are those of the minimised negative) with three entries added: ``lml``, the
        Laplace log marginal likelihood at ``x``; ``value``, the maximised objective there (``lml``
        plus the log prior, if any); ``grad``, its gradient. A theta whose fit fails inside the
        line search counts as ``+inf`` and does not raise, so that the optimiser backs off."""
        from scipy.optimize import minimize
        if (prior_mean is None) != (prior_std is None):
            raise ValueError('prior_mean and prior_std go together')
        theta0 = np.asarray(theta0, dtype=np.float64)
        if theta0.ndim != 1:
            raise ValueError('maximise takes one start of shape (P,), got {0}'
                             .format(theta0.shape))

        def value_and_grad(theta):
            if prior_mean is None:
                return self(theta, 'nan')
            return self.log_posterior(theta, prior_mean, prior_std, 'nan')

        def negative(theta):
            val, grad = value_and_grad(theta)
            if not np.isfinite(val[0]):
                return np.inf, np.zeros_like(theta)
            return -val[0], -grad[0]

        # ftol at machine epsilon: the stop is gtol's (scipy's default relative-decrease test,
        # 2.2e-9, ends a well-conditioned fit with a gradient above gtol)
        res = minimize(negative, theta0, jac=True, method='L-BFGS-B',
                       options=dict(gtol=gtol, maxiter=maxiter, ftol=np.finfo(np.float64).eps))
        lml, grad = self(res.x, 'nan')
        res['lml'] = float(lml[0])
        if prior_mean is not None:
            lml, grad = add_gaussian_log_prior(res.x, lml, grad, prior_mean, prior_std)
        res['value'], res['grad'] = float(lml[0]), grad[0]
        return res

    def close(self):
        self._ctx.close()
