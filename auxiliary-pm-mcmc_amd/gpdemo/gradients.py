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

:class:`EPGradient` is the same for the expectation-propagation evidence ``log Z_EP`` of the probit
classifier (``apm_ep_grad``): the explicit derivative at the EP fixed point (R&W
eq. 5.27), with the same ``__call__`` / ``log_posterior`` / ``maximise`` contract, so that theta
can be fitted under the EP approximation as well.
"""
import numpy as np

from . import _native
from .estimators import _kernel_spec, _raise_for_status
from .latent_posterior_approximations import raise_for_ep_status

__all__ = ['LaplaceGradient', 'EPGradient', 'add_gaussian_log_prior']


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


class _EvidenceGradient(object):
    """What :class:`LaplaceGradient` and :class:`EPGradient` share: one device context per
    ``(X, y, kernel_func)``, batches of thetas through it, the Gaussian log prior and the L-BFGS-B
    fit. A subclass names its evidence (``_name``, the key ``maximise`` adds to its result), makes
    the device call (``_evaluate``: ``(value (T,), grad (T, P), status, counts)``), keeps the
    counts (``_keep``) and maps a status to its exception (``_raise``)."""

    _name = None

    def _make_context(self, X, y, kernel_func, max_batch, device, likelihood):
        kind, eps = _kernel_spec(kernel_func)
        if kind == _native.KERNEL_PRECOMPUTED:
            raise NotImplementedError(
                'the device gradient builds the kernel derivatives itself and needs one of '
                'gpdemo.kernels.make_kernel_func("iso" | "ard"); got {0!r}'.format(kernel_func))
        self.likelihood = likelihood
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.kernel_func = kernel_func
        # the gradient uses neither cache slots nor U buffers: one of each, one draw
        self._ctx = _native.Context(self.X, self.y, kind, eps, 1, max_batch=int(max_batch),
                                    n_slots=1, n_ubufs=1, device=device, likelihood=likelihood)
        self.status = None

    def __call__(self, thetas, on_error='raise'):
        if on_error not in ('raise', 'nan'):
            raise ValueError("on_error must be 'raise' or 'nan'")
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        val, grad, st, counts = self._evaluate(th)
        self._keep(counts)
        self.status = st
        if on_error == 'raise':
            for s in st:
                self._raise(int(s))
        return val, grad

    def log_posterior(self, thetas, prior_mean, prior_std, on_error='raise'):
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        val, grad = self(th, on_error)
        return add_gaussian_log_prior(th, val, grad, prior_mean, prior_std)

    def maximise(self, theta0, prior_mean=None, prior_std=None, gtol=1e-5, maxiter=100):
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
        val, grad = self(res.x, 'nan')
        res[self._name] = float(val[0])
        if prior_mean is not None:
            val, grad = add_gaussian_log_prior(res.x, val, grad, prior_mean, prior_std)
        res['value'], res['grad'] = float(val[0]), grad[0]
        return res

    def close(self):
        self._ctx.close()


class LaplaceGradient(_EvidenceGradient):
    """Laplace log marginal likelihood and its gradient with respect to ``theta`` for the probit
    (``likelihood='logit'``: logistic) GP classifier trained on ``(X, y)``, for batches of
    hyperparameter vectors.

    ``kernel_func`` must be one of the two device kernels (``gpdemo.kernels.make_kernel_func``):
    the kernel's derivatives are built on the device, so a foreign callable raises
    ``NotImplementedError``. ``diff_f_tol`` / ``max_iters`` are the Newton settings of
    ``laplace_approximation``; ``max_batch`` thetas are fitted per device call.
    """

    _name = 'lml'

    def __init__(self, X, y, kernel_func, diff_f_tol=1e-14, max_iters=1000, max_batch=8,
                 device=None, likelihood='probit'):
        _native.likelihood_code(likelihood)
        self.max_iters = int(max_iters)
        self._make_context(X, y, kernel_func, max_batch, device, likelihood)
        self._ctx.set_newton(diff_f_tol, max_iters)
        self.n_iter = None

    def _evaluate(self, th):
        return self._ctx.laplace_grad(th)

    def _keep(self, counts):
        self.n_iter = counts

    def _raise(self, status):
        _raise_for_status(status, self._ctx, self.max_iters)

    def __call__(self, thetas, on_error='raise'):
        """``(lml (T,), grad (T, P))`` for thetas of shape (T, P) or (P,). A theta whose Laplace
        fit fails raises the estimators' exception (``LinAlgError``,
        ``MaximumIterationsExceededError``); with ``on_error='nan'`` its row is NaN instead.
        ``self.n_iter`` keeps the Newton iteration counts and ``self.status`` the status codes."""
        return super(LaplaceGradient, self).__call__(thetas, on_error)

    def log_posterior(self, thetas, prior_mean, prior_std, on_error='raise'):
        """``(value (T,), grad (T, P))`` of the Laplace log marginal likelihood plus an
        independent Gaussian log prior N(prior_mean, prior_std^2) on theta."""
        return super(LaplaceGradient, self).log_posterior(thetas, prior_mean, prior_std, on_error)

    def maximise(self, theta0, prior_mean=None, prior_std=None, gtol=1e-5, maxiter=100):
        """L-BFGS-B ascent of the Laplace log marginal likelihood (type-II maximum likelihood)
        or, with ``prior_mean`` and ``prior_std``, of the log posterior (MAP) from the one start
        ``theta0`` (P,). Returns scipy's result object (``x``, ``success``, ``nfev``, ...; ``fun``
        and ``jac`` are those of the minimised negative) with three entries added: ``lml``, the
        Laplace log marginal likelihood at ``x``; ``value``, the maximised objective there (``lml``
        plus the log prior, if any); ``grad``, its gradient. A theta whose fit fails inside the
        line search counts as ``+inf`` and does not raise, so that the optimiser backs off."""
        return super(LaplaceGradient, self).maximise(theta0, prior_mean, prior_std, gtol, maxiter)


class EPGradient(_EvidenceGradient):
    """Expectation-propagation evidence ``log Z_EP`` and its gradient with respect to ``theta``
    for the probit GP classifier trained on ``(X, y)``, for batches of hyperparameter vectors
    (``apm_ep_grad``).

    ``kernel_func`` must be one of the device kernels (``gpdemo.kernels.make_kernel_func``); a
    foreign callable raises ``NotImplementedError``, and so does ``likelihood='logit'`` without
    ``quadrature=True`` (the tilted moments by the quadrature rule of DESIGN.md §27; the gradient
    itself has no likelihood in it). ``damping`` / ``diff_tol`` / ``max_sweeps`` are the EP
    settings; ``max_batch`` thetas are fitted per device call.

    The derivative is the explicit one at the EP fixed point, so it is only as exact as the fit
    is converged. The class therefore defaults to a tight stop tolerance (``diff_tol=1e-16``,
    about twice the sweeps of the estimators' ``1e-8``, hence ``max_sweeps=1000``): over the
    shapes of DESIGN.md §18's table the gradient is then within 1.9e-8 of max(1, max|grad|) of
    the converged one, against 2.0e-4 at ``1e-8``, which would stall L-BFGS at ``gtol=1e-5``.
    """

    _name = 'logz'

    def __init__(self, X, y, kernel_func, damping=0.8, diff_tol=1e-16, max_sweeps=1000,
                 max_batch=8, device=None, likelihood='probit', quadrature=False):
        if _native.likelihood_code(likelihood) != _native.LIK_PROBIT and not quadrature:
            raise NotImplementedError('expectation propagation is implemented for the probit '
                                      'likelihood only, unless quadrature=True')
        self.max_sweeps = int(max_sweeps)
        self._make_context(X, y, kernel_func, max_batch, device, likelihood)
        self._ctx.set_ep(damping, diff_tol, max_sweeps, quadrature=bool(quadrature))
        self.n_sweeps = None

    def _evaluate(self, th):
        return self._ctx.ep_grad(th)

    def _keep(self, counts):
        self.n_sweeps = counts

    def _raise(self, status):
        raise_for_ep_status(status, self.max_sweeps)

    def __call__(self, thetas, on_error='raise'):
        """``(logz (T,), grad (T, P))`` for thetas of shape (T, P) or (P,). A theta whose EP fit
        fails raises the EP estimator's exception (``LinAlgError``, ``InvalidCavityError``,
        ``MaximumIterationsExceededError``); with ``on_error='nan'`` its row is NaN instead.
        ``self.n_sweeps`` keeps the sweep counts and ``self.status`` the status codes."""
        return super(EPGradient, self).__call__(thetas, on_error)

    def log_posterior(self, thetas, prior_mean, prior_std, on_error='raise'):
        """``(value (T,), grad (T, P))`` of ``log Z_EP`` plus an independent Gaussian log prior
        N(prior_mean, prior_std^2) on theta."""
        return super(EPGradient, self).log_posterior(thetas, prior_mean, prior_std, on_error)

    def maximise(self, theta0, prior_mean=None, prior_std=None, gtol=1e-5, maxiter=100):
        """:meth:`LaplaceGradient.maximise` on ``log Z_EP``: the entries added to scipy's result
        are ``logz`` (``log Z_EP`` at ``x``), ``value`` and ``grad``."""
        return super(EPGradient, self).maximise(theta0, prior_mean, prior_std, gtol, maxiter)
