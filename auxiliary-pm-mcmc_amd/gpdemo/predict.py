# -*- coding: utf-8 -*-
"""Laplace predictive distribution of the probit GP classifier at held-out inputs, on the GPU.

For a hyperparameter sample ``theta`` the Laplace fit of ``latent_posterior_approximations``
(Newton quantities ``W``, ``L = chol(I + W^1/2 K W^1/2)``, ``a`` of the last iteration) gives at
a test input ``x*`` the latent mean ``mu* = k*^T a``, the latent variance ``var* = k** -
|L^-1 (W^1/2 . k*)|^2`` and the class probability ``pi* = Phi(mu* / sqrt(1 + var*))`` (Rasmussen
& Williams, Alg. 3.2 with the probit's closed-form average). ``k*`` and ``k** = exp(theta_0)``
carry no jitter: the reference's kernels add epsilon to the diagonal of one point set's Gram
matrix only. With ``likelihood='logit'`` ``mu*`` and ``var*`` are the same expressions of the
logit's Laplace fit and ``pi* = int sigma(x) N(x | mu*, var*) dx`` is a Gauss-Hermite average
computed on the device. The reference has no such function; everything runs in
libapm.so (``apm_predict``,
DESIGN.md §12) and nothing but theta and the test inputs crosses the host boundary.

:class:`LaplacePredictor` evaluates a set of theta samples (e.g. a saved run's, see
INTEGRATION.md); the array math on its outputs is in the module-level functions, which need no
device.
"""
import numpy as np
from scipy.special import log_ndtr

from . import _native
from .estimators import _kernel_spec, _raise_for_status
from .latent_posterior_approximations import raise_for_ep_status

__all__ = ['LaplacePredictor', 'EPPredictor', 'ISPredictor', 'posterior_average',
           'log_predictive_density']


def _keep(a, burn, thin):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError('expected a (T, M) array, got shape {0}'.format(a.shape))
    a = a[int(burn)::int(thin)]
    if a.shape[0] == 0:
        raise ValueError('no samples left after burn / thin')
    return a


def posterior_average(prob, burn=0, thin=1):
    """Hyperparameter-marginalised class probability: the mean of ``prob`` (T, M) over the kept
    samples ``burn::thin``."""
    return _keep(prob, burn, thin).mean(0)


def log_predictive_density(mean, var, y_test, burn=0, thin=1, likelihood='probit', prob=None):
    """Test log predictive density per point: the mean over the M test points of
    ``log(mean_t Phi(y* z_t))`` with ``z = mean / sqrt(1 + var)`` (T, M) and labels ``y*`` in
    {-1, +1}. ``log Phi`` through ``log_ndtr`` and a log-mean-exp over the samples, so that
    confident predictions neither underflow to ``-inf`` nor round to 0. The logit's average has no
    closed form: with ``likelihood='logit'`` the per-sample terms are ``log(prob)`` (y* = +1) and
    ``log1p(-prob)`` (y* = -1) of the device's class probabilities ``prob`` (T, M), and ``mean``
    / ``var`` are not read."""
    _native.likelihood_code(likelihood)
    y = np.asarray(y_test, dtype=np.float64)
    if likelihood == 'logit':
        if prob is None:
            raise ValueError("likelihood='logit' needs the device's prob")
        lp = _log_prob_of_labels(_keep(prob, burn, thin), y)
    else:
        z = _keep(mean, burn, thin) / np.sqrt(1.0 + _keep(var, burn, thin))
        if y.shape != (z.shape[1],):
            raise ValueError('y_test has shape {0}, expected ({1},)'.format(y.shape, z.shape[1]))
        lp = log_ndtr(y[None, :] * z)
    return _log_mean_exp_density(lp)


def _log_prob_of_labels(p, y):
    """log p (y* = +1) or log1p(-p) (y* = -1) per sample and test point, p (T, M)."""
    if y.shape != (p.shape[1],):
        raise ValueError('y_test has shape {0}, expected ({1},)'.format(y.shape, p.shape[1]))
    with np.errstate(divide='ignore'):
        return np.where(y[None, :] > 0, np.log(p), np.log1p(-p))


def _log_mean_exp_density(lp):
    top = lp.max(0)
    return float(np.mean(top + np.log(np.mean(np.exp(lp - top[None, :]), axis=0))))


class LaplacePredictor(object):
    """Predictive distribution at ``X_test`` (M, D) of the GP classifier (``likelihood='probit'``
    or ``'logit'``) trained on ``(X, y)``, for batches of hyperparameter samples.

    ``kernel_func`` must be one of the two device kernels (``gpdemo.kernels.make_kernel_func``):
    the cross-covariance is built on the device, so a foreign callable raises
    ``NotImplementedError``. ``diff_f_tol`` / ``max_iters`` are the Newton settings of
    ``laplace_approximation``; ``max_batch`` thetas are fitted per device call.
    """

    def __init__(self, X, y, kernel_func, X_test, diff_f_tol=1e-4, max_iters=1000, max_batch=8,
                 device=None, likelihood='probit'):
        _native.likelihood_code(likelihood)
        self.likelihood = likelihood
        kind, eps = _kernel_spec(kernel_func)
        if kind == _native.KERNEL_PRECOMPUTED:
            raise NotImplementedError(
                'the device predictor builds the cross-covariance itself and needs one of '
                'gpdemo.kernels.make_kernel_func("iso" | "ard"); got {0!r}'.format(kernel_func))
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.X_test = np.ascontiguousarray(X_test, dtype=np.float64)
        if self.X_test.ndim != 2 or self.X_test.shape[1] != self.X.shape[1]:
            raise ValueError('X_test has shape {0}, expected (M, {1})'
                             .format(self.X_test.shape, self.X.shape[1]))
        self.kernel_func = kernel_func
        self.max_iters = int(max_iters)
        # prediction uses neither cache slots nor U buffers: one of each, one draw
        self._ctx = _native.Context(self.X, self.y, kind, eps, 1, max_batch=int(max_batch),
                                    n_slots=1, n_ubufs=1, device=device, likelihood=likelihood)
        self._ctx.set_newton(diff_f_tol, max_iters)
        self.n_iter = None

    def __call__(self, thetas, on_error='raise'):
        """``(mean, var, prob)``, each (T, M), for thetas of shape (T, P) or (P,). A theta whose
        Laplace fit fails raises the estimators' exception (``LinAlgError``,
        ``MaximumIterationsExceededError``); with ``on_error='nan'`` its rows are NaN instead.
        ``self.n_iter`` keeps the Newton iteration counts and ``self.status`` the status codes."""
        if on_error not in ('raise', 'nan'):
            raise ValueError("on_error must be 'raise' or 'nan'")
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        mean, var, prob, st, nit = self._ctx.predict(th, self.X_test)
        self.n_iter, self.status = nit, st
        if on_error == 'raise':
            for s in st:
                _raise_for_status(int(s), self._ctx, self.max_iters)
        return mean, var, prob

    def posterior_average(self, thetas, burn=0, thin=1, on_error='raise'):
        """Class probabilities (M,) averaged over the kept theta samples."""
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))[int(burn)::int(thin)]
        return posterior_average(self(th, on_error)[2])

    def log_predictive_density(self, thetas, y_test, burn=0, thin=1, on_error='raise'):
        """Mean test log predictive density of labels ``y_test`` (M,) in {-1, +1}."""
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))[int(burn)::int(thin)]
        mean, var, prob = self(th, on_error)
        return log_predictive_density(mean, var, y_test, likelihood=self.likelihood, prob=prob)

    _joint_approx = _native.JOINT_LAPLACE

    def _joint(self, thetas, on_error, **what):
        if on_error not in ('raise', 'nan'):
            raise ValueError("on_error must be 'raise' or 'nan'")
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        mean, cov, draws, lpd, st, nit = self._ctx.predict_joint(
            self._joint_approx, th, self.X_test, **what)
        self.n_iter, self.status = nit, st
        if on_error == 'raise':
            for s in st:
                self._raise_joint(int(s))
        return mean, cov, draws, lpd

    def _raise_joint(self, status):
        # (STATUS_CHOL_C, the factor of the joint covariance: InvalidCovarianceMatrixError)
        _raise_for_status(status, self._ctx, self.max_iters)

    @staticmethod
    def _seeds(seed, T):
        """One Philox seed per theta: an array of T seeds as it is, a scalar s as s, s + 1, ..."""
        sd = np.asarray(seed, dtype=np.uint64)
        return sd if sd.ndim else sd + np.arange(T, dtype=np.uint64)

    def joint(self, thetas, on_error='raise'):
        """``(mean, cov)``: the latent mean (T, M) and the full latent covariance (T, M, M) across
        the test inputs, ``K** - V V^T`` without jitter, for thetas (T, P) or (P,). The M test
        inputs are one block: M must not exceed the training set's padded size. Failures as in
        ``__call__``."""
        return self._joint(thetas, on_error, want_cov=True)[:2]

    def sample_latent(self, thetas, n_draws, seed, on_error='raise'):
        """``draws`` (T, n_draws, M) of the latent function at the test inputs from N(mean, cov +
        epsilon I), drawn on the device from the Philox stream ``(seed_t, 0)``; ``seed`` is one
        seed per theta or a scalar s for s, s + 1, ... The same seeds give the same draws. A
        covariance whose factor fails raises ``InvalidCovarianceMatrixError``."""
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        return self._joint(th, on_error, want_cov=False, n_draws=int(n_draws),
                           seeds=self._seeds(seed, th.shape[0]), want_draws=True)[2]

    def joint_log_predictive_density(self, thetas, y_test, n_draws, seed, burn=0, thin=1,
                                     on_error='raise'):
        """Joint log predictive density of the labels ``y_test`` (M,) in {-1, +1}: the log of the
        average over the kept thetas ``burn::thin`` of the per-theta joint density, itself a
        Monte-Carlo average over ``n_draws`` draws of the latent function taken on the device in log
        space. It does not factorise over the test points. ``seed`` as in ``sample_latent``, one
        per kept theta."""
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))[int(burn)::int(thin)]
        lpd = self._joint(th, on_error, want_cov=False, n_draws=int(n_draws),
                          seeds=self._seeds(seed, th.shape[0]), y_test=y_test)[3]
        return _log_mean_exp_density(_keep(lpd[:, None], 0, 1))

    def close(self):
        self._ctx.close()


class EPPredictor(LaplacePredictor):
    """The same predictive quantities from the expectation-propagation fit
    instead of the Laplace fit: ``mu* = k*^T a``, ``var* = k** - |L^-1 (S^1/2 . k*)|^2`` with the
    EP sites' ``S = diag(tau~)``, ``a`` and ``L = chol(I + S^1/2 K S^1/2)``, ``pi* = Phi(mu* /
    sqrt(1 + var*))`` (Rasmussen & Williams Alg. 3.6). ``quadrature=True`` takes the tilted
    moments by the quadrature rule of DESIGN.md §27; ``likelihood='logit'`` needs it (``pi*`` is
    then the Gauss-Hermite average of sigma, as :class:`LaplacePredictor`'s) and raises
    ``NotImplementedError`` without it. ``damping``, ``diff_tol`` and ``max_sweeps`` are the EP
    settings; the methods are :class:`LaplacePredictor`'s, ``self.n_iter`` holding the sweep
    counts."""

    def __init__(self, X, y, kernel_func, X_test, damping=0.8, diff_tol=1e-8, max_sweeps=100,
                 max_batch=8, device=None, likelihood='probit', quadrature=False):
        if _native.likelihood_code(likelihood) != _native.LIK_PROBIT and not quadrature:
            raise NotImplementedError('expectation propagation is implemented for the probit '
                                      'likelihood only, unless quadrature=True')
        super(EPPredictor, self).__init__(X, y, kernel_func, X_test, max_batch=max_batch,
                                          device=device, likelihood=likelihood)
        self.max_sweeps = int(max_sweeps)
        self._ctx.set_ep(damping, diff_tol, max_sweeps, quadrature=bool(quadrature))

    def __call__(self, thetas, on_error='raise'):
        """``(mean, var, prob)``, each (T, M); a theta whose EP fit fails raises
        ``MaximumIterationsExceededError``, ``LinAlgError`` or ``InvalidCavityError``, or gives
        NaN rows with ``on_error='nan'``."""
        if on_error not in ('raise', 'nan'):
            raise ValueError("on_error must be 'raise' or 'nan'")
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        mean, var, prob, st, nsw = self._ctx.ep_predict(th, self.X_test)
        self.n_iter, self.status = nsw, st
        if on_error == 'raise':
            for s in st:
                raise_for_ep_status(int(s), self.max_sweeps)
        return mean, var, prob

    _joint_approx = _native.JOINT_EP

    def _raise_joint(self, status):
        if status == _native.STATUS_CHOL_C:
            _raise_for_status(status, self._ctx, self.max_sweeps)
        raise_for_ep_status(status, self.max_sweeps)


class ISPredictor(object):
    """Importance-sampling predictive distribution at ``X_test`` (M, D): for each pair
    ``(theta, u)`` the self-normalised average over the importance samples ``f_s = f_post +
    C_chol u_s`` of ``p(y* = 1 | f_s, theta)`` (``prob``), of the conditional latent mean (``mean``)
    and the matching total variance (``var``), with the weights of the IS estimate of
    ``p(y | theta)`` (``apm_is_predict``). Averaged over the states ``(theta, u)``
    of a pseudo-marginal chain, ``prob`` estimates the exact posterior predictive at any fixed
    ``n_imp``: no Gaussian approximation of ``p(f | theta, y)`` is left in it, unlike
    :class:`LaplacePredictor` and :class:`EPPredictor`.

    ``proposal`` is the importance distribution, ``'laplace'`` or ``'ep'`` (with
    ``likelihood='logit'`` the EP proposal needs ``quadrature=True``, DESIGN.md §27, and raises
    ``NotImplementedError`` without it); ``diff_f_tol`` / ``max_iters`` are the
    Newton settings, ``damping`` / ``diff_tol`` / ``max_sweeps`` the EP fit's. ``kernel_func`` must
    be a device kernel (``gpdemo.kernels.make_kernel_func``). The arguments are checked first and
    the device context is created at the first call."""

    def __init__(self, X, y, kernel_func, X_test, n_imp, proposal='laplace', likelihood='probit',
                 max_batch=8, diff_f_tol=1e-4, max_iters=1000, damping=0.8, diff_tol=1e-8,
                 max_sweeps=100, device=None, quadrature=False):
        lik = _native.likelihood_code(likelihood)
        if proposal not in ('laplace', 'ep'):
            raise ValueError("proposal must be 'laplace' or 'ep', got {0!r}".format(proposal))
        if proposal == 'ep' and lik != _native.LIK_PROBIT and not quadrature:
            raise NotImplementedError('expectation propagation is implemented for the probit '
                                      'likelihood only, unless quadrature=True')
        self.likelihood, self.proposal = likelihood, proposal
        self.quadrature = bool(quadrature)
        self._est = _native.EST_IS_EP if proposal == 'ep' else _native.EST_IS
        self._kind, self._eps = _kernel_spec(kernel_func)
        if self._kind == _native.KERNEL_PRECOMPUTED:
            raise NotImplementedError(
                'the device predictor builds the cross-covariance itself and needs one of '
                'gpdemo.kernels.make_kernel_func(...); got {0!r}'.format(kernel_func))
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.X_test = np.ascontiguousarray(X_test, dtype=np.float64)
        if self.X_test.ndim != 2 or self.X_test.shape[1] != self.X.shape[1]:
            raise ValueError('X_test has shape {0}, expected (M, {1})'
                             .format(self.X_test.shape, self.X.shape[1]))
        self.n_imp, self.max_batch = int(n_imp), int(max_batch)
        if self.n_imp < 1 or self.max_batch < 1:
            raise ValueError('n_imp and max_batch must be positive')
        self.kernel_func = kernel_func
        self.max_iters, self.max_sweeps = int(max_iters), int(max_sweeps)
        self._newton = (float(diff_f_tol), int(max_iters))
        self._ep = (float(damping), float(diff_tol), int(max_sweeps))
        self._device = device
        self._ctx = None
        self.status = self.n_cubic_ops = None

    def _context(self):
        if self._ctx is None:
            B = self.max_batch
            ctx = _native.Context(self.X, self.y, self._kind, self._eps, self.n_imp, max_batch=B,
                                  n_slots=B, n_ubufs=B, device=self._device,
                                  likelihood=self.likelihood)
            ctx.set_newton(*self._newton)
            if self._est == _native.EST_IS_EP:
                ctx.set_ep(*self._ep, quadrature=self.quadrature)
            self._ctx = ctx
        return self._ctx

    def _raise(self, status, ctx):
        if self._est == _native.EST_IS_EP and status in (
                _native.STATUS_CHOL_B, _native.STATUS_EP_CAVITY, _native.STATUS_MAXITER):
            raise_for_ep_status(status, self.max_sweeps)
        _raise_for_status(status, ctx, self.max_iters)

    def __call__(self, thetas, us=None, seeds=None, on_error='raise'):
        """``(prob, mean, var, ess, logf)`` for thetas (T, P) or (P,): prob / mean / var (T, M),
        ess and logf (T,). The draws are either ``us``, host arrays (n, n_imp) per theta, or
        ``seeds``, one Philox seed per theta for the device's own normals (``apm_u_normal``,
        counter 0) - exactly one of the two. A theta whose fit fails raises the estimators'
        exception, or gives NaN rows with ``on_error='nan'``; ``self.status`` keeps the codes."""
        if on_error not in ('raise', 'nan'):
            raise ValueError("on_error must be 'raise' or 'nan'")
        if (us is None) == (seeds is None):
            raise ValueError('give exactly one of us (host draws) and seeds (device draws)')
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        T, M = th.shape[0], self.X_test.shape[0]
        if us is not None:
            us = np.asarray(us, dtype=np.float64)
            if us.ndim == 2:
                us = us[None]
            if us.shape != (T, self.X.shape[0], self.n_imp):
                raise ValueError('us has shape {0}, expected {1}'
                                 .format(us.shape, (T, self.X.shape[0], self.n_imp)))
        else:
            seeds = np.atleast_1d(np.asarray(seeds, dtype=np.uint64))
            if seeds.shape != (T,):
                raise ValueError('one seed per theta')
        ctx = self._context()
        prob, mean, var = (np.full((T, M), np.nan) for _ in range(3))
        ess, logf = np.full(T, np.nan), np.full(T, np.nan)
        st = np.zeros(T, dtype=np.int32)
        nops = np.zeros(T, dtype=np.int64)
        for t0 in range(0, T, self.max_batch):
            cnt = min(self.max_batch, T - t0)
            idx = np.arange(cnt, dtype=np.int64)
            if us is not None:
                for i in range(cnt):
                    ctx.u_upload(i, us[t0 + i])
            else:
                ctx.u_normal(idx, seeds[t0:t0 + cnt], np.zeros(cnt, dtype=np.uint64))
            sl = slice(t0, t0 + cnt)
            logf[sl], prob[sl], mean[sl], var[sl], ess[sl], st[sl], nops[sl] = ctx.is_predict(
                self._est, th[sl], idx, idx, self.X_test)
        self.status, self.n_cubic_ops = st, nops
        if on_error == 'raise':
            for s in st:
                self._raise(int(s), ctx)
        return prob, mean, var, ess, logf

    def posterior_average(self, thetas, us=None, seeds=None, burn=0, thin=1, on_error='raise'):
        """Class probabilities (M,) averaged over the kept ``(theta, u)`` states."""
        th, us, seeds = self._kept(thetas, us, seeds, burn, thin)
        return posterior_average(self(th, us, seeds, on_error)[0])

    def log_predictive_density(self, thetas, y_test, us=None, seeds=None, burn=0, thin=1,
                               on_error='raise'):
        """Mean test log predictive density of labels ``y_test`` (M,) in {-1, +1}, from ``prob``
        (``log prob`` for y* = +1, ``log1p(-prob)`` for y* = -1, a log-mean-exp over the states):
        ``mean`` and ``var`` describe the latent value and are not read."""
        th, us, seeds = self._kept(thetas, us, seeds, burn, thin)
        prob = _keep(self(th, us, seeds, on_error)[0], 0, 1)
        return _log_mean_exp_density(
            _log_prob_of_labels(prob, np.asarray(y_test, dtype=np.float64)))

    @staticmethod
    def _kept(thetas, us, seeds, burn, thin):
        k = slice(int(burn), None, int(thin))
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))[k]
        if us is not None:
            us = np.asarray(us, dtype=np.float64)
            us = (us[None] if us.ndim == 2 else us)[k]
        if seeds is not None:
            seeds = np.atleast_1d(np.asarray(seeds, dtype=np.uint64))[k]
        return th, us, seeds

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
