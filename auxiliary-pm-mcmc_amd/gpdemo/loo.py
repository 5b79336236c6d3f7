# -*- coding: utf-8 -*-
"""Leave-one-out cross-validation of the GP classifier at its training points, on the GPU.

For a state ``(theta, u)`` of a pseudo-marginal chain the importance samples ``f_s = f_post +
C_chol u_s`` and their self-normalised weights ``wbar_s`` give per training point

    ``loo_i = -log sum_s wbar_s / p(y_i | f_si)``,   ``lpd_i = log sum_s wbar_s p(y_i | f_si)``

(``apm_is_loo``). The identity ``p(y_i | y_-i) = 1 / E[1 / p(y_i | f_i) | y]`` makes
``exp(-loo_i)``, averaged over the states of a run, a consistent estimate of the exact
leave-one-out density: no Gaussian approximation of ``p(f | theta, y)`` enters, unlike the cavity
value ``gauss_i`` that the same call returns for comparison (Vehtari et al. 2016). The reference
has no such function; the sums run in libapm.so and only theta, u and the rows cross the host
boundary.

:class:`ISLeaveOneOut` evaluates given ``(theta, u)`` pairs; :func:`combine_loo` turns the rows of
a run into the model-comparison criterion and needs no device.
"""
import numpy as np
from scipy.special import logsumexp

from . import _native
from .estimators import _kernel_spec, _raise_for_status
from .latent_posterior_approximations import raise_for_ep_status
from .predict import _keep

__all__ = ['ISLeaveOneOut', 'combine_loo']


def combine_loo(loo, lpd, burn=0, thin=1, khat=None):
    """The chain-level criterion from per-state rows ``loo`` and ``lpd`` (T, n), kept samples
    ``burn::thin``. The identity averages ``1 / p`` over the states, so

        ``loo_i = -log mean_t exp(-loo_it)``,   ``lpd_i = log mean_t exp(lpd_it)``

    (both by logsumexp). Returns a dict with ``elpd_loo = sum_i loo_i``, its standard error
    ``se = sqrt(n var_i loo_i)``, ``p_loo = sum_i lpd_i - elpd_loo`` (the effective number of
    parameters) and the pointwise arrays ``loo`` and ``lpd`` (n,).

    ``loo`` may as well be the Pareto-smoothed rows ``loo_psis``, which have the same form. With
    their per-state shapes ``khat`` (T, n) the dict gains ``khat`` (n,), the per-point mean over
    the kept states (NaN entries, states whose tail could not be fitted, are ignored; NaN where
    no state has a value), and ``n_bad``, the number of points whose mean exceeds 0.7: their
    ``loo`` is not to be trusted (Vehtari et al. 2024)."""
    lo, lp = _keep(loo, burn, thin), _keep(lpd, burn, thin)
    if lo.shape != lp.shape:
        raise ValueError('loo has shape {0}, lpd {1}'.format(lo.shape, lp.shape))
    T, n = lo.shape
    loo_i = -(logsumexp(-lo, axis=0) - np.log(T))
    lpd_i = logsumexp(lp, axis=0) - np.log(T)
    elpd = float(loo_i.sum())
    out = dict(elpd_loo=elpd, se=float(np.sqrt(n * np.var(loo_i))),
               p_loo=float(lpd_i.sum()) - elpd, loo=loo_i, lpd=lpd_i)
    if khat is not None:
        kh = _keep(khat, burn, thin)
        if kh.shape != lo.shape:
            raise ValueError('khat has shape {0}, loo {1}'.format(kh.shape, lo.shape))
        seen = np.isfinite(kh)
        cnt = seen.sum(axis=0)
        mean = np.where(seen, kh, 0.0).sum(axis=0) / np.maximum(cnt, 1)
        out['khat'] = np.where(cnt > 0, mean, np.nan)
        out['n_bad'] = int((out['khat'] > 0.7).sum())
    return out


class ISLeaveOneOut(object):
    """Leave-one-out predictive densities at the training points ``(X, y)`` for pairs
    ``(theta, u)``, shaped like :class:`gpdemo.predict.ISPredictor`.

    ``proposal`` is the importance distribution, ``'laplace'`` or ``'ep'`` (under
    ``likelihood='logit'`` the EP proposal needs ``quadrature=True``);
    ``diff_f_tol`` / ``max_iters`` are the Newton settings, ``damping`` / ``diff_tol`` /
    ``max_sweeps`` the EP fit's. ``kernel_func`` must be a device kernel
    (``gpdemo.kernels.make_kernel_func``). The arguments are checked first and the device context
    is created at the first call."""

    def __init__(self, X, y, kernel_func, n_imp, proposal='laplace', likelihood='probit',
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
                'the device builds the covariance itself and needs one of '
                'gpdemo.kernels.make_kernel_func(...); got {0!r}'.format(kernel_func))
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        if self.X.ndim != 2 or self.y.shape != (self.X.shape[0],):
            raise ValueError('X has shape {0}, y {1}: expected (N, D) and (N,)'
                             .format(self.X.shape, self.y.shape))
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

    def __call__(self, thetas, us=None, seeds=None, on_error='raise', psis=False):
        """For thetas (T, P) or (P,): a dict with ``loo``, ``lpd``, ``ess_loo`` and ``gauss``
        (T, n), ``ess`` and ``logf`` (T,) and ``status`` (T,). The draws are either ``us``, host
        arrays (n, n_imp) per theta, or ``seeds``, one Philox seed per theta for the device's own
        normals (``apm_u_normal``, counter 0) - exactly one of the two. Each batch runs the
        theta-call and then ``apm_is_loo`` on the slots it wrote. A theta whose fit fails raises
        the estimators' exception, or gives NaN rows with ``on_error='nan'``.

        With ``psis=True`` each batch also runs ``apm_is_loo_psis`` and the dict
        gains ``loo_psis`` and ``khat`` (T, n), the Pareto-smoothed densities and the Pareto shape
        of each point's ratios (above 0.7: distrust ``loo`` at that point; NaN: the tail was too
        short to fit and ``loo_psis`` is ``loo``), and ``khat_w`` (T,), the shape of the weights
        themselves. The other entries are bitwise what they are without it."""
        if on_error not in ('raise', 'nan'):
            raise ValueError("on_error must be 'raise' or 'nan'")
        if (us is None) == (seeds is None):
            raise ValueError('give exactly one of us (host draws) and seeds (device draws)')
        th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        T, n = th.shape[0], self.X.shape[0]
        if us is not None:
            us = np.asarray(us, dtype=np.float64)
            if us.ndim == 2:
                us = us[None]
            if us.shape != (T, n, self.n_imp):
                raise ValueError('us has shape {0}, expected {1}'
                                 .format(us.shape, (T, n, self.n_imp)))
        else:
            seeds = np.atleast_1d(np.asarray(seeds, dtype=np.uint64))
            if seeds.shape != (T,):
                raise ValueError('one seed per theta')
        ctx = self._context()
        out = {k: np.full((T, n), np.nan) for k in ('loo', 'lpd', 'ess_loo', 'gauss')}
        out.update(ess=np.full(T, np.nan), logf=np.full(T, np.nan))
        if psis:
            out.update(loo_psis=np.full((T, n), np.nan), khat=np.full((T, n), np.nan),
                       khat_w=np.full(T, np.nan))
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
            _, st[sl], nops[sl] = ctx.theta_eval(self._est, th[sl], idx, idx)
            (out['logf'][sl], out['loo'][sl], out['lpd'][sl], out['ess_loo'][sl],
             out['gauss'][sl], out['ess'][sl], _) = ctx.is_loo(idx, idx)
            if psis:
                _, out['loo_psis'][sl], out['khat'][sl], out['khat_w'][sl], _, _ = \
                    ctx.is_loo_psis(idx, idx)
        self.status, self.n_cubic_ops = st, nops
        out['status'] = st
        if on_error == 'raise':
            for s in st:
                self._raise(int(s), ctx)
        return out

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
