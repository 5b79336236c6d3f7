# -*- coding: utf-8 -*-
"""Estimators of log p(y | theta, X) for GP classification (probit or logit likelihood),
evaluated on the MI355X.

Drop-in for the reference's ``gpdemo/estimators.py``: the three classes keep their constructor
arguments, ``__call__`` signatures, return values, ``n_cubic_ops`` accounting and exceptions.
The work runs in libapm.so (include/apm.h) in fp64 (Gram, Newton/Laplace, Cholesky factors)
with the importance-sampling product L.U in fp32 MFMA. ``likelihood=`` (not in
the reference, which has the probit only) selects ``'probit'`` (default) or ``'logit'``
(DESIGN.md §15).

``cached_results`` / ``K_chol`` become :class:`DeviceCache` handles: opaque references to a
device-resident cache slot that is released when the handle is garbage-collected. Passing one
back skips the O(N^3) work exactly as the reference's tuple does.
"""
import numpy as np

from . import _native
from .latent_posterior_approximations import (MaximumIterationsExceededError,
                                              raise_for_ep_status)

__all__ = ['LogMarginalLikelihoodLaplaceEstimator', 'LogMarginalLikelihoodEPEstimator',
           'InvalidCovarianceMatrixError',
           'LogMarginalLikelihoodApproxPosteriorISEstimator',
           'LogMarginalLikelihoodPriorMCEstimator', 'DeviceCache', 'DeviceInvariantError',
           'n_imp_curve', 'select_n_imp', 'tune_n_imp']

_UBUF = 0  # single-chain estimators upload each call's draws into this device buffer


class InvalidCovarianceMatrixError(Exception):
    """Raised when the posterior approximation's covariance is not positive definite."""


class DeviceInvariantError(RuntimeError):
    """A device-side invariant of the theta-call failed (APM_STATUS_GUARD): the
    estimate is withheld rather than returned. No reference counterpart (the reference has no
    device); a sampler treats it like any other failed estimator call."""


class DeviceCache(object):
    """Handle to the per-theta state kept on the device (replaces the reference's
    ``(K_chol, C_chol, f_post)`` tuple / ``K_chol`` array). Iterating an IS cache reads the
    state back as that tuple (reference estimators.py:166-176) for inspection; the samplers only
    pass the handle back. The slot keeps C_chol and f_post; L_K = chol(K) is consumed by the
    posterior factor on the device, so iterating refactors K on the device
    (a PriorMC theta-call into a scratch slot) — all three factors are read back rounded to fp32
    like the slot itself. That refactor runs once per handle (memoised): an O(N^3) device call,
    so unpacking the tuple is not free the first time. ``numpy.asarray`` is defined for a PriorMC
    handle only (the reference's K_chol array); an IS handle is a tuple, not an array."""

    __slots__ = ('_ctx', 'slot', 'kind', '_owner', '_theta', '_kchol', '__weakref__')

    def __init__(self, ctx, slot, kind, owner=None, theta=None):
        self._ctx = ctx
        self.slot = slot
        self.kind = kind
        self._owner = owner  # the estimator (its kernel_func / X) for the K_chol refactor
        self._theta = None if theta is None else np.array(theta, dtype=np.float64)
        self._kchol = None

    def __del__(self):
        try:
            self._ctx.slots.release(self.slot)
        except Exception:
            pass

    def read(self):
        """(factor (n, n) lower, f_post (n,), g (n,), const) — factor rounded to fp32."""
        return self._ctx.slot_read(self.slot)

    def k_chol(self):
        """chol(K(theta)) (n, n) lower, computed on the device (fp32-rounded read-back)."""
        if self.kind == _native.EST_PRIORMC:
            return self.read()[0]
        if self._kchol is not None:  # a fresh array per call, as the reference's tuple element
            return self._kchol.copy()
        if self._owner is None or self._theta is None:
            raise ValueError('this cache does not record its theta')
        tmp = self._ctx.slots.acquire()
        try:
            _, st, _ = self._owner._theta_call(_native.EST_PRIORMC, self._ctx, self._theta,
                                               _UBUF, tmp)
            _raise_for_status(int(st[0]), self._ctx)
            self._kchol = self._ctx.slot_read(tmp)[0]
            return self._kchol.copy()
        finally:
            self._ctx.slots.release(tmp)

    def __iter__(self):
        L, f, _, _ = self.read()
        if self.kind == _native.EST_PRIORMC:  # the reference's K_chol is the array itself
            return iter(L)
        return iter((self.k_chol(), L, f))

    def __array__(self, dtype=None, copy=None):
        if self.kind != _native.EST_PRIORMC:
            raise TypeError('an importance-sampling cache is the tuple (K_chol, C_chol, f_post), '
                            'not an array: unpack it')
        L = self.read()[0]
        return L if dtype is None else L.astype(dtype)


def _kernel_spec(kernel_func):
    kind = getattr(kernel_func, 'native_kind', None)
    if kind is None:
        return _native.KERNEL_PRECOMPUTED, 1e-8
    return kind, getattr(kernel_func, 'epsilon', 1e-8)


def _raise_for_status(status, ctx, n_iter_cap=1000):
    if status == _native.STATUS_OK:
        return
    if status == _native.STATUS_CHOL_C:
        raise InvalidCovarianceMatrixError(
            'Posterior covariance matrix not PSD: sum of negative eigenvalues nan '
            '(Cholesky of C failed on the device)')
    if status == _native.STATUS_GUARD:
        raise DeviceInvariantError('a device-side invariant of the theta-call failed '
                                   '(apm_guard_read gives the residuals)')
    if status == _native.STATUS_MAXITER:
        raise MaximumIterationsExceededError('Failed to converge in {0} iterations'
                                             .format(n_iter_cap))
    what = 'K' if status == _native.STATUS_CHOL_K else 'B'
    raise np.linalg.LinAlgError('{0}-th leading minor not positive definite (Cholesky of {1} '
                                'on the device)'.format('?', what))


class _Problem(object):
    """Device contexts for one (X, y, kernel) problem, created lazily per number of draws."""

    def __init__(self, X, y, kernel_func, n_slots=8, likelihood='probit'):
        _native.likelihood_code(likelihood)
        self.likelihood = likelihood
        self.X = X
        self.y = np.asarray(y, dtype=np.float64)
        self.kind, self.eps = _kernel_spec(kernel_func)
        self.n_slots = n_slots
        self._ctxs = {}

    @property
    def device_gram(self):
        return self.kind != _native.KERNEL_PRECOMPUTED

    def ctx(self, n_imp):
        c = self._ctxs.get(n_imp)
        if c is None:
            c = _native.Context(self.X, self.y, self.kind, self.eps, n_imp, max_batch=1,
                                n_slots=self.n_slots, n_ubufs=1, likelihood=self.likelihood)
            self._ctxs[n_imp] = c
        return c


class _EstimatorBase(object):
    def __init__(self, X, y, kernel_func, likelihood='probit'):
        self.X = X
        self.y = y
        self.kernel_func = kernel_func
        self.likelihood = likelihood
        self._prob = _Problem(X, y, kernel_func, likelihood=likelihood)  # (ValueError if unknown)
        self._K = None if self._prob.device_gram else np.empty((X.shape[0], X.shape[0]))
        self.n_cubic_ops = 0
        _native.load_library()  # fail loudly here, not at the first call

    def reset_cubic_op_count(self):
        """Reset the count of executed ops with order ``n_data**3`` cost."""
        self.n_cubic_ops = 0

    def _theta_call(self, est, ctx, theta, ubuf, slot):
        if self._prob.device_gram:
            return ctx.theta_eval(est, np.atleast_1d(theta)[None], [ubuf], [slot])
        self.kernel_func(self._K, self.X, theta)
        return ctx.theta_eval_K(est, self._K, ubuf, slot)


def _spread_result(logf, ess, wmax, block, n_cubic_ops):
    """One block length's replicates (each (n_rep, nblk)) as spread() returns them."""
    return {'log_estimates': logf, 'sd': float(np.std(logf, ddof=1)) if logf.size > 1 else np.nan,
            'ess': ess, 'wmax': wmax, 'block': int(block), 'n_cubic_ops': int(n_cubic_ops)}


def _require_quadrature(likelihood, quadrature):
    """EP's closed-form tilted moments are the probit's: NotImplementedError for another
    likelihood unless the moments come by quadrature (before any device call)."""
    if _native.likelihood_code(likelihood) != _native.LIK_PROBIT and not quadrature:
        raise NotImplementedError('expectation propagation is implemented for the probit '
                                  'likelihood only, unless quadrature=True')


def _check_spread_args(n_imp, n_rep, blocks):
    """ValueError for what apm_is_spread would refuse, before any device call."""
    if n_imp is None or int(n_imp) < 1:
        raise ValueError('n_imp is not known: pass n_imp=, or call the estimator once first')
    if int(n_rep) < 1:
        raise ValueError('n_rep = {0} < 1'.format(n_rep))
    for b in blocks:
        if not 1 <= int(b) <= int(n_imp):
            raise ValueError('block = {0} outside [1, n_imp = {1}]'.format(b, n_imp))
        if int(n_rep) * (int(n_imp) // int(b)) > _native.SPREAD_MAX_BLOCKS:
            raise ValueError('n_rep * (n_imp // block) above {0}'.format(_native.SPREAD_MAX_BLOCKS))


class _SpreadMixin(object):
    """Replicate spread of the estimators that average over draws u."""

    _spread_est = None  # the theta-call's APM_EST_*
    _last_n_imp = None  # the number of draws of the last __call__ (spread's default n_imp)

    def _spread_raise(self, status, ctx):
        _raise_for_status(status, ctx)

    def _spread_blocks(self, theta, n_rep, blocks, seed=0, n_imp=None):
        """One theta-call, then apm_is_spread per block length on the same draws (the Philox
        stream (seed, 0 .. n_rep - 1), in the context's one U buffer - scratch between calls)."""
        n_imp = self._last_n_imp if n_imp is None else n_imp
        blocks = [n_imp if b is None else b for b in blocks]
        _check_spread_args(n_imp, n_rep, blocks)
        ctx = self._prob.ctx(int(n_imp))
        if self._spread_est == _native.EST_IS_EP:
            ctx.set_ep(*self.ep_settings, quadrature=self.quadrature)
        ctx.u_normal([_UBUF], [seed], [0])
        slot = ctx.slots.acquire()
        try:
            _, st, nops = self._theta_call(self._spread_est, ctx, theta, _UBUF, slot)
            self._spread_raise(int(st[0]), ctx)
            self.n_cubic_ops += int(nops[0])
            res = []
            for b in blocks:
                logf, ess, wmax, st = ctx.is_spread([slot], [_UBUF], [seed], [0], n_rep, b)
                _raise_for_status(int(st[0]), ctx)
                res.append(_spread_result(logf[0], ess[0], wmax[0], b, nops[0]))
        finally:
            ctx.slots.release(slot)
        return res

    def spread(self, theta, n_rep=32, block=None, seed=0, n_imp=None):
        """How noisy the log-estimate is at `theta`: one theta-call, then `n_rep` independent
        redraws of u on the device, each cut into blocks of `block` samples (None: n_imp, one
        block per replicate). Returns a dict: ``log_estimates`` (n_rep, nblk), one estimate per
        block; ``sd``, their standard deviation (ddof = 1 over all of them) - the spread of an
        estimator that uses `block` samples; ``ess`` and ``wmax`` (n_rep, nblk), each block's
        weight ESS (sum w)^2 / sum w^2 and largest normalised weight; ``block``; ``n_cubic_ops``
        of the theta-call. `n_imp` defaults to that of the estimator's last call. The draws are
        the Philox stream (seed, 0 .. n_rep - 1): the same for every block length."""
        return self._spread_blocks(theta, n_rep, [block], seed, n_imp)[0]


def n_imp_curve(estimator, theta, n_rep=32, seed=0, n_imp=None):
    """``estimator.spread`` at `theta` for every block length 64 * 2^k <= n_imp, and n_imp
    itself, on the same draws and one theta-call: ``{block: spread dict}``, ascending."""
    n_imp = getattr(estimator, '_last_n_imp', None) if n_imp is None else n_imp
    _check_spread_args(n_imp, n_rep, [])
    blocks = []
    b = 64
    while b <= n_imp:
        blocks.append(b)
        b *= 2
    if n_imp not in blocks:
        blocks.append(int(n_imp))
    res = estimator._spread_blocks(theta, n_rep, blocks, seed, n_imp)
    return dict(zip(blocks, res))


def select_n_imp(curves, target_sd=1.0):
    """The smallest block length present in every curve (``n_imp_curve`` dicts) whose ``sd`` is
    at most `target_sd` in every one of them, or None when no measured length is. A NaN sd does
    not meet the target."""
    if not curves:
        return None
    common = set(curves[0])
    for c in curves[1:]:
        common &= set(c)
    for b in sorted(common):
        if all(c[b]['sd'] <= target_sd for c in curves):
            return b
    return None


def tune_n_imp(estimator, thetas, target_sd=1.0, n_rep=32, seed=0, n_imp=None):
    """The number of importance samples that keeps the standard deviation of the log-estimate at
    or below `target_sd` (the pseudo-marginal rule of thumb is about one) at every row of
    `thetas`: ``(curves, block)`` with ``curves[t] = n_imp_curve(estimator, thetas[t], n_rep)``
    and ``block`` the smallest measured block length that meets the target at every theta - or
    None when even n_imp does not.

    Nothing is extrapolated beyond n_imp. Where the target is missed the weights are degenerate
    (a handful of effective samples), and there the spread falls much slower than 1 / sqrt(N):
    with the Laplace proposal at a large signal variance (theta_0 = 3, n = 130) the sd at N = 64,
    128, 256 was measured as 1.66, 1.44, 1.28 where 1 / sqrt(N) scaling from N = 64 predicts
    1.17 and 0.83. An extrapolated N would be far too small exactly when it is needed; raise
    n_imp (or change the proposal) and measure again."""
    curves = [n_imp_curve(estimator, th, n_rep, seed, n_imp) for th in np.atleast_2d(thetas)]
    return curves, select_n_imp(curves, target_sd)


class LogMarginalLikelihoodLaplaceEstimator(_EstimatorBase):
    """Deterministic (biased) Laplace-approximation estimate of log p(y | theta, X)
    (reference estimators.py:19-82)."""

    def __call__(self, theta):
        ctx = self._prob.ctx(1)
        out, st, nops = self._theta_call(_native.EST_LAPLACE, ctx, theta, _UBUF, 0)
        _raise_for_status(int(st[0]), ctx)
        self.n_cubic_ops += int(nops[0])
        return float(out[0])


class LogMarginalLikelihoodEPEstimator(_EstimatorBase):
    """Deterministic (biased) expectation-propagation estimate ``log Z_EP`` of
    log p(y | theta, X) for the probit likelihood. No reference counterpart; the
    call signature is the Laplace estimator's, so it can stand wherever that one does (e.g. as
    the deterministic target of PM-MH). ``n_cubic_ops`` grows by 2 per sweep, one factorisation
    and one matrix triangular solve: the project's own accounting. ``damping``, ``diff_tol`` and
    ``max_sweeps`` are the EP settings. ``quadrature=True`` takes the tilted moments by the
    quadrature rule of DESIGN.md §27 instead of the probit's closed form; ``likelihood='logit'``
    needs it and raises ``NotImplementedError`` without it."""

    def __init__(self, X, y, kernel_func, likelihood='probit', damping=0.8, diff_tol=1e-8,
                 max_sweeps=100, quadrature=False):
        _require_quadrature(likelihood, quadrature)
        super(LogMarginalLikelihoodEPEstimator, self).__init__(X, y, kernel_func, likelihood)
        self.ep_settings = (float(damping), float(diff_tol), int(max_sweeps))
        self.quadrature = bool(quadrature)
        self.n_sweeps = None

    def __call__(self, theta):
        if self._prob.device_gram:
            ctx = self._prob.ctx(1)
            ctx.set_ep(*self.ep_settings, quadrature=self.quadrature)
            logz, _, _, _, _, st, nsw = ctx.ep(np.atleast_1d(theta)[None])
            logz, st, nsw = float(logz[0]), int(st[0]), int(nsw[0])
        else:
            self.kernel_func(self._K, self.X, theta)
            # (a K of the caller's: apm_ep_lik, the probit's closed form or the logit's rule)
            logz, nsw, st = _native.ep(self._K, self.y, False, *self.ep_settings,
                                       likelihood=self.likelihood)[5:]
        raise_for_ep_status(st, self.ep_settings[2])
        self.n_sweeps = nsw
        self.n_cubic_ops += 2 * nsw
        return logz


class LogMarginalLikelihoodApproxPosteriorISEstimator(_SpreadMixin, _EstimatorBase):
    """Unbiased importance-sampling estimate of p(y | theta, X) with the Laplace posterior as
    proposal (reference estimators.py:90-241). ``ns``: (n_data, n_imp_sample) N(0,1) draws.

    With ``post_approx_func=ep_approximation`` the proposal is the posterior of the converged
    expectation-propagation fit instead (``EST_IS_EP`` theta-calls, DESIGN.md §17;
    ``likelihood='logit'`` needs ``quadrature=True``, the tilted moments by the rule of DESIGN.md
    §27, and raises ``NotImplementedError`` without it). ``damping``, ``diff_tol`` and
    ``max_sweeps`` are that fit's settings; ``n_cubic_ops`` then grows by two per sweep plus the
    estimator's own three."""

    def __init__(self, X, y, kernel_func, post_approx_func, likelihood='probit', damping=0.8,
                 diff_tol=1e-8, max_sweeps=100, quadrature=False):
        _native.likelihood_code(likelihood)
        name = getattr(post_approx_func, '__name__', '')
        if not (getattr(post_approx_func, 'apm_fused', False) or
                name == 'laplace_approximation'):
            raise NotImplementedError(
                'the device estimator fuses the Laplace approximation or the EP approximation '
                '(gpdemo.latent_posterior_approximations.laplace_approximation / '
                'ep_approximation); got {0!r}'.format(post_approx_func))
        self._est = _native.EST_IS_EP if name == 'ep_approximation' else _native.EST_IS
        if self._est == _native.EST_IS_EP:
            _require_quadrature(likelihood, quadrature)
        super(LogMarginalLikelihoodApproxPosteriorISEstimator, self).__init__(
            X, y, kernel_func, likelihood)
        self.post_approx_func = post_approx_func
        self.ep_settings = (float(damping), float(diff_tol), int(max_sweeps))
        self.quadrature = bool(quadrature)
        self._spread_est = self._est

    def _spread_raise(self, status, ctx):
        self._raise(status, ctx)

    def _raise(self, status, ctx):
        if self._est == _native.EST_IS_EP and status in (
                _native.STATUS_CHOL_B, _native.STATUS_EP_CAVITY, _native.STATUS_MAXITER):
            raise_for_ep_status(status, self.ep_settings[2])
        _raise_for_status(status, ctx)

    def __call__(self, ns, theta=None, cached_results=None):
        if theta is None and cached_results is None:
            raise ValueError('One of theta or cached_results must be provided')
        ns = np.asarray(ns, dtype=np.float64)
        self._last_n_imp = ns.shape[1]
        if cached_results is None:
            ctx = self._prob.ctx(ns.shape[1])
            if self._est == _native.EST_IS_EP:
                ctx.set_ep(*self.ep_settings, quadrature=self.quadrature)
            ctx.u_upload(_UBUF, ns)
            slot = ctx.slots.acquire()
            cache = DeviceCache(ctx, slot, self._est, self, theta)
            out, st, nops = self._theta_call(self._est, ctx, theta, _UBUF, slot)
            self._raise(int(st[0]), ctx)
            self.n_cubic_ops += int(nops[0])
            return float(out[0]), cache
        ctx = cached_results._ctx
        if ns.shape[1] != ctx.n_imp:
            raise ValueError('cached results were computed for {0} importance samples, got {1}'
                             .format(ctx.n_imp, ns.shape[1]))
        ctx.u_upload(_UBUF, ns)
        out, st = ctx.u_eval([cached_results.slot], [_UBUF])
        _raise_for_status(int(st[0]), ctx)
        return float(out[0]), cached_results


class LogMarginalLikelihoodPriorMCEstimator(_SpreadMixin, _EstimatorBase):
    """Unbiased simple Monte Carlo estimate of p(y | theta, X) with draws from the GP prior
    (reference estimators.py:244-325). Returns ``(log_estimate, K_chol)``; ``K_chol`` is a
    :class:`DeviceCache`."""

    _spread_est = _native.EST_PRIORMC

    def __call__(self, ns, theta=None, K_chol=None):
        if theta is None and K_chol is None:
            raise ValueError('One of theta or K_chol must be provided')
        ns = np.asarray(ns, dtype=np.float64)
        self._last_n_imp = ns.shape[1]
        if K_chol is None:
            ctx = self._prob.ctx(ns.shape[1])
            ctx.u_upload(_UBUF, ns)
            slot = ctx.slots.acquire()
            cache = DeviceCache(ctx, slot, _native.EST_PRIORMC, self, theta)
            out, st, nops = self._theta_call(_native.EST_PRIORMC, ctx, theta, _UBUF, slot)
            _raise_for_status(int(st[0]), ctx)
            self.n_cubic_ops += int(nops[0])
            return float(out[0]), cache
        ctx = K_chol._ctx
        ctx.u_upload(_UBUF, ns)
        out, st = ctx.u_eval([K_chol.slot], [_UBUF])
        _raise_for_status(int(st[0]), ctx)
        return float(out[0]), K_chol
