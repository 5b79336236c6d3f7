# -*- coding: utf-8 -*-
"""Gram builders on the GPU: the squared-exponential kernels that replace the reference's Cython
kernels.pyx, and the Matérn 3/2 and 5/2 families beside them.

Every function keeps the reference signature ``f(K, X, theta, epsilon=1e-8)`` and fills the
caller-owned ``K`` in place (kernels.pyx:12-49, :52-90); ``theta`` entries beyond the ones the
kernel reads are ignored and a too-short ``theta`` raises ``IndexError`` as the bounds-checked
Cython does. :func:`make_kernel_func` returns the ``kernel_func(K, X, theta)`` callable the
estimators expect; the estimators recognise it and build K directly in device memory instead of
round-tripping it through the host.

With ``s = exp(theta[0])``, ``tau_k = exp(theta[k+1])`` (ARD) or ``exp(theta[1])`` for every k
(isotropic) and ``r = sqrt(sum_k ((x_ik - x_jk) / tau_k)^2)``::

    squared exponential   s exp(-r^2 / 2)
    Matérn 3/2            s (1 + sqrt(3) r) exp(-sqrt(3) r)
    Matérn 5/2            s (1 + sqrt(5) r + 5/3 r^2) exp(-sqrt(5) r)

plus ``epsilon`` on the diagonal (one point set's Gram only).

``bias=True`` adds a constant term to any of the six: ``K = S + beta 1 1^T + epsilon I`` with
``beta = exp(theta[-1])`` one more, last entry of ``theta`` - a N(0, beta) prior on a constant
offset of the latent function, integrated out. The cross-covariance gains ``beta`` as well and
the prior variance at a test point is ``s + beta``.

``linear=True`` ('iso' and 'ard' only, with or without ``bias``) adds the linear term
``lambda X X^T`` on the raw (unscaled) inputs, ``lambda = exp(theta[-1])`` one more, last entry -
a N(0, lambda I) prior on the weights of a linear function of the inputs, integrated out; with
both, ``beta = exp(theta[-2])``. The cross-covariance gains ``lambda x* . x`` and the prior
variance at a test point is ``s [+ beta] + lambda |x*|^2``.
"""
from . import _native

__all__ = ['isotropic_squared_exponential_kernel', 'diagonal_squared_exponential_kernel',
           'isotropic_matern32_kernel', 'diagonal_matern32_kernel',
           'isotropic_matern52_kernel', 'diagonal_matern52_kernel',
           'make_kernel_func', 'SEKernelFunc', 'MaternKernelFunc']


def isotropic_squared_exponential_kernel(K, X, theta, epsilon=1e-8):
    """K[i,j] = exp(theta[0]) exp(-|x_i - x_j|^2 / (2 exp(theta[1])^2)) + epsilon [i == j]."""
    _native.gram(_native.KERNEL_ISO, K, X, theta, epsilon)


def diagonal_squared_exponential_kernel(K, X, theta, epsilon=1e-8):
    """K[i,j] = exp(theta[0]) exp(-1/2 sum_k ((x_ik - x_jk) / exp(theta[k+1]))^2) + eps [i == j]."""
    _native.gram(_native.KERNEL_ARD, K, X, theta, epsilon)


def isotropic_matern32_kernel(K, X, theta, epsilon=1e-8):
    """Matérn 3/2 with one length scale exp(theta[1]), + epsilon [i == j]."""
    _native.gram(_native.KERNEL_M32_ISO, K, X, theta, epsilon)


def diagonal_matern32_kernel(K, X, theta, epsilon=1e-8):
    """Matérn 3/2 with a length scale exp(theta[k+1]) per feature (ARD), + epsilon [i == j]."""
    _native.gram(_native.KERNEL_M32_ARD, K, X, theta, epsilon)


def isotropic_matern52_kernel(K, X, theta, epsilon=1e-8):
    """Matérn 5/2 with one length scale exp(theta[1]), + epsilon [i == j]."""
    _native.gram(_native.KERNEL_M52_ISO, K, X, theta, epsilon)


def diagonal_matern52_kernel(K, X, theta, epsilon=1e-8):
    """Matérn 5/2 with a length scale exp(theta[k+1]) per feature (ARD), + epsilon [i == j]."""
    _native.gram(_native.KERNEL_M52_ARD, K, X, theta, epsilon)


class SEKernelFunc(object):
    """``kernel_func(K, X, theta)`` for the isotropic ('iso') or ARD ('ard') SE kernel."""

    def __init__(self, kind, epsilon=1e-8, bias=False, linear=False):
        if kind not in ('iso', 'ard'):
            raise ValueError("kind must be 'iso' or 'ard'")
        self.kind = kind
        self.epsilon = float(epsilon)
        self.bias = bool(bias)
        self.linear = bool(linear)
        self.native_kind = _native.KERNEL_ISO if kind == 'iso' else _native.KERNEL_ARD
        if self.bias:
            self.native_kind |= _native.COV_BIAS
        if self.linear:
            self.native_kind |= _native.COV_LINEAR

    def __call__(self, K, X, theta):
        _native.gram(self.native_kind, K, X, theta, self.epsilon)

    def __repr__(self):
        return 'SEKernelFunc({0!r}, epsilon={1!r}{2}{3})'.format(
            self.kind, self.epsilon, ', bias=True' if self.bias else '',
            ', linear=True' if self.linear else '')


_MATERN_KINDS = {'matern32_iso': _native.KERNEL_M32_ISO, 'matern32_ard': _native.KERNEL_M32_ARD,
                 'matern52_iso': _native.KERNEL_M52_ISO, 'matern52_ard': _native.KERNEL_M52_ARD}


class MaternKernelFunc(object):
    """``kernel_func(K, X, theta)`` for 'matern32_iso', 'matern32_ard', 'matern52_iso' or
    'matern52_ard'. Like :class:`SEKernelFunc` it carries ``native_kind`` and ``epsilon``, which
    is what sends the estimators, ``LaplacePredictor`` and ``LaplaceGradient`` down the device
    path."""

    def __init__(self, kind, epsilon=1e-8, bias=False):
        if kind not in _MATERN_KINDS:
            raise ValueError('kind must be one of {0}'.format(sorted(_MATERN_KINDS)))
        self.kind = kind
        self.epsilon = float(epsilon)
        self.bias = bool(bias)
        self.native_kind = _MATERN_KINDS[kind] | (_native.COV_BIAS if self.bias else 0)

    def __call__(self, K, X, theta):
        _native.gram(self.native_kind, K, X, theta, self.epsilon)

    def __repr__(self):
        return 'MaternKernelFunc({0!r}, epsilon={1!r}{2})'.format(
            self.kind, self.epsilon, ', bias=True' if self.bias else '')


def make_kernel_func(kind, epsilon=1e-8, bias=False, linear=False):
    """'iso' | 'ard' (SE) or 'matern32_iso' | 'matern32_ard' | 'matern52_iso' | 'matern52_ard';
    bias=True adds the constant term exp(theta[-1]) (theta has one more entry); linear=True
    ('iso' and 'ard' only) the linear term exp(theta[-1]) x x^T (one more entry again, the last;
    the constant term's is then theta[-2])."""
    if linear and kind not in ('iso', 'ard'):
        raise ValueError("linear=True needs kind 'iso' or 'ard'")
    if kind in _MATERN_KINDS:
        return MaternKernelFunc(kind, epsilon, bias)
    if kind in ('iso', 'ard'):
        return SEKernelFunc(kind, epsilon, bias, linear)
    raise ValueError("kind must be 'iso', 'ard' or one of {0}".format(sorted(_MATERN_KINDS)))
