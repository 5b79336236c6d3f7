"""The linear (dot-product) covariance term without a device: the restatement's dK
against central differences, the trend study that motivates the term, the names and flags of the
Python layer, the header's define and the C-ABI's refusals."""
import inspect
import math
import os
import re

import numpy as np
import pytest
from scipy.special import ndtr

import cov_restatement as cr
import grad_restatement as gr
from cov_restatement import Cov

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-8


@pytest.mark.parametrize('kind,bias', cr.LINEAR_KINDS)
@pytest.mark.parametrize('log_lambda', [-2.0, 1.0])
def test_dk_against_central_differences(kind, bias, log_lambda):
    """The restatement's gradient (M against the P matrices dK/dtheta_j, the last one
    lambda x_i . x_j) against central differences of its own converged LML: 1e-6 of
    max(1, max|grad|) (test_bias_host's bound), n = 40, d = 3."""
    cov = Cov('se', kind, bias, linear=True)
    c = gr.make_case(40, 3, kind, 300, rows=[(0.3, 1.5, log_lambda) if bias else (0.3, log_lambda)])
    th = c['thetas'][0]
    assert th.shape[0] == cov.theta_len(3) and th[-1] == log_lambda
    assert (not bias) or th[-2] == 1.5
    ref = cr.laplace_grad(cov, c['X'], c['y'], th, EPS, tol=1e-24)
    fd = gr.central_differences(lambda x: cr.lml(cov, c['X'], c['y'], x, EPS), th)
    err = np.abs(ref['grad'] - fd).max() / max(1.0, np.abs(ref['grad']).max())
    print('linear dK vs fd {0}: {1:.3e}'.format((kind, bias, log_lambda), err))
    assert err <= 1e-6
    assert ref['grad'][-1] != 0.0


def test_restatement_definition():
    """K = S [+ beta] + lambda x x^T on the data pairs with (s [+ beta]) + lambda |x_i|^2 + eps on
    the diagonal, k* without eps, k** per test row; with lambda = 0 the kind without the flag; a
    theta one entry short is refused."""
    rng = np.random.RandomState(3)
    X, Xs = rng.normal(size=(7, 3)), rng.normal(size=(4, 3))
    Xs[0] = X[2]
    lam = math.exp(1.0)
    for kind, bias in cr.LINEAR_KINDS:
        cov = Cov('se', kind, bias, linear=True)
        beta = math.exp(1.5) if bias else 0.0
        th = np.r_[0.3, rng.normal(size=cov.n_base(3) - 1), [1.5] if bias else [], 1.0]
        assert th.shape[0] == cov.theta_len(3)
        th0 = np.r_[th[:-1], -800.0]
        K0 = cov.gram(X, th0, EPS)
        if bias:
            assert np.array_equal(K0, Cov('se', kind, bias=True).gram(X, th[:-1], EPS))
        else:
            Kb = Cov('se', kind).gram(X, th[:-1], EPS)
            off = ~np.eye(7, dtype=bool)
            assert np.array_equal(K0[off], Kb[off])
            assert np.all(K0.diagonal() == math.exp(0.3) + EPS)
        K = cov.gram(X, th, EPS)
        assert np.allclose(K - K0, lam * X.dot(X.T), rtol=1e-13, atol=1e-14)
        assert np.array_equal(K, K.T)
        assert np.allclose(K.diagonal(), math.exp(0.3) + beta + lam * (X * X).sum(1) + EPS,
                           rtol=1e-15, atol=0)
        Ks = cov.gram_cross(Xs, X, th)
        assert abs(Ks[0, 2] - (math.exp(0.3) + beta + lam * X[2].dot(X[2]))) <= 1e-14 * Ks[0, 2]
        kss = cov.prior_var(Xs, th)
        assert kss.shape == (4,) and abs(kss[0] - Ks[0, 2]) <= 1e-14 * kss[0]
        D = cov.dK(X, th, EPS)
        assert len(D) == th.shape[0] and np.allclose(D[-1], lam * X.dot(X.T), rtol=1e-15)
        assert np.all(D[0].diagonal() == math.exp(0.3))
        if bias:
            assert np.all(D[-2] == math.exp(1.5))
        with pytest.raises(IndexError):
            cov.gram(X, th[:-1], EPS)


def _trend_data():
    """RandomState(5), n = 200, d = 2, latent = SE-GP draw (s = 1, tau = 1) + 2 x_0 - x_1, labels
    Bernoulli(Phi(latent))."""
    rng = np.random.RandomState(5)
    X = rng.normal(size=(200, 2))
    K = Cov('se', 'iso').base_S(X, np.zeros(2)) + 1e-8 * np.eye(200)
    f = np.linalg.cholesky(K).dot(rng.normal(size=200)) + 2.0 * X[:, 0] - X[:, 1]
    y = np.where(rng.uniform(size=200) < ndtr(f), 1.0, -1.0)
    return X, y


def test_linear_term_raises_the_evidence_of_data_with_a_trend():
    """The grid maximum of the restated Laplace LML over a 6 x 5 grid of (theta_0, theta_1) with
    log lambda = 1 exceeds the one with lambda = 0 (the sign only is asserted; DESIGN.md §25 holds
    the measured gap)."""
    X, y = _trend_data()

    cov = Cov('se', 'iso', linear=True)

    def grid_max(log_lambda):
        return max(gr.newton(cov.gram(X, np.r_[t0, t1, log_lambda], EPS), y, 1e-10)['lml']
                   for t0 in np.linspace(-2.0, 3.0, 6) for t1 in np.linspace(-1.0, 1.0, 5))
    with_linear, without = grid_max(1.0), grid_max(-800.0)
    print('data with a trend: grid max LML {0:.2f} with log lambda = 1, {1:.2f} with lambda = 0'
          .format(with_linear, without))
    assert with_linear > without


def test_python_names_and_flags():
    """COV_LINEAR, native_kind and repr of the kernel callables, the theta lengths of the binding,
    the refusal of linear=True on a Matern name and the linear= keyword of every batched sampler -
    no device."""
    from gpdemo import _native
    import gpdemo.kernels as krn
    import auxpm.batched as bt
    assert _native.COV_LINEAR == 64
    for kind, bias in cr.LINEAR_KINDS:
        base = krn.make_kernel_func(kind, 1e-6, bias=bias)
        lin = krn.make_kernel_func(kind, 1e-6, bias=bias, linear=True)
        cov = Cov('se', kind, bias, linear=True)
        assert lin.native_kind == cov.native_kind == base.native_kind | 64
        assert lin.native_kind in (64, 65, 80, 81)
        assert lin.linear is True and base.linear is False and lin.bias is bias
        assert 'linear' not in repr(base)
        assert repr(lin) == repr(base)[:-1] + ', linear=True)'
        for d in (1, 5):
            assert _native.theta_len(lin.native_kind, d) == cov.theta_len(d)
            assert _native.theta_len(base.native_kind, d) == cov.theta_len(d) - 1
    for name in ('matern32_iso', 'matern32_ard', 'matern52_iso', 'matern52_ard', 'nonsense'):
        with pytest.raises(ValueError):
            krn.make_kernel_func(name, 1e-8, linear=True)
    with pytest.raises(ValueError):
        krn.make_kernel_func('matern52_ard', 1e-8, bias=True, linear=True)
    assert inspect.signature(krn.make_kernel_func).parameters['linear'].default is False
    samplers = [c for _, c in inspect.getmembers(bt, inspect.isclass)
                if c.__module__ == bt.__name__ and c.__name__.startswith('Batched')]
    assert len(samplers) >= 6
    for cls in samplers:
        params = inspect.signature(cls.__init__).parameters
        assert params['linear'].default is False, cls.__name__


def test_abi_declares_the_flag_and_refuses_what_it_should():
    """include/apm.h defines APM_COV_LINEAR 64 (not an APM_KERNEL_* name), apm_version stays 3,
    the flag on PRECOMPUTED, on the four Matern kinds and with bit 5 is refused as kind 7 is
    (apm_create NULL with its message, apm_gram / apm_gram_cross APM_E_INVALID), what
    test_bias_host lists stays refused, and a theta of length P - 1 is 'theta too short' for each
    of the four kinds - all before any device work."""
    from gpdemo import _native
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    assert re.findall(r'#define\s+APM_COV_LINEAR\s+(\d+)', txt) == ['64']
    assert not re.findall(r'#define\s+APM_KERNEL_\w*LINEAR', txt)
    lib = _native.load_library(check_device=False)
    assert lib.apm_version() == 3
    X = np.zeros((2, 1))
    y = np.ones(2)
    K = np.zeros((2, 2))
    th = np.zeros(4)
    refused = [64 | k for k in (2, 3, 4, 5, 6, 32)] + [64 | 16 | k for k in (2, 3, 4, 5, 6)]
    refused += [16 | 2, 23, 24, 32, 33, 48, 7, -1, 99, 128, 64 | 128]
    for kind in refused:
        h = lib.apm_create(0, kind, X.ctypes.data, 2, 1, 1, y.ctypes.data, 1e-8, 1, 1, 1, 1)
        assert h is None, kind
        assert lib.apm_global_error() == b'apm_create: invalid arguments'
        assert lib.apm_gram(0, kind, X.ctypes.data, 2, 1, 1, th.ctypes.data, 4, 1e-8,
                            K.ctypes.data, 2) == _native.APM_E_INVALID, kind
        assert lib.apm_gram_cross(0, kind, X.ctypes.data, 2, X.ctypes.data, 2, 1, 1,
                                  th.ctypes.data, 4, K.ctypes.data, 2) == _native.APM_E_INVALID
    # each of the four kinds: a theta of length P - 1 is too short (d = 3)
    X3 = np.zeros((2, 3))
    th6 = np.zeros(6)
    for kind, bias in cr.LINEAR_KINDS:
        cov = Cov('se', kind, bias, linear=True)
        nk, P = cov.native_kind, cov.theta_len(3)
        assert nk in (64, 65, 80, 81)
        assert lib.apm_gram(0, nk, X3.ctypes.data, 2, 3, 3, th6.ctypes.data, P - 1, 1e-8,
                            K.ctypes.data, 2) == _native.APM_E_INVALID
        assert b'apm_gram: theta too short' in lib.apm_global_error()
        assert lib.apm_gram_cross(0, nk, X3.ctypes.data, 2, X3.ctypes.data, 2, 3, 3,
                                  th6.ctypes.data, P - 1, K.ctypes.data, 2) == _native.APM_E_INVALID
        assert b'apm_gram_cross: theta too short' in lib.apm_global_error()
