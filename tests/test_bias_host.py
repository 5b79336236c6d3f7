"""The constant (bias) covariance term without a device: the restatement's dK
against central differences, the imbalanced-data study that motivates the term, the names and flags
of the Python layer, the header's define and the C-ABI's refusals."""
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


@pytest.mark.parametrize('family,kind', cr.FAMILY_KINDS)
@pytest.mark.parametrize('log_beta', [-2.0, 1.5])
def test_dk_against_central_differences(family, kind, log_beta):
    """The restatement's gradient (M against the P matrices dK/dtheta_j, the last one beta on
    every pair) against central differences of its own converged LML: 1e-6 of max(1, max|grad|),
    n = 40, d = 3."""
    cov = Cov(family, kind, bias=True)
    c = gr.make_case(40, 3, kind, 300, rows=[(0.3, log_beta)], offset=1.0)
    th = c['thetas'][0]
    assert th.shape[0] == cov.n_base(3) + 1 and th[-1] == log_beta
    ref = cr.laplace_grad(cov, c['X'], c['y'], th, EPS, tol=1e-24)
    fd = gr.central_differences(lambda x: cr.lml(cov, c['X'], c['y'], x, EPS), th)
    err = np.abs(ref['grad'] - fd).max() / max(1.0, np.abs(ref['grad']).max())
    print('bias dK vs fd {0}: {1:.3e}'.format((family, kind, log_beta), err))
    assert err <= 1e-6
    assert ref['grad'][-1] != 0.0
    # the wrong reading (theta_0's weight from K's own entries, S + beta) is told apart
    bad = cr.laplace_grad(cov, c['X'], c['y'], th, EPS, tol=1e-24, wrong='plus_beta')
    assert abs(bad['grad'][0] - fd[0]) > 1e-4 * max(1.0, np.abs(fd).max())


def test_restatement_definition():
    """K = S + beta on the data pairs with s + beta + eps on the diagonal, k* = S* + beta without
    eps, k** = s + beta; a theta of the base kind's length is refused."""
    rng = np.random.RandomState(3)
    X, Xs = rng.normal(size=(7, 3)), rng.normal(size=(4, 3))
    Xs[0] = X[2]
    for family, kind in cr.FAMILY_KINDS:
        cov = Cov(family, kind, bias=True)
        th = np.r_[0.3, rng.normal(size=cov.n_base(3) - 1), 1.5]
        K0 = cov.gram(X, np.r_[th[:-1], -800.0], EPS)
        K = cov.gram(X, th, EPS)
        off = ~np.eye(7, dtype=bool)
        assert np.allclose(K[off], K0[off] + math.exp(1.5), rtol=1e-15, atol=0)
        assert np.all(K.diagonal() == math.exp(0.3) + math.exp(1.5) + EPS)
        Ks = cov.gram_cross(Xs, X, th)
        assert Ks[0, 2] == math.exp(0.3) + math.exp(1.5)
        assert cov.prior_var(Xs, th) == math.exp(0.3) + math.exp(1.5)
        D = cov.dK(X, th, EPS)
        assert len(D) == th.shape[0] and np.all(D[-1] == math.exp(1.5))
        assert np.all(D[0].diagonal() == math.exp(0.3))
        with pytest.raises(IndexError):
            cov.gram(X, th[:-1], EPS)


def _imbalanced_data():
    """RandomState(11), n = 200, d = 2, latent = SE-GP draw + 1.5, labels Bernoulli(Phi(latent))."""
    rng = np.random.RandomState(11)
    X = rng.normal(size=(200, 2))
    K = Cov('se', 'iso').base_S(X, np.zeros(2)) + 1e-8 * np.eye(200)
    f = np.linalg.cholesky(K).dot(rng.normal(size=200)) + 1.5
    y = np.where(rng.uniform(size=200) < ndtr(f), 1.0, -1.0)
    return X, y


def test_constant_term_raises_the_evidence_of_imbalanced_data():
    """The grid maximum of the restated Laplace LML over an 11 x 7 grid of (theta_0, theta_1) with
    log beta = 2 exceeds the one with beta = 0 by more than 1 nat (measured: -50.35 against -52.86,
    2.51 nats, 92 % positive labels)."""
    X, y = _imbalanced_data()
    frac = float((y > 0).mean())
    assert 0.85 <= frac <= 0.95

    cov = Cov('se', 'iso', bias=True)

    def grid_max(log_beta):
        return max(gr.newton(cov.gram(X, np.r_[t0, t1, log_beta], EPS), y, 1e-10)['lml']
                   for t0 in np.linspace(-2.0, 3.0, 11) for t1 in np.linspace(-1.5, 1.5, 7))
    with_bias, without = grid_max(2.0), grid_max(-800.0)
    print('imbalanced data ({0:.0%} positive): grid max LML {1:.2f} with log beta = 2, {2:.2f} '
          'with beta = 0'.format(frac, with_bias, without))
    assert with_bias - without > 1.0


def test_python_names_and_flags():
    """COV_BIAS, native_kind and repr of the kernel callables, the theta lengths of the binding
    and the bias= keyword of every batched sampler - no device."""
    from gpdemo import _native
    import gpdemo.kernels as krn
    import auxpm.batched as bt
    assert _native.COV_BIAS == 16
    for family, kind in cr.FAMILY_KINDS:
        cov, cov0 = Cov(family, kind, bias=True), Cov(family, kind)
        base = krn.make_kernel_func(cov.name, 1e-6)
        biased = krn.make_kernel_func(cov.name, 1e-6, bias=True)
        assert base.native_kind == cov0.native_kind
        assert biased.native_kind == cov.native_kind == base.native_kind | 16
        assert biased.bias is True and base.bias is False and biased.epsilon == 1e-6
        assert 'bias' not in repr(base)
        assert repr(biased) == repr(base)[:-1] + ', bias=True)'
        assert type(biased) is type(base)
        for d in (1, 5):
            assert _native.theta_len(biased.native_kind, d) == cov.n_base(d) + 1
            assert _native.theta_len(base.native_kind, d) == cov.n_base(d)
    assert repr(krn.SEKernelFunc('ard')) == "SEKernelFunc('ard', epsilon=1e-08)"
    assert repr(krn.SEKernelFunc('ard', bias=True)) == "SEKernelFunc('ard', epsilon=1e-08, bias=True)"
    assert inspect.signature(krn.make_kernel_func).parameters['bias'].default is False
    samplers = [c for _, c in inspect.getmembers(bt, inspect.isclass)
                if c.__module__ == bt.__name__ and c.__name__.startswith('Batched')]
    assert len(samplers) >= 6
    for cls in samplers:
        params = inspect.signature(cls.__init__).parameters
        assert 'kernel' in params and params['bias'].default is False, cls.__name__
    assert 16 not in bt._KERNEL_KINDS.values() and all(v < 16 for v in bt._KERNEL_KINDS.values())


def test_abi_declares_the_flag_and_refuses_what_it_should():
    """include/apm.h defines APM_COV_BIAS 16 (not an APM_KERNEL_* name), apm_version stays 3, and
    the flag on PRECOMPUTED, kind 23 and anything above 22 are refused as kind 7 is: apm_create
    NULL with its message, apm_gram / apm_gram_cross APM_E_INVALID; a theta of the base kind's
    length is 'theta too short' - all before any device work."""
    from gpdemo import _native
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    assert re.findall(r'#define\s+APM_COV_BIAS\s+(\d+)', txt) == ['16']
    assert not re.findall(r'#define\s+APM_KERNEL_\w*BIAS', txt)
    lib = _native.load_library(check_device=False)
    assert lib.apm_version() == 3
    X = np.zeros((2, 1))
    y = np.ones(2)
    K = np.zeros((2, 2))
    th = np.zeros(3)
    for kind in (16 | 2, 23, 24, 32, 33, 48, 7, -1, 99):
        h = lib.apm_create(0, kind, X.ctypes.data, 2, 1, 1, y.ctypes.data, 1e-8, 1, 1, 1, 1)
        assert h is None, kind
        assert lib.apm_global_error() == b'apm_create: invalid arguments'
        assert lib.apm_gram(0, kind, X.ctypes.data, 2, 1, 1, th.ctypes.data, 3, 1e-8,
                            K.ctypes.data, 2) == _native.APM_E_INVALID
        assert lib.apm_gram_cross(0, kind, X.ctypes.data, 2, X.ctypes.data, 2, 1, 1,
                                  th.ctypes.data, 3, K.ctypes.data, 2) == _native.APM_E_INVALID
    # every biased kind: a theta of the base kind's length is too short (iso 2, ARD d + 1 = 4)
    X3 = np.zeros((2, 3))
    th4 = np.zeros(4)
    for family, kind in cr.FAMILY_KINDS:
        nk, p0 = Cov(family, kind, bias=True).native_kind, Cov(family, kind).n_base(3)
        assert lib.apm_gram(0, nk, X3.ctypes.data, 2, 3, 3, th4.ctypes.data, p0, 1e-8,
                            K.ctypes.data, 2) == _native.APM_E_INVALID
        assert b'apm_gram: theta too short' in lib.apm_global_error()
        assert lib.apm_gram_cross(0, nk, X3.ctypes.data, 2, X3.ctypes.data, 2, 3, 3,
                                  th4.ctypes.data, p0, K.ctypes.data, 2) == _native.APM_E_INVALID
        assert b'apm_gram_cross: theta too short' in lib.apm_global_error()
