"""Host side of the gradient of log Z_EP: the C-ABI / Python surface without a
device, and the numpy restatement the device is compared with (tests/ep_grad_restatement.py)
checked against central differences of its own log Z_EP, the iso / ARD identity, the epsilon rule
and the error the class default stop tolerance leaves."""
import os
import re

import numpy as np
import pytest

import cov_restatement as cr
import grad_restatement as gr
from cov_restatement import Cov
from conftest import REPO

EPS = 1e-8
# (n, d, kind, seed), each at theta_0 = 0.3, 3, -1, 6 (grad_restatement.make_case)
SHAPES = [(65, 4, 'ard', 401), (130, 5, 'ard', 402), (200, 3, 'iso', 403)]
SIGMAS = (0.3, 3.0, -1.0, 6.0)
CONVERGED = dict(diff_tol=1e-22, max_sweeps=2000)
# EPGradient's default stop tolerance, and ten times the worst error of the gradient it leaves
# against the diff_tol = 1e-22 fit over SHAPES x SIGMAS, relative to max(1, max|grad|): 1.9e-8
# measured. The restatement is deterministic; the factor covers library and BLAS
# differences.
DEFAULT_TOL_BOUND = 10 * 1.9e-8


@pytest.fixture(scope='module')
def cases():
    """Data and the converged restatement gradient per shape and theta, computed once."""
    out = []
    for n, d, kind, seed in SHAPES:
        c = gr.make_case(n, d, kind, seed, rows=SIGMAS)
        c['ref'] = [cr.ep_grad(Cov('se', kind), c['X'], c['y'], th, EPS, **CONVERGED) for th in c['thetas']]
        out.append(c)
    return out


def test_header_declares_apm_ep_grad():
    """Fails without the feature: the header lines are new."""
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    m = re.search(r'\bint\s+apm_ep_grad\s*\(([^)]*)\)', txt)
    assert m
    assert len(m.group(1).split(',')) == 9


def test_library_exports_and_binds_apm_ep_grad():
    """Fails without the feature: the symbol, the binding and the class are new. apm_version()
    stays 3."""
    from gpdemo import _native
    lib = _native.load_library(check_device=False)
    assert 'apm_ep_grad' in _native.exported_symbols() and hasattr(lib, 'apm_ep_grad')
    assert lib.apm_version() == 3
    assert callable(_native.Context.ep_grad)
    import gpdemo.gradients as gd
    assert 'EPGradient' in gd.__all__
    for name in ('__call__', 'log_posterior', 'maximise', 'close'):
        assert callable(getattr(gd.EPGradient, name))
    # one L-BFGS driver for both evidences: the two classes share their base
    assert gd.EPGradient.__mro__[1] is gd.LaplaceGradient.__mro__[1] is not object


def test_argument_checks_come_before_any_device_call():
    from gpdemo import _native
    import gpdemo.gradients as gd
    import gpdemo.kernels as krn
    lib = _native.load_library(check_device=False)
    one = np.ones(4)
    st = np.zeros(1, dtype=np.int32)
    assert lib.apm_ep_grad(None, 1, one.ctypes.data, 2, None, one.ctypes.data, 2, st.ctypes.data,
                           None) == _native.APM_E_INVALID
    X, y = np.zeros((3, 2)), np.ones(3)
    with pytest.raises(NotImplementedError):
        gd.EPGradient(X, y, krn.make_kernel_func('ard', 1e-8), likelihood='logit')
    with pytest.raises(NotImplementedError):
        gd.EPGradient(X, y, lambda K, X, theta: None)
    with pytest.raises(ValueError):
        gd.EPGradient(X, y, krn.make_kernel_func('ard', 1e-8), likelihood='cauchy')


def _fd_error(kind, X, y, theta, family, grad):
    fd = gr.central_differences(
        lambda th: cr.ep_logz(Cov(family, kind), X, y, th, EPS, **CONVERGED), theta)
    return np.abs(grad - fd).max() / max(1.0, np.abs(fd).max())


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_analytic_against_central_differences(cases, ci):
    """The restatement's gradient at diff_tol = 1e-22 against central differences (h = 1e-5) of
    its own log Z_EP, to 1e-6 of max(1, max|fd|) (test_gpu_grad's finite-difference bound; the
    worst measured here is 6.9e-9, the finite-difference error itself)."""
    c = cases[ci]
    for th, ref in zip(c['thetas'], c['ref']):
        err = _fd_error(c['kind'], c['X'], c['y'], th, 'se', ref['grad'])
        print('EP grad vs fd shape {0} theta_0 {1}: {2:.3e} (max|grad| {3:.3e}, {4} sweeps)'
              .format(SHAPES[ci][:3], th[0], err, np.abs(ref['grad']).max(), ref['n_sweeps']))
        assert err <= 1e-6


def test_analytic_against_central_differences_matern52():
    c = gr.make_case(65, 4, 'ard', 404, rows=(0.3,))
    th = c['thetas'][0]
    ref = cr.ep_grad(Cov('52', 'ard'), c['X'], c['y'], th, EPS, **CONVERGED)
    err = _fd_error('ard', c['X'], c['y'], th, '52', ref['grad'])
    print('EP grad vs fd Matern 5/2 (65, 4, ard): {0:.3e}'.format(err))
    assert err <= 1e-6


def test_iso_equals_ard_with_equal_length_scales(cases):
    """grad_iso[0] == grad_ard[0] and grad_iso[1] == sum grad_ard[1:], to 1e-12 of the summands'
    size (test_gpu_grad's bound): the same K and M, the features' sums added in another order.
    Both sides are fitted on the iso Gram. The oracle's two C Grams differ in their last bit
    (2.8e-16 of max|K|), and a fit driven to diff_tol = 1e-22 stops on rounding noise: at
    theta_0 = 6 the ARD Gram's fit stops one sweep earlier (47 against 48), which moves grad[0] by
    7.5e-12. That is the fit's noise floor, not the identity under test."""
    c = cases[2]
    assert c['kind'] == 'iso'
    for th, iso in zip(c['thetas'], c['ref']):
        th_ard = np.r_[th[0], np.full(c['d'], th[1])]
        ard = cr.ep_grad(Cov('se', 'ard'), c['X'], c['y'], th_ard, EPS,
                         K=Cov('se', 'iso').gram(c['X'], th, EPS), **CONVERGED)
        assert ard['n_sweeps'] == iso['n_sweeps']
        scale = max(1.0, np.abs(ard['grad'][1:]).sum())
        assert abs(iso['grad'][0] - ard['grad'][0]) <= 1e-12 * max(1.0, abs(ard['grad'][0]))
        assert abs(iso['grad'][1] - ard['grad'][1:].sum()) <= 1e-12 * scale


def test_epsilon_is_not_in_the_gradient():
    """epsilon = 1e-2: the gradient with dK/dtheta_0 = S matches central differences of log Z_EP
    (theta does not move the jitter), and the reading that keeps epsilon on dK/dtheta_0's diagonal
    is off by more than 1e-6."""
    c = gr.make_case(130, 5, 'ard', 402, rows=(0.3, -1.0))
    for th in c['thetas']:
        ref = cr.ep_grad(Cov('se', 'ard'), c['X'], c['y'], th, 1e-2, **CONVERGED)
        wrong = cr.ep_grad(Cov('se', 'ard'), c['X'], c['y'], th, 1e-2, wrong='eps_in_dk0', **CONVERGED)
        fd = gr.central_differences(
            lambda t: cr.ep_logz(Cov('se', 'ard'), c['X'], c['y'], t, 1e-2, **CONVERGED), th)
        scale = max(1.0, np.abs(fd).max())
        off = np.abs(ref['grad'] - wrong['grad']).max() / scale
        print('epsilon rule theta_0 {0}: fd error {1:.3e}, wrong reading off by {2:.3e}'
              .format(th[0], np.abs(ref['grad'] - fd).max() / scale, off))
        assert np.abs(ref['grad'] - fd).max() <= 1e-6 * scale
        assert off > 1e-6
        assert np.array_equal(ref['grad'][1:], wrong['grad'][1:])


def test_class_default_tolerance(cases):
    """EPGradient's default diff_tol against the converged fit on every shape and theta."""
    import inspect
    import gpdemo.gradients as gd
    sig = inspect.signature(gd.EPGradient.__init__).parameters
    settings = dict(damping=sig['damping'].default, diff_tol=sig['diff_tol'].default,
                    max_sweeps=sig['max_sweeps'].default)
    assert settings == dict(damping=0.8, diff_tol=1e-16, max_sweeps=1000)
    worst = 0.0
    for ci, c in enumerate(cases):
        for th, ref in zip(c['thetas'], c['ref']):
            got = cr.ep_grad(Cov('se', c['kind']), c['X'], c['y'], th, EPS, **settings)
            err = np.abs(got['grad'] - ref['grad']).max() / max(1.0, np.abs(ref['grad']).max())
            print('default diff_tol shape {0} theta_0 {1}: {2:.3e} ({3} of {4} sweeps)'
                  .format(SHAPES[ci][:3], th[0], err, got['n_sweeps'], ref['n_sweeps']))
            worst = max(worst, err)
    print('default diff_tol: worst {0:.3e} (bound {1:.1e})'.format(worst, DEFAULT_TOL_BOUND))
    assert worst <= DEFAULT_TOL_BOUND
