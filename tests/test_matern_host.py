"""Host side of the Matérn covariance kinds: the numpy restatement the device is
compared with (tests/cov_restatement.py) agrees with central differences of its own log
marginal likelihood - which pins the G formulas of the length-scale derivatives before any device
work -, make_kernel_func knows the four names, and the C-ABI declares the four kinds and refuses
an unknown one. No device is needed."""
import os
import re

import numpy as np
import pytest

import cov_restatement as cr
import grad_restatement as gr
from cov_restatement import Cov
from conftest import REPO

EPS = 1e-8
NAMES = {'matern32_iso': 3, 'matern32_ard': 4, 'matern52_iso': 5, 'matern52_ard': 6}


@pytest.mark.parametrize('family', cr.MATERN)
@pytest.mark.parametrize('kind', ['iso', 'ard'])
def test_restatement_vs_central_differences(family, kind):
    """Analytic gradient against central differences (h = 1e-5) of the restatement's own LML at
    a Newton tolerance of 1e-24, (n, d) = (40, 3), theta_0 = 0.3, 3.0, -1.0: 1e-6 of
    max(1, max|fd|), the figure of test_grad_host.py. With S in place of G the length-scale
    entries are off by order one."""
    c = gr.make_case(40, 3, kind, 700)
    for th in c['thetas']:
        ref = cr.laplace_grad(Cov(family, kind), c['X'], c['y'], th, EPS, tol=1e-24)
        fd = gr.central_differences(
            lambda t: cr.lml(Cov(family, kind), c['X'], c['y'], t, EPS, tol=1e-24), th)
        err = np.abs(ref['grad'] - fd).max() / max(1.0, np.abs(fd).max())
        print('matern {0} {1} restatement vs fd, theta_0 {2}: {3:.3e}'
              .format(family, kind, th[0], err))
        assert ref['grad'].shape == (Cov(family, kind).theta_len(3),)
        assert err <= 1e-6


def test_restatement_leaves_grad_restatement_as_it_was():
    """A Matern call leaves the SE results as they were: nothing is substituted anywhere."""
    c = gr.make_case(8, 2, 'ard', 1)
    se = Cov('se', 'ard')

    def se_results():
        ref = cr.laplace_grad(se, c['X'], c['y'], c['thetas'][0], EPS)
        return [se.gram(c['X'], c['thetas'][0], EPS), ref['grad']] + se.dK(c['X'], c['thetas'][0], EPS)
    before = se_results()
    cr.laplace_grad(Cov('32', 'ard'), c['X'], c['y'], c['thetas'][0], EPS)
    assert all(np.array_equal(a, b) for a, b in zip(before, se_results()))


def test_restatement_values_by_hand():
    """Two points at scaled distance r = 2 (tau = 1/2, |x - x'| = 1), s = e^0.5."""
    X = np.array([[0.0], [1.0]])
    th = np.array([0.5, np.log(0.5)])
    s, r = np.exp(0.5), 2.0
    for kind in ('iso', 'ard'):
        K3 = Cov('32', kind).gram(X, th, 1e-3)
        K5 = Cov('52', kind).gram(X, th, 1e-3)
        assert abs(K3[0, 1] - s * (1 + 3 ** 0.5 * r) * np.exp(-3 ** 0.5 * r)) <= 1e-15
        assert abs(K5[0, 1] - s * (1 + 5 ** 0.5 * r + 5.0 / 3.0 * r * r) * np.exp(-5 ** 0.5 * r)) <= 1e-15
        assert K3[0, 0] == s + 1e-3 and K5[1, 1] == s + 1e-3 and np.array_equal(K3, K3.T)
        d3 = Cov('32', kind).dK(X, th, 1e-3)
        d5 = Cov('52', kind).dK(X, th, 1e-3)
        assert len(d3) == 2 and d3[0][0, 0] == s and d3[1][0, 0] == 0.0
        assert abs(d3[1][0, 1] - 3 * s * np.exp(-3 ** 0.5 * r) * r * r) <= 1e-15
        assert abs(d5[1][0, 1] - 5.0 / 3.0 * s * (1 + 5 ** 0.5 * r) * np.exp(-5 ** 0.5 * r) * r * r) <= 1e-15
    assert Cov('32', 'iso').gram_cross(X[:1], X[:1], th)[0, 0] == s  # no epsilon on k*
    with pytest.raises(IndexError):
        Cov('52', 'ard').gram(np.zeros((2, 3)), np.zeros(3), EPS)


def test_make_kernel_func_names_and_kinds():
    import gpdemo.kernels as krn
    from gpdemo import _native
    assert (_native.KERNEL_M32_ISO, _native.KERNEL_M32_ARD, _native.KERNEL_M52_ISO,
            _native.KERNEL_M52_ARD) == (3, 4, 5, 6)
    assert (_native.KERNEL_ISO, _native.KERNEL_ARD, _native.KERNEL_PRECOMPUTED) == (0, 1, 2)
    for name, kind in NAMES.items():
        kf = krn.make_kernel_func(name, 1e-6)
        assert kf.native_kind == kind and kf.epsilon == 1e-6 and callable(kf)
        assert name in repr(kf)
    # the SE callables keep their class, repr and kinds
    for name, kind in (('iso', 0), ('ard', 1)):
        kf = krn.make_kernel_func(name)
        assert isinstance(kf, krn.SEKernelFunc) and kf.native_kind == kind and kf.epsilon == 1e-8
        assert repr(kf) == 'SEKernelFunc({0!r}, epsilon=1e-08)'.format(name)
    for bad in ('matern12_iso', 'matern32', 'se', ''):
        with pytest.raises(ValueError):
            krn.make_kernel_func(bad)
    with pytest.raises(ValueError):
        krn.SEKernelFunc('matern32_iso')
    for fn in ('isotropic_matern32_kernel', 'diagonal_matern32_kernel',
               'isotropic_matern52_kernel', 'diagonal_matern52_kernel'):
        assert fn in krn.__all__ and callable(getattr(krn, fn))


def test_estimators_take_the_device_path_for_a_matern_kernel_func():
    """_kernel_spec reads native_kind / epsilon: no precomputed-K round trip."""
    import gpdemo.kernels as krn
    from gpdemo import _native
    from gpdemo.estimators import _kernel_spec
    assert _kernel_spec(krn.make_kernel_func('matern52_ard', 1e-7)) == (_native.KERNEL_M52_ARD, 1e-7)
    assert _kernel_spec(lambda K, X, theta: None)[0] == _native.KERNEL_PRECOMPUTED


def test_batched_sampler_kernel_names():
    import auxpm.batched as bt
    from gpdemo import _native
    assert bt._KERNEL_KINDS == {'ard': _native.KERNEL_ARD, 'matern32_iso': 3, 'matern32_ard': 4,
                                'matern52_iso': 5, 'matern52_ard': 6}


def test_abi_declares_the_kinds_and_refuses_an_unknown_one():
    """include/apm.h defines the four kinds after the existing three, apm_version says so, and
    apm_create with kind 7 (every other argument valid) fails as an invalid argument: NULL and
    the APM_E_INVALID message, before any device work."""
    from gpdemo import _native
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    defs = dict(re.findall(r'#define\s+(APM_KERNEL_[A-Z0-9_]+)\s+(\d+)', txt))
    assert defs == {'APM_KERNEL_ISO': '0', 'APM_KERNEL_ARD': '1', 'APM_KERNEL_PRECOMPUTED': '2',
                    'APM_KERNEL_M32_ISO': '3', 'APM_KERNEL_M32_ARD': '4',
                    'APM_KERNEL_M52_ISO': '5', 'APM_KERNEL_M52_ARD': '6'}
    lib = _native.load_library(check_device=False)
    assert lib.apm_version() >= 2
    X = np.zeros((2, 1))
    y = np.ones(2)
    for kind in (7, -1, 99):
        h = lib.apm_create(0, kind, X.ctypes.data, 2, 1, 1, y.ctypes.data, 1e-8, 1, 1, 1, 1)
        assert h is None
        assert lib.apm_global_error() == b'apm_create: invalid arguments'
    # the stand-alone builders refuse it the same way (and PRECOMPUTED, which has no formula)
    K = np.zeros((2, 2))
    th = np.zeros(2)
    for kind in (7, 2):
        assert lib.apm_gram(0, kind, X.ctypes.data, 2, 1, 1, th.ctypes.data, 2, 1e-8,
                            K.ctypes.data, 2) == _native.APM_E_INVALID
        assert lib.apm_gram_cross(0, kind, X.ctypes.data, 2, X.ctypes.data, 2, 1, 1,
                                  th.ctypes.data, 2, K.ctypes.data, 2) == _native.APM_E_INVALID
    # a too-short theta for an ARD Matern kind: refused before any device work, too
    X3 = np.zeros((2, 3))
    assert lib.apm_gram(0, 4, X3.ctypes.data, 2, 3, 3, th.ctypes.data, 2, 1e-8, K.ctypes.data,
                        2) == _native.APM_E_INVALID
    assert b'theta too short' in lib.apm_global_error()
