"""Host side of expectation propagation: the C-ABI / Python surface without a
device, and the numpy restatement the device is compared with (tests/ep_restatement.py) checked
against independent routes - sequential EP, the exact n = 1 value, grid quadrature of a 2 x 2
problem, and the damping-independence of the fixed point."""
import math
import os
import re

import numpy as np
from scipy.special import ndtr
from scipy.stats import multivariate_normal

import ep_restatement as ep
from conftest import REPO

EP_SYMBOLS = ('apm_set_ep', 'apm_ep_eval', 'apm_ep_predict', 'apm_ep')


def _se_case(n, d, theta0, seed):
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) > 0, 1.0, -1.0)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return math.exp(theta0) * np.exp(-0.5 * D / d) + 1e-8 * np.eye(n), y


def test_header_declares_the_ep_entry_points():
    """Fails without the feature: the header lines are new."""
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    assert re.search(r'#define\s+APM_STATUS_EP_CAVITY\s+6\b', txt)
    n_args = {'apm_set_ep': 4, 'apm_ep_eval': 12, 'apm_ep_predict': 13, 'apm_ep': 18}
    for name, k in n_args.items():
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', txt)
        assert m, name
        assert len(m.group(1).split(',')) == k, name


def test_library_exports_and_binds_the_ep_entry_points():
    """Fails without the feature: the symbols and bindings are new. apm_version() stays 3."""
    from gpdemo import _native
    syms = _native.exported_symbols()
    lib = _native.load_library(check_device=False)
    for name in EP_SYMBOLS:
        assert name in syms and hasattr(lib, name)
    assert lib.apm_version() == 3
    assert _native.STATUS_EP_CAVITY == 6
    for name in ('set_ep', 'ep', 'ep_predict'):
        assert callable(getattr(_native.Context, name))
    import gpdemo.estimators as est
    import gpdemo.latent_posterior_approximations as lpa
    import gpdemo.predict as prd
    assert issubclass(lpa.InvalidCavityError, Exception) and callable(lpa.ep_approximation)
    assert callable(est.LogMarginalLikelihoodEPEstimator) and callable(prd.EPPredictor)


def test_argument_checks_come_before_any_device_call():
    from gpdemo import _native
    lib = _native.load_library(check_device=False)
    bad = _native.APM_E_INVALID
    one = np.ones(4)
    st = np.zeros(1, dtype=np.int32)
    assert lib.apm_set_ep(None, 0.8, 1e-8, 100) == bad
    assert lib.apm_ep_eval(None, 1, one.ctypes.data, 2, None, None, None, None, None, 1,
                           st.ctypes.data, None) == bad
    assert lib.apm_ep_predict(None, 1, one.ctypes.data, 2, one.ctypes.data, 1, 1, None, None,
                              None, 1, st.ctypes.data, None) == bad

    def ep_call(n, ldk, damping, diff_tol, max_sweeps):
        return lib.apm_ep(0, one.ctypes.data, n, ldk, one.ctypes.data, 0, damping, diff_tol,
                          max_sweeps, None, None, None, None, None, n, None, None, st.ctypes.data)
    assert ep_call(2, 1, 0.8, 1e-8, 100) == bad     # ldk < n
    assert ep_call(2, 2, 0.0, 1e-8, 100) == bad     # damping outside (0, 1]
    assert ep_call(2, 2, 1.5, 1e-8, 100) == bad
    assert ep_call(2, 2, 0.8, -1.0, 100) == bad     # diff_tol < 0
    assert ep_call(2, 2, 0.8, 1e-8, 0) == bad       # max_sweeps < 1


def test_logit_is_refused_by_the_python_classes_before_any_device_call():
    import gpdemo.estimators as est
    import gpdemo.kernels as krn
    import gpdemo.predict as prd
    import pytest
    X, y = np.zeros((3, 2)), np.ones(3)
    kf = krn.make_kernel_func('ard', 1e-8)
    with pytest.raises(NotImplementedError):
        est.LogMarginalLikelihoodEPEstimator(X, y, kf, likelihood='logit')
    with pytest.raises(NotImplementedError):
        prd.EPPredictor(X, y, kf, X, likelihood='logit')


def test_parallel_fixed_point_equals_sequential_ep():
    """n = 40, diff_tol = 1e-22: tau~, nu~ and mu of the parallel scheme against R&W Alg. 3.5
    within 1e-9 (the CPU study measured 3e-12 and 7e-12)."""
    K, y = _se_case(40, 2, 0.7, 0)
    par = ep.ep_fit(K, y, diff_tol=1e-22, max_sweeps=1000)
    tau, nu, mu = ep.ep_sequential(K, y)
    errs = [np.abs(par[k] - v).max() for k, v in (('tau', tau), ('nu', nu), ('mu', mu))]
    print('parallel vs sequential EP (tau, nu, mu):', errs, 'sweeps', par['n_sweeps'])
    assert max(errs) <= 1e-9


def test_single_point_gives_log_half():
    for k, yy in ((1.7, 1.0), (0.2, -1.0), (400.0, 1.0)):
        fit = ep.ep_fit(np.array([[k]]), np.array([yy]))
        assert abs(fit['logz'] - math.log(0.5)) <= 1e-14


def test_two_points_against_grid_quadrature():
    """A fixed 2 x 2 K: log Z_EP within 1e-3 of the evidence int Phi(y1 f1) Phi(y2 f2) N(f|0,K) df
    on a grid. 1e-3 bounds EP's own approximation error (3e-4 in the CPU study)."""
    K = np.array([[2.0, 1.2], [1.2, 1.5]])
    y = np.array([1.0, -1.0])
    g = np.linspace(-12.0, 12.0, 1201)
    F1, F2 = np.meshgrid(g, g, indexing='ij')
    pdf = multivariate_normal(np.zeros(2), K).pdf(np.stack([F1, F2], -1))
    Z = (ndtr(y[0] * F1) * ndtr(y[1] * F2) * pdf).sum() * (g[1] - g[0]) ** 2
    fit = ep.ep_fit(K, y)
    print('2x2: log Z_EP {0:.8f} quadrature {1:.8f}'.format(fit['logz'], math.log(Z)))
    assert abs(fit['logz'] - math.log(Z)) <= 1e-3


def test_fixed_point_does_not_depend_on_the_damping():
    """delta = 0.5 and delta = 1 against delta = 0.8 at diff_tol = 1e-20: each run stops once mu
    moves by less than 1e-10 (rms) per sweep, so with a contraction rate up to ~0.99 per sweep it
    is within ~1e-8 of the fixed point: the bound, relative to max(1, max|value|); log Z_EP is
    stationary in the sites at the fixed point, so its error is second order: 1e-10."""
    K, y = _se_case(40, 2, 0.7, 0)
    ref = ep.ep_fit(K, y, damping=0.8, diff_tol=1e-20, max_sweeps=2000)
    for d in (0.5, 1.0):
        fit = ep.ep_fit(K, y, damping=d, diff_tol=1e-20, max_sweeps=2000)
        for k in ('tau', 'nu', 'mu'):
            assert np.abs(fit[k] - ref[k]).max() <= 1e-8 * max(1.0, np.abs(ref[k]).max())
        assert abs(fit['logz'] - ref['logz']) <= 1e-10
