"""Host side of the logistic likelihood: the numpy restatement the device is
compared with (tests/logit_restatement.py) is checked against itself - gradient against central
differences of its LML, the consistent importance-sampling form against the reference's direct
one - the committed Gauss-Hermite table against the 400-node rule, and the C-ABI / Python
surface without a device."""
import math
import os
import re

import numpy as np
import pytest

import grad_restatement as gr
import logit_restatement as lr
from cov_restatement import Cov
from conftest import REPO

EPS = 1e-8


def test_restated_gradient_vs_central_differences():
    """n = 40, d = 3 (SE ARD), theta_0 = 0.3, 3.0, -1.0: the formula of include/apm.h with the
    logit's g and d3 against central differences (h = 1e-5) of the restated LML, relative to
    max(1, max|fd|). A wrong sign or a factor of 2 in d3 misses either bound by five orders.
      * Newton tolerance 1e-12: the formula is the derivative at the exact mode, while the LML
        keeps the W and L of the iteration before its last step (lpa.py:103-106), a first-order
        error in that step, |f_new - f| <= sqrt(1e-12) = 1e-6 per point, which the differences
        differentiate: bound 10 sqrt(tol) = 1e-5 (measured 6.9e-7, 1.4e-8, 4.4e-10);
      * Newton tolerance 1e-24 (to convergence): 1e-6, the bound of test_grad_host's probit twin -
        the differences' own error is h^2 |LML'''| / 6 + u |LML| / h ~ 1e-10 + 1e-9."""
    c = gr.make_case(40, 3, 'ard', 40)
    for tol, bound in ((1e-12, 1e-5), (1e-24, 1e-6)):
        for th in c['thetas']:
            K = Cov('se', 'ard').gram(c['X'], th, EPS)
            ref = lr.laplace_grad(K, Cov('se', 'ard').dK(c['X'], th, EPS, K=K), c['y'], tol=tol)
            fd = lr.central_differences(
                lambda t: lr.lml(Cov('se', 'ard').gram(c['X'], t, EPS), c['y'], tol=tol), th)
            err = np.abs(ref['grad'] - fd).max() / max(1.0, np.abs(fd).max())
            print('logit restatement vs fd, Newton tol {0:g}, theta_0 {1}: {2:.3e} (max|fd| '
                  '{3:.3e})'.format(tol, th[0], err, np.abs(fd).max()))
            assert err <= bound
    # (the probit's restatement at the same theta is another function altogether)
    th = c['thetas'][0]
    K = Cov('se', 'ard').gram(c['X'], th, EPS)
    assert abs(gr.newton(K, c['y'], 1e-12)['lml'] - lr.lml(K, c['y'], 1e-12)) > 1e-3


def test_consistent_is_form_equals_the_direct_one():
    """n = 30: log p(y|f) + log N(f|0, K) - log N(f|f_post, C) at f_s = f_post + chol(C) u_s
    against the form the device evaluates with the same factor. The two differ by
    the rounding of the quadratic forms, ~1e-16 x cond(K) x |f|^2: 1e-6 at epsilon = 1e-8 would be
    the honest bound, so the check runs at epsilon = 1e-4 (cond(K) <= 2e5 at sigma = e^3), where
    1e-9 relative to max(1, |value|) holds with orders to spare (measured: at most 1.0e-13)."""
    c = gr.make_case(30, 3, 'ard', 30)
    ns = np.random.RandomState(3).normal(size=(30, 64))
    for th in c['thetas']:
        K = Cov('se', 'ard').gram(c['X'], th, 1e-4)
        st = lr.is_state(K, c['y'])
        direct, C_chol = lr.is_direct(K, c['y'], st, ns)
        cons = lr.is_consistent(c['y'], st, ns, C_chol)
        own = lr.is_consistent(c['y'], st, ns)  # chol(C) by the device's route
        print('logit IS forms theta_0 {0}: direct {1:.12f} consistent {2:.12f} ({3:.2e}), '
              'push-through factor {4:.2e}'.format(th[0], direct, cons, abs(direct - cons),
                                                   abs(own - cons)))
        assert abs(direct - cons) <= 1e-9 * max(1.0, abs(direct))
        assert abs(own - cons) <= 1e-9 * max(1.0, abs(direct))
    # PriorMC is the same form with W = z = 0 and chol(K) as the factor
    K = Cov('se', 'ard').gram(c['X'], c['thetas'][0], 1e-4)
    zero = dict(f=np.zeros(30), W=np.zeros(30), a=np.zeros(30), logdet_B=0.0,
                C_chol=np.linalg.cholesky(K))
    assert abs(lr.priormc(K, c['y'], ns) - lr.is_consistent(c['y'], zero, ns)) <= 1e-12


def test_committed_quadrature_table_within_bound():
    """The table k_predict_reduce<LOGIT> sums (csrc/gh_table.h), through the kernel's own
    pairing, against the 400-node rule on mu* in [-30, 30] x sigma*^2 in [1e-6, e^6]: within 1e-7
    absolute. Q = 400 is the smallest count that meets this bound (399 nodes are 9.5e-4 away, 398
    3.0e-5: tools/make_gh_table.py --study), so the table IS the 400-node rule, less the 272
    outer nodes whose weights sum to 2.8e-24; the measured maximum is rounding, 4.4e-16."""
    x, w = lr.committed_table()
    assert np.all(np.diff(x) > 0) and x[0] > 0 and np.all(w > 0)
    assert abs(2.0 * w.sum() - 1.0) <= 1e-15
    mu = np.linspace(-30.0, 30.0, 121)
    var = np.exp(np.linspace(math.log(1e-6), 6.0, 57))
    MU, VAR = np.meshgrid(mu, var, indexing='ij')
    got = lr.table_average(MU, VAR, x, w)
    ref = lr.logistic_normal(MU, VAR, 400)
    err = np.abs(got - ref).max()
    print('quadrature table vs 400-node rule: max {0:.3e} over {1} grid points'
          .format(err, MU.size))
    assert err <= lr.GH_BOUND
    # the properties the device relies on: 0.5 bitwise at mu = 0 whatever the variance, sigma(mu)
    # at var <= 0, a relative lower tail
    assert np.all(lr.table_average(np.zeros(57), var, x, w) == 0.5)
    m = np.array([-3.0, 0.7])
    assert np.allclose(lr.table_average(m, np.array([0.0, -1.0]), x, w),
                       1.0 / (1.0 + np.exp(-m)), rtol=1e-15, atol=0)
    tail = lr.table_average(np.array([-40.0]), np.array([1.0]), x, w)[0]
    assert abs(tail / math.exp(-40.0 + 0.5) - 1.0) <= 1e-12  # E sigma(x) -> e^(mu + var/2)
    # the 400-node rule against a smaller one is NOT within the bound: the check can fail
    assert np.abs(lr.logistic_normal(MU, VAR, 399) - ref).max() > 1e-4


def test_c_abi_declares_the_likelihood_entry_points():
    """Fails without the feature: the three symbols are new."""
    from gpdemo import _native
    syms = _native.exported_symbols()
    for name in ('apm_set_likelihood', 'apm_likelihood', 'apm_laplace_lik'):
        assert name in syms
    lib = _native.load_library(check_device=False)
    for name in ('apm_set_likelihood', 'apm_likelihood', 'apm_laplace_lik'):
        assert hasattr(lib, name)
    assert lib.apm_version() == 3
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    assert re.search(r'#define\s+APM_LIK_PROBIT\s+0\b', txt)
    assert re.search(r'#define\s+APM_LIK_LOGIT\s+1\b', txt)
    assert (_native.LIK_PROBIT, _native.LIK_LOGIT) == (0, 1)
    m = re.search(r'int\s+apm_laplace_lik\s*\(([^)]*)\)', txt)
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 16 and args[1] == 'int lik'
    # null contexts are refused, not dereferenced
    assert lib.apm_set_likelihood(None, 1) == _native.APM_E_INVALID
    assert lib.apm_likelihood(None) < 0
    # an unknown likelihood is refused before any device work
    one = np.ones(1)
    st = np.zeros(1, dtype=np.int32)
    assert lib.apm_laplace_lik(0, 2, one.ctypes.data, 1, 1, one.ctypes.data, 0, 0, 1e-4, 10,
                               one.ctypes.data, None, 1, None, None,
                               st.ctypes.data) == _native.APM_E_INVALID


def test_unknown_likelihood_is_a_value_error_everywhere():
    """likelihood='cauchit' raises ValueError in each Python entry point, before a device or the
    library is needed."""
    import auxpm.batched as bt
    import gpdemo.estimators as est
    import gpdemo.gradients as gd
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    import gpdemo.predict as prd
    import gpdemo.utils as ut
    from gpdemo import _native
    X, y = np.zeros((4, 2)), np.ones(4)
    kf = krn.make_kernel_func('ard')
    bad = dict(likelihood='cauchit')
    prior = dict(a_sigma=1., b_sigma=1., a_tau=1., b_tau=1.)
    calls = [
        lambda: est.LogMarginalLikelihoodLaplaceEstimator(X, y, kf, **bad),
        lambda: est.LogMarginalLikelihoodPriorMCEstimator(X, y, kf, **bad),
        lambda: est.LogMarginalLikelihoodApproxPosteriorISEstimator(
            X, y, kf, lpa.laplace_approximation, **bad),
        lambda: lpa.laplace_approximation(np.eye(4), y, **bad),
        lambda: prd.LaplacePredictor(X, y, kf, X, **bad),
        lambda: prd.log_predictive_density(np.zeros((1, 4)), np.ones((1, 4)), y, **bad),
        lambda: gd.LaplaceGradient(X, y, kf, **bad),
        lambda: ut.synthetic_gp_data(8, 2, 0, **bad),
        lambda: _native.Context(X, y, _native.KERNEL_ARD, 1e-8, 4, **bad),
        lambda: _native.laplace(np.eye(4), y, False, False, 1e-4, 10, **bad),
        lambda: bt.BatchedAPMEllSSPlusRandDirSliceSampler(X, y, 2, 4, prior, **bad),
        lambda: bt.BatchedAPMEllSSPlusMHSampler(X, y, 2, 4, prior, np.ones(3), **bad),
        lambda: bt.BatchedPMMHSampler(X, y, 2, 4, prior, np.ones(2), **bad),
        lambda: bt.BatchedAPMMetIndPlusRandDirSliceSampler(X, y, 2, 4, prior, **bad),
        lambda: bt.BatchedAPMMetIndPlusMHSampler(X, y, 2, 4, prior, np.ones(3), **bad),
        lambda: bt.BatchedAPMMetIndPlusSeqSliceSampler(X, y, 2, 4, prior, 1.0, **bad),
        lambda: bt.BatchedAPMEllSSPlusEllSSSampler(X, y, 2, 4, 1.0, **bad),
    ]
    for call in calls:
        with pytest.raises(ValueError, match='likelihood'):
            call()
    assert _native.likelihood_code('probit') == 0 and _native.likelihood_code('logit') == 1


def test_host_helpers_of_the_logit():
    """The synthetic-data helper keeps the probit call's X (and labels, by default) and draws
    Bernoulli(sigma(f)) labels for the logit; the log predictive density takes log(prob) /
    log1p(-prob) under the logit and keeps its log_ndtr line under the probit."""
    import gpdemo.predict as prd
    import gpdemo.utils as ut
    from scipy.special import log_ndtr
    Xp, yp = ut.synthetic_gp_data(50, 3, 11)
    Xp2, yp2 = ut.synthetic_gp_data(50, 3, 11, likelihood='probit')
    Xl, yl = ut.synthetic_gp_data(50, 3, 11, likelihood='logit')
    assert np.array_equal(Xp, Xp2) and np.array_equal(yp, yp2) and np.array_equal(Xp, Xl)
    assert set(np.unique(yl)) <= {-1.0, 1.0} and not np.array_equal(yl, yp)
    prob = np.array([[0.9, 0.2, 1e-300], [0.8, 0.4, 1e-300]])
    ys = np.array([1.0, -1.0, 1.0])
    got = prd.log_predictive_density(None, None, ys, likelihood='logit', prob=prob)
    want = np.mean([math.log(0.85), math.log(0.7), math.log(1e-300)])
    assert abs(got - want) <= 1e-12 * abs(want)
    with pytest.raises(ValueError):
        prd.log_predictive_density(None, None, ys, likelihood='logit')
    mean, var = np.array([[0.3, -2.0, 1.0]]), np.array([[1.0, 0.5, 2.0]])
    assert prd.log_predictive_density(mean, var, ys) == \
        float(np.mean(log_ndtr(ys * mean[0] / np.sqrt(1.0 + var[0]))))
