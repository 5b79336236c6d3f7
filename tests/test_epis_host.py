"""Host side of the IS estimator with the EP importance distribution (APM_EST_IS_EP, DESIGN.md
§17): the C-ABI / Python surface without a device, and the restatement the device is compared
with (tests/epis_restatement.py) checked on its own - the consistent form against the reference's
direct form, the slot identity a + tau~ mu = nu~, the spread of the estimate against the Laplace
proposal's, and unbiasedness against grid quadrature of a 2 x 2 problem."""
import math
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp, ndtr
from scipy.stats import multivariate_normal

import epis_restatement as eis
import grad_restatement as gr
from cov_restatement import Cov
from conftest import REPO

EPS = 1e-8
N_IMP = 64
CASES = ((65, 4, 'ard', 7081), (130, 5, 'ard', 7141))


def test_surface_names_the_fourth_estimator():
    """Fails without the feature: the macro, the constant, the fused mark and the sampler key are
    new. apm_version() stays 3."""
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    pos = [re.search(r'#define\s+' + name + r'\s+' + str(k) + r'\b', txt)
           for k, name in enumerate(('APM_EST_IS', 'APM_EST_PRIORMC', 'APM_EST_LAPLACE',
                                     'APM_EST_IS_EP'))]
    assert all(pos)
    assert [m.start() for m in pos] == sorted(m.start() for m in pos)
    from gpdemo import _native
    assert _native.EST_IS_EP == 3
    assert (_native.EST_IS, _native.EST_PRIORMC, _native.EST_LAPLACE) == (0, 1, 2)
    assert _native.load_library(check_device=False).apm_version() == 3
    import gpdemo.latent_posterior_approximations as lpa
    assert lpa.ep_approximation.apm_fused is True and lpa.laplace_approximation.apm_fused is True
    from auxpm import batched
    assert batched._EST['is_ep'] == _native.EST_IS_EP
    assert batched._EST['is'] == _native.EST_IS


def test_argument_checks_come_before_any_device_call():
    from gpdemo import _native
    lib = _native.load_library(check_device=False)
    one = np.ones(4)
    st = np.zeros(1, dtype=np.int32)
    for est in (_native.EST_IS_EP, 4):
        assert lib.apm_theta_eval(None, est, 1, one.ctypes.data, 2, None, None, one.ctypes.data,
                                  st.ctypes.data, None) == _native.APM_E_INVALID
        assert lib.apm_theta_eval_K(None, est, one.ctypes.data, 2, 0, 0, one.ctypes.data,
                                    st.ctypes.data, None) == _native.APM_E_INVALID


def test_python_estimator_refuses_the_logit_before_any_device_call():
    import gpdemo.estimators as est
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    X, y = np.zeros((3, 2)), np.ones(3)
    kf = krn.make_kernel_func('ard', 1e-8)
    with pytest.raises(NotImplementedError):
        est.LogMarginalLikelihoodApproxPosteriorISEstimator(X, y, kf, lpa.ep_approximation,
                                                            likelihood='logit')
    with pytest.raises(NotImplementedError):  # (any other function: as before)
        est.LogMarginalLikelihoodApproxPosteriorISEstimator(X, y, kf, lambda K, y: None)


@pytest.fixture(scope='module')
def states():
    """Per case and theta: K (the oracle's Gram), the EP state and the oracle's Laplace state,
    computed once and left unchanged."""
    out = []
    for n, d, kind, seed in CASES:
        c = gr.make_case(n, d, kind, seed)
        c['st'] = []
        for th in c['thetas']:
            K = Cov('se', kind).gram(c['X'], th, EPS)
            c['st'].append((K, eis.state(K, c['y']), eis.laplace_state(K, c['y'])))
        out.append(c)
    return out


def test_consistent_form_equals_the_direct_form(states):
    """1e-9 nats at (65, 4) and (130, 5), the three thetas (the CPU study measured <= 1e-11)."""
    worst = 0.0
    for c in states:
        ns = np.random.RandomState(1).normal(size=(c['n'], N_IMP))
        for th, (K, st, _) in zip(c['thetas'], c['st']):
            a, b = eis.is_consistent(c['y'], st, ns), eis.is_direct(K, c['y'], st, ns)
            print('n {0} theta_0 {1}: consistent {2:.12f} direct {3:.12f} diff {4:.2e}'.format(
                c['n'], th[0], a, b, abs(a - b)))
            worst = max(worst, abs(a - b))
    assert worst <= 1e-9


def test_slot_z_is_the_site_precision_mean(states):
    """|a + tau~ mu - nu~| <= 1e-10 max(1, max|nu~|): the slot writer's z = a + W f_post is nu~."""
    for c in states:
        for _, st, _ in c['st']:
            err = np.abs(st['a'] + st['tau'] * st['mu'] - st['nu']).max()
            print('n {0}: |a + tau mu - nu| = {1:.2e}'.format(c['n'], err))
            assert err <= 1e-10 * max(1.0, np.abs(st['nu']).max())
            assert abs(eis.cst(st) - (0.5 * st['f'].dot(st['a'] + st['W'] * st['f'])
                                      - 0.5 * st['logdet_B'])) <= 1e-10 * max(1, abs(eis.cst(st)))


def test_ep_proposal_has_the_smaller_spread(states):
    """Standard deviation of the log-estimate over 60 draw matrices (RandomState(1), N_imp = 64):
    smaller with the EP state than with the oracle's probit Laplace state, at every theta. A
    condition on the restatements alone; the ratios are in DESIGN.md §17."""
    for c in states:
        rng = np.random.RandomState(1)
        draws = [rng.normal(size=(c['n'], N_IMP)) for _ in range(60)]
        for th, (_, st, lap) in zip(c['thetas'], c['st']):
            v_ep = np.array([eis.is_consistent(c['y'], st, ns) for ns in draws])
            v_la = np.array([eis.is_consistent(c['y'], lap, ns) for ns in draws])
            print('n {0} theta_0 {1}: sd EP {2:.4f} Laplace {3:.4f} ratio {4:.3f}; log-mean-exp '
                  '{5:.4f} / {6:.4f}; sweeps {7}'.format(
                      c['n'], th[0], v_ep.std(), v_la.std(), v_ep.std() / v_la.std(),
                      logsumexp(v_ep) - math.log(60), logsumexp(v_la) - math.log(60),
                      st['n_sweeps']))
            assert v_ep.std() < v_la.std()


def test_two_points_unbiased_against_grid_quadrature():
    """The 2 x 2 problem of test_ep_host: the log of the mean of exp(estimate) over 400 draw
    matrices of N_imp = 64 within four standard errors of the grid-quadrature evidence. Checks the
    formula's unbiasedness, not EP."""
    K = np.array([[2.0, 1.2], [1.2, 1.5]])
    y = np.array([1.0, -1.0])
    g = np.linspace(-12.0, 12.0, 1201)
    F1, F2 = np.meshgrid(g, g, indexing='ij')
    pdf = multivariate_normal(np.zeros(2), K).pdf(np.stack([F1, F2], -1))
    Z = (ndtr(y[0] * F1) * ndtr(y[1] * F2) * pdf).sum() * (g[1] - g[0]) ** 2
    st = eis.state(K, y)
    rng = np.random.RandomState(1)
    w = np.exp([eis.is_consistent(y, st, rng.normal(size=(2, N_IMP))) for _ in range(400)])
    se = w.std(ddof=1) / math.sqrt(w.size) / w.mean()  # (of log mean w, first order)
    print('2x2: log mean {0:.6f} quadrature {1:.6f} se {2:.2e}'.format(
        math.log(w.mean()), math.log(Z), se))
    assert abs(math.log(w.mean()) - math.log(Z)) <= 4.0 * se
