"""The importance-sampling predictive on the host: the route through h_j against
the naive route through K^-1 f_s, the restatement's exactness against grid quadrature of the true
posterior predictive, the far test point and padded samples, and the refusals the Python classes
make before any device call."""
import math

import numpy as np
import pytest
from scipy.special import expit, ndtr

import epis_restatement as er
import is_predict_restatement as ipr
import logit_restatement as lr


def _se(A, B, s, ell):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    return s * np.exp(-0.5 * d2 / ell ** 2)


def _problem(eps, n=40, m=7, S=32, seed=3):
    """n points on [-1, 1] under a unit length scale (K is numerically of low rank: at eps = 1e-8
    its condition is s / eps) and m test points from -1 to 2, the outer ones extrapolating: their
    kriging weights K^-1 k* reach 4e2 at eps = 1e-8."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(-1.0, 1.0, size=(n, 1))
    y = np.where(X[:, 0] + 0.3 * rng.normal(size=n) > 0, 1.0, -1.0)
    Xs = np.linspace(-1.0, 2.0, m)[:, None]
    s = math.exp(0.5)
    K = _se(X, X, s, 1.0) + eps * np.eye(n)
    return K, _se(Xs, X, s, 1.0), s, y, rng.normal(size=(n, S))


def test_h_route_equals_the_naive_route_and_is_stable_where_it_is_not():
    """eps = 1e-2: m_sj = c_j + h_j^T u_s equals k*^T K^-1 f_s to 1e-9 relative. eps = 1e-8, same
    data, with what the device computes in fp32 rounded through float32 (f_s for the naive
    route; the h-route has no computed fp32 input, so its draws u_s are rounded instead): the
    naive route moves by orders of magnitude more. Measured: naive 5.7e-05,
    h-route 5.5e-08 on values up to 3.4, a ratio of 1.0e+03; at eps = 1e-2 the two routes agree to
    2e-14 relative."""
    K, Ks, s, y, U = _problem(1e-2)
    fit = er.laplace_state(K, y)
    hr = ipr.h_route(K, Ks, s, fit['W'], fit['a'], U)
    naive = ipr.naive_route(K, Ks, ipr.samples(hr, fit['f'], U))
    assert np.abs(hr['m'] - naive).max() <= 1e-9 * np.abs(naive).max()

    K, Ks, s, y, U = _problem(1e-8)
    fit = er.laplace_state(K, y)
    hr = ipr.h_route(K, Ks, s, fit['W'], fit['a'], U)
    f_s = ipr.samples(hr, fit['f'], U)
    # the two-line demonstration: K^-1 amplifies the fp32 rounding of f_s by up to s / eps
    d_naive = np.abs(ipr.naive_route(K, Ks, f_s.astype(np.float32).astype(np.float64)) -
                     ipr.naive_route(K, Ks, f_s)).max()
    d_h = np.abs(ipr.h_route(K, Ks, s, fit['W'], fit['a'],
                             U.astype(np.float32).astype(np.float64))['m'] - hr['m']).max()
    print('naive route moves by {0:.3e}, h-route by {1:.3e}, ratio {2:.3e}, max|m| {3:.3e}'
          .format(d_naive, d_h, d_naive / d_h, np.abs(hr['m']).max()))
    assert d_naive > 100.0 * d_h


def _grid_predictive(K, ks, s, y, likelihood):
    """p(y* = 1 | y) of the n = 2 problem by trapezoid quadrature on a grid over (f_1, f_2, f*):
    sum p(y*|f*) N(f*| k*^T K^-1 f, v*) N(f|0, K) prod p(y_i|f_i) / the same without p(y*|f*).
    Independent of the restatement: no proposal, no weights, no factor of M."""
    lik = expit if likelihood == 'logit' else ndtr
    Ki = np.linalg.inv(K)
    sd = np.sqrt(np.diag(K))
    g1 = np.linspace(-9 * sd[0], 9 * sd[0], 361)
    g2 = np.linspace(-9 * sd[1], 9 * sd[1], 361)
    F1, F2 = np.meshgrid(g1, g2, indexing='ij')
    q = Ki[0, 0] * F1 ** 2 + 2 * Ki[0, 1] * F1 * F2 + Ki[1, 1] * F2 ** 2
    post = np.exp(-0.5 * q) * lik(y[0] * F1) * lik(y[1] * F2)      # unnormalised p(f | y)
    w = ks.dot(Ki)
    mstar = w[0] * F1 + w[1] * F2
    vstar = s - w.dot(ks)
    t = np.linspace(-10.0, 10.0, 801)
    pt = np.exp(-0.5 * t ** 2)
    pt /= pt.sum()
    pred = np.zeros_like(mstar)
    for tk, pk in zip(t, pt):                                       # int p(y*|f*) N(f*|m, v*) df*
        pred += pk * lik(mstar + math.sqrt(vstar) * tk)
    return (pred * post).sum() / post.sum()


@pytest.mark.parametrize('proposal,likelihood',
                         [('laplace', 'probit'), ('ep', 'probit'), ('laplace', 'logit')])
def test_restatement_is_exact_against_grid_quadrature(proposal, likelihood):
    """n = 2, one test point: the self-normalised average at S = 200 000 agrees with the grid
    quadrature of the true p(y* = 1 | y) within 5 standard errors of the weighted sample (delta
    method for the self-normalised ratio)."""
    X = np.array([[0.0, 0.0], [1.2, -0.4]])
    y = np.array([1.0, 1.0])
    Xs = np.array([[0.5, 0.3]])
    s = math.exp(1.0)
    K = _se(X, X, s, 1.0) + 1e-8 * np.eye(2)
    Ks = _se(Xs, X, s, 1.0)
    if likelihood == 'logit':
        fit = lr.is_state(K, y)
    elif proposal == 'ep':
        fit = er.state(K, y)
    else:
        fit = er.laplace_state(K, y)
    U = np.random.RandomState(11).normal(size=(2, 200000))
    out = ipr.predictive(K, Ks, s, y, U, fit, likelihood)
    h = ipr.link(out['m'], out['vstar'], likelihood)[0]
    est, se = ipr.prob_stderr(h, out['lw'])
    ref = _grid_predictive(K, Ks[0], s, y, likelihood)
    print('{0}/{1}: IS {2:.6f} +- {3:.1e}, grid {4:.6f}'.format(proposal, likelihood, est, se, ref))
    assert est == pytest.approx(out['prob'][0], abs=1e-12)
    assert 0.0 < se < 1e-3
    assert abs(est - ref) <= 5.0 * se


def test_far_test_point_and_padded_samples():
    K, Ks, s, y, _ = _problem(1e-8)
    Ks = Ks.copy()
    Ks[2] = 0.0  # an uninformed test point
    fit = er.laplace_state(K, y)
    U = np.random.RandomState(5).normal(size=(40, 100))
    out = ipr.predictive(K, Ks, s, y, U, fit)
    assert abs(out['prob'][2] - 0.5) <= 1e-15
    assert out['mean'][2] == 0.0 and abs(out['var'][2] - s) <= 1e-15 * s
    assert 1.0 <= out['ess'] <= 100.0
    Up = np.zeros((40, 128))
    Up[:, :100] = U
    pad = ipr.predictive(K, Ks, s, y, Up, fit, n_real=100)
    assert np.all(pad['wbar'][100:] == 0.0)
    for k in ('prob', 'mean', 'var'):
        np.testing.assert_allclose(pad[k], out[k], rtol=0, atol=1e-13)
    assert pad['ess'] == pytest.approx(out['ess'], rel=1e-13)
    assert pad['logf'] == pytest.approx(out['logf'], abs=1e-12)
    # logf is the estimator's own value
    assert out['logf'] == pytest.approx(er.is_consistent(y, dict(fit, C_chol=_c_chol(K, fit)), U),
                                        abs=1e-9)


def _c_chol(K, fit):
    hr = ipr.h_route(K, np.zeros((1, K.shape[0])), 1.0, fit['W'], fit['a'],
                     np.zeros((K.shape[0], 1)))
    return ipr.samples(hr, np.zeros(K.shape[0]), np.eye(K.shape[0]))


def test_python_classes_refuse_before_any_device_call():
    import gpdemo.kernels as krn
    import gpdemo.predict as prd
    rng = np.random.RandomState(0)
    X, y, Xs = rng.normal(size=(6, 2)), np.array([1., -1., 1., 1., -1., 1.]), rng.normal(size=(3, 2))
    kf = krn.make_kernel_func('ard', 1e-8)
    with pytest.raises(NotImplementedError):
        prd.ISPredictor(X, y, kf, Xs, 8, proposal='ep', likelihood='logit')
    with pytest.raises(ValueError):
        prd.ISPredictor(X, y, kf, Xs, 8, proposal='vb')
    with pytest.raises(ValueError):
        prd.ISPredictor(X, y, kf, Xs, 8, likelihood='cloglog')
    p = prd.ISPredictor(X, y, kf, Xs, 8)  # (no device yet: the context comes with the first call)
    with pytest.raises(ValueError):
        p(np.zeros(3), us=np.zeros((6, 8)), seeds=[1])
    with pytest.raises(ValueError):
        p(np.zeros(3))
    with pytest.raises(ValueError):
        p(np.zeros(3), us=np.zeros((5, 8)))
