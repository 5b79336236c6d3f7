"""Host side of the joint Laplace / EP predictive: the restatement that the GPU
tests compare the device against (tests/joint_predict_restatement.py) is itself checked against
the marginal predictive's restatement, the oracle's Laplace covariance, a grid quadrature and the
draws' own sample moments; and the Python layer imports and checks its arguments without a device."""
import math

import numpy as np
import pytest
from scipy.special import log_ndtr

import apm_oracle as orc
import cov_restatement as cr
import joint_predict_restatement as jr
from cov_restatement import Cov

EPS = 1e-8
KINDS = [Cov('se', 'iso'), Cov('se', 'ard'), Cov('52', 'ard'),
         Cov('se', 'ard', bias=True, linear=True)]


def _theta(cov, d, s0=0.3):
    nl = d if cov.kind == 'ard' else 1
    return np.r_[s0, np.full(nl, 0.5 * math.log(d) - 0.1), [1.0] * cov.bias, [-1.5] * cov.linear]


def _case(n, d, m, seed):
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) > 0, 1.0, -1.0)
    return X, y, 2.0 * rng.normal(size=(m, d))


@pytest.mark.parametrize('cov', KINDS, ids=repr)
def test_cov_diagonal_is_the_marginal_variance(cov):
    """diag Sigma against var* of the predictive restatements (cov_restatement.predictive and
    ep_predictive), which share the fit: the two differ in the order of one sum."""
    X, y, Xs = _case(40, 3, 17, 1)
    th = _theta(cov, 3)
    kss = cov.prior_var(Xs, th) * np.ones(17)
    lap = jr.at_test_inputs(cov, X, Xs, th, jr.laplace_state(cov, X, y, th, EPS), EPS)
    ref = cr.predictive(cov, X, y, Xs, th, EPS)
    assert np.array_equal(lap['mean'], ref['mean'])
    assert np.all(np.abs(lap['cov'].diagonal() - ref['var']) <= 1e-13 * kss)
    assert np.array_equal(lap['cov'], lap['cov'].T)
    epj = jr.at_test_inputs(cov, X, Xs, th, jr.ep_state(cov, X, y, th, EPS), EPS)
    ref = cr.ep_predictive(cov, X, y, Xs, th, EPS)
    assert np.array_equal(epj['mean'], ref['mean'])
    assert np.all(np.abs(epj['cov'].diagonal() - ref['var']) <= 1e-13 * kss)


@pytest.mark.parametrize('cov', KINDS, ids=repr)
def test_training_inputs_give_the_laplace_covariance(cov):
    """With Xs = X, Sigma is the oracle's Laplace covariance C = K - K W^1/2 B^-1 W^1/2 K up to
    the epsilon that K carries on its diagonal and k*, K** do not: with K = K0 + eps I and
    R = W^1/2 B^-1 W^1/2, C - Sigma = eps (I - R K0 - K0 R) - eps^2 R exactly."""
    X, y, _ = _case(30, 2, 1, 2)
    th = _theta(cov, 2)
    K = cov.gram(X, th, EPS)
    _, C, _, internals = orc.laplace_approximation(K, y, return_internals=True)
    st = dict(L=internals['L'], Ws=np.sqrt(internals['W_diag']), a=internals['a'])
    got = jr.at_test_inputs(cov, X, X, th, st, EPS)['cov']
    n = X.shape[0]
    Binv = np.linalg.inv(internals['L'].dot(internals['L'].T))
    R = st['Ws'][:, None] * Binv * st['Ws'][None, :]
    K0 = K - EPS * np.eye(n)
    diff = EPS * (np.eye(n) - R.dot(K0) - K0.dot(R)) - EPS ** 2 * R
    assert np.abs(C - got).max() <= 3 * EPS * max(1.0, np.abs(R.dot(K0)).max())  # it is O(eps)
    assert np.abs((C - got) - diff).max() <= 1e-12 * np.abs(K).max()


def _grid_density(mean, S, ys, half=9.0, pts=1201):
    """int int Phi(y1 f1) Phi(y2 f2) N(f | mean, S) df by the trapezoid rule on a grid of +-half
    standard deviations in the factor's coordinates (f = mean + L z, z standard normal): the
    integrand is smooth and decays like e^(-z^2/2), so the rule converges geometrically."""
    L = np.linalg.cholesky(S)
    z = np.linspace(-half, half, pts)
    w = np.full(pts, z[1] - z[0])
    w[[0, -1]] *= 0.5
    g = w * np.exp(-0.5 * z ** 2) / math.sqrt(2.0 * math.pi)
    f1 = mean[0] + L[0, 0] * z                                   # (pts,)
    f2 = mean[1] + L[1, 0] * z[:, None] + L[1, 1] * z[None, :]   # (z1, z2)
    inner = np.exp(log_ndtr(ys[1] * f2)).dot(g)
    return float((np.exp(log_ndtr(ys[0] * f1)) * inner).dot(g))


@pytest.fixture(scope='module')
def tiny():
    """n = 1, m = 2, 4096 draws from the oracle's normal stream."""
    cov = Cov('se', 'ard')
    X, y = np.array([[0.4, -0.2]]), np.array([1.0])
    Xs = np.array([[0.1, 0.3], [1.0, -0.9]])
    th = np.array([0.7, 0.1, 0.3])
    ys = np.array([1.0, -1.0])
    xi = orc.u_normal(11, 0, 2, 4096)
    st = jr.laplace_state(cov, X, y, th, EPS, tol=1e-14)
    out = jr.at_test_inputs(cov, X, Xs, th, st, EPS, xi=xi, ys=ys)
    return dict(out, ys=ys)


def test_joint_lpd_vs_grid_quadrature(tiny):
    """exp(lpd) is the mean over the draws of w_r = prod_j p(ys_j | f_rj): within 4 standard
    errors std(w) / sqrt(4096) of the integral."""
    f, ys = tiny['draws'], tiny['ys']
    w = np.exp(log_ndtr(ys[None, :] * f).sum(1))
    exact = _grid_density(tiny['mean'], tiny['cov'] + EPS * np.eye(2), ys)
    coarse = _grid_density(tiny['mean'], tiny['cov'] + EPS * np.eye(2), ys, pts=601)
    assert abs(exact - coarse) <= 1e-12  # the grid has converged
    se = w.std(ddof=1) / math.sqrt(w.shape[0])
    assert abs(math.exp(tiny['lpd']) - w.mean()) <= 1e-14
    assert abs(math.exp(tiny['lpd']) - exact) <= 4.0 * se
    assert se < 0.02 * exact  # (and the bound is no free pass)
    # the two labels are dependent: the product of the marginals lies outside the same bound
    marg = [math.exp(log_ndtr(ys[j] * tiny['mean'][j] / math.sqrt(1.0 + tiny['cov'][j, j])))
            for j in range(2)]
    assert abs(exact - marg[0] * marg[1]) > 4.0 * se


def test_sample_moments_of_the_draws(tiny):
    """Sample mean and covariance of the 4096 draws against mean and Sigma within 4 standard
    errors: sqrt(S_jj / R) for a mean, sqrt((S_ii S_jj + S_ij^2) / R) for a covariance entry."""
    f, S = tiny['draws'], tiny['cov']
    R = f.shape[0]
    assert np.all(np.abs(f.mean(0) - tiny['mean']) <= 4.0 * np.sqrt(S.diagonal() / R))
    se = np.sqrt((np.outer(S.diagonal(), S.diagonal()) + S ** 2) / R)
    assert np.all(np.abs(np.cov(f.T) - S) <= 4.0 * se)
    assert np.all(se <= 0.05 * np.abs(S).max())


def test_long_double_version_agrees_and_is_a_yardstick():
    """The long-double version reproduces the fp64 one to fp64 rounding and its hand-written
    Cholesky refuses a singular matrix."""
    cov = KINDS[3]
    X, y, Xs = _case(40, 3, 17, 3)
    th = _theta(cov, 3)
    ys = np.where(np.arange(17) % 3 == 0, -1.0, 1.0)
    xi = orc.u_normal(5, 2, 17, 64)
    st = jr.laplace_state(cov, X, y, th, EPS)
    a = jr.at_test_inputs(cov, X, Xs, th, st, EPS, xi=xi, ys=ys)
    b = jr.at_test_inputs_ld(cov, X, Xs, th, st, EPS, xi=xi, ys=ys)
    for key, scale in (('mean', 1.0), ('cov', np.abs(a['cov']).max()), ('draws', 10.0),
                       ('lpd', abs(a['lpd']))):
        assert 0.0 <= jr.gap(a, b, key) <= 1e-11 * scale, key
    assert b['draws'].dtype == np.longdouble
    with pytest.raises(np.linalg.LinAlgError):
        jr.cholesky_ld(np.ones((3, 3)))


def test_python_layer_without_a_device():
    import gpdemo.predict as prd
    from gpdemo import _native
    for name in ('joint', 'sample_latent', 'joint_log_predictive_density'):
        assert getattr(prd.EPPredictor, name) is getattr(prd.LaplacePredictor, name)
    assert prd.EPPredictor._joint_approx == _native.JOINT_EP
    assert prd.LaplacePredictor._joint_approx == _native.JOINT_LAPLACE
    assert 'apm_predict_joint' in _native.exported_symbols()
    sd = prd.LaplacePredictor._seeds(7, 3)
    assert sd.dtype == np.uint64 and sd.tolist() == [7, 8, 9]
    assert prd.LaplacePredictor._seeds([4, 4], 2).tolist() == [4, 4]
