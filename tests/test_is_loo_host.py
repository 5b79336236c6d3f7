"""Leave-one-out predictive densities from the importance samples on the host:
the restatement's exactness against grid quadrature of the true log p(y_i | y_-i, theta), how
combine_loo combines a run's rows, the cavity density against EP's own cavity, the properties that
hold pointwise, and the refusals ISLeaveOneOut makes before any device call."""
import math

import numpy as np
import pytest
from scipy.special import expit, log_ndtr, ndtr

import ep_restatement as ep
import epis_restatement as er
import is_loo_restatement as ilr
import logit_restatement as lr
from test_is_predict_host import _se


def _grid_loo(K, y, likelihood):
    """log p(y_i | y_-i) of the n = 2 problem, i = 0, 1, by trapezoid quadrature over (f_1, f_2):
    int p(y_1|f_1) p(y_2|f_2) N(f|0, K) df over the same integral without p(y_i|f_i).
    Independent of the restatement: no proposal, no weights, no factor."""
    lik = expit if likelihood == 'logit' else ndtr
    Ki = np.linalg.inv(K)
    sd = np.sqrt(np.diag(K))
    g1 = np.linspace(-9 * sd[0], 9 * sd[0], 1441)
    g2 = np.linspace(-9 * sd[1], 9 * sd[1], 1441)
    F1, F2 = np.meshgrid(g1, g2, indexing='ij')
    prior = np.exp(-0.5 * (Ki[0, 0] * F1 ** 2 + 2 * Ki[0, 1] * F1 * F2 + Ki[1, 1] * F2 ** 2))
    l1, l2 = lik(y[0] * F1), lik(y[1] * F2)
    joint = (prior * l1 * l2).sum()
    return np.log(np.array([joint / (prior * l2).sum(), joint / (prior * l1).sum()]))


@pytest.mark.parametrize('likelihood', ['probit', 'logit'])
def test_restatement_is_exact_against_grid_quadrature(likelihood):
    """n = 2, S = 200 000, Laplace proposal: loo_i agrees with the grid quadrature of the true
    log p(y_i | y_-i, theta) within 5 standard errors, the standard error 1 / sqrt(ess_loo_i) by
    the delta method (is_loo_restatement.loo_stderr). Measured: probit IS -0.4919 / -0.4980 against
    the grid's -0.5000 (se 3.8e-3 and 3.5e-3: 2.1 and 0.6 of them), where the Laplace cavity value
    is -0.5359; logit IS -0.5569 / -0.5624 against -0.5619 (se 2.9e-3), cavity -0.5740."""
    X = np.array([[0.0, 0.0], [1.2, -0.4]])
    y = np.array([1.0, 1.0])
    K = _se(X, X, math.exp(1.0), 1.0) + 1e-8 * np.eye(2)
    fit = lr.is_state(K, y) if likelihood == 'logit' else er.laplace_state(K, y)
    U = np.random.RandomState(11).normal(size=(2, 200000))
    out = ilr.loo_quantities(y, *ilr.slot_of(fit), U, likelihood)
    ref = _grid_loo(K, y, likelihood)
    se = ilr.loo_stderr(out['ess_loo'])
    for i in range(2):
        print('{0} point {1}: IS {2:.5f} +- {3:.1e} (ratio form {4:.1e}), grid {5:.5f}, cavity '
              '{6:.5f}, ess_loo {7:.3g}'.format(likelihood, i, out['loo'][i], se[i],
                                                ilr.loo_stderr_ratio(out['lw'], out['lp'][i]),
                                                ref[i], out['gauss'][i], out['ess_loo'][i]))
    assert np.all((se > 0.0) & (se < 1e-2))
    assert np.all(np.abs(out['loo'] - ref) <= 5.0 * se)


def test_combine_loo_of_equal_pieces_is_the_whole():
    """One long weighted sample cut into T equal-weight pieces: each piece's rows are formed with
    the piece's share of the whole's weights, so the arithmetic mean of 1 / p over the pieces is
    the whole's. burn and thin select rows as predict._keep does."""
    from gpdemo.loo import combine_loo
    from scipy.special import logsumexp
    rng = np.random.RandomState(4)
    n, S, T = 7, 240, 6
    lp = -np.abs(rng.normal(size=(n, S))) * 3.0             # log p_si
    lw = rng.normal(size=(T, S // T)) * 2.0
    lw_piece = lw - logsumexp(lw, axis=1)[:, None]          # each piece's own normalised weights
    lwbar = (lw_piece - np.log(T)).reshape(S)               # the whole's: every piece weighs 1/T
    whole_loo = -logsumexp(lwbar[None] - lp, axis=1)
    whole_lpd = logsumexp(lwbar[None] + lp, axis=1)
    pieces = lp.reshape(n, T, S // T)
    lo = np.stack([-logsumexp(lw_piece[t][None] - pieces[:, t], axis=1) for t in range(T)])
    ld = np.stack([logsumexp(lw_piece[t][None] + pieces[:, t], axis=1) for t in range(T)])
    out = combine_loo(lo, ld)
    np.testing.assert_allclose(out['loo'], whole_loo, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out['lpd'], whole_lpd, rtol=0, atol=1e-12)
    assert out['elpd_loo'] == pytest.approx(whole_loo.sum(), abs=1e-12)
    assert out['p_loo'] == pytest.approx(whole_lpd.sum() - whole_loo.sum(), abs=1e-12)
    assert out['se'] == pytest.approx(math.sqrt(n * np.var(whole_loo)), abs=1e-12)
    assert out['p_loo'] >= 0.0
    kept = combine_loo(lo, ld, burn=1, thin=2)
    np.testing.assert_array_equal(kept['loo'], combine_loo(lo[1::2], ld[1::2])['loo'])
    np.testing.assert_array_equal(kept['lpd'], combine_loo(lo[1::2], ld[1::2])['lpd'])
    with pytest.raises(ValueError):
        combine_loo(lo, ld, burn=T)
    with pytest.raises(ValueError):
        combine_loo(lo, ld[:, :3])
    with pytest.raises(ValueError):
        combine_loo(lo[0], ld[0])


def _problem(n=130, d=5, seed=100):
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * X[:, 1] + 0.5 * rng.normal(size=n) > 0, 1.0, -1.0)
    return _se(X, X, math.exp(0.3), 2.0) + 1e-8 * np.eye(n), y


def test_cavity_is_eps_own_on_a_converged_ep_fit():
    """On ep_restatement's converged fit the slot quantities are C_ii = the posterior variance,
    W = tau~ and z = C^-1 mu; gauss_i is then that fit's cavity normaliser
    log Phi(y_i mu_-i / sqrt(1 + sigma^2_-i)) to 1e-10."""
    K, y = _problem(60, 3, 7)
    st = er.state(K, y, diff_tol=1e-16, max_sweeps=400)
    f, W, z, C_chol, _ = ilr.slot_of(st)
    got = ilr.cavity(y, f, W, z, (C_chol * C_chol).sum(1))
    tau_c = 1.0 / st['var'] - st['tau']
    mu_c, var_c = (st['mu'] / st['var'] - st['nu']) / tau_c, 1.0 / tau_c
    own = log_ndtr(ep.tilted(y, mu_c, var_c)[0])
    print('cavity vs EP: max |d| {0:.2e}, min tau {1:.3g}'.format(np.abs(got['gauss'] - own).max(),
                                                                  got['tau'].min()))
    np.testing.assert_allclose(got['gauss'], own, rtol=0, atol=1e-10)


@pytest.mark.parametrize('proposal,likelihood',
                         [('laplace', 'probit'), ('ep', 'probit'), ('laplace', 'logit')])
def test_pointwise_properties(proposal, likelihood):
    """(n, d) = (130, 5), S = 64, with and without padded columns: lpd_i >= loo_i (Jensen: the
    harmonic mean of p is at most its arithmetic mean) and 1 <= ess_loo_i <= S at every point,
    none left out; padding adds nothing."""
    K, y = _problem()
    if likelihood == 'logit':
        fit = lr.is_state(K, y)
    else:
        fit = er.state(K, y) if proposal == 'ep' else er.laplace_state(K, y)
    U = np.random.RandomState(9).normal(size=(130, 64))
    out = ilr.loo_quantities(y, *ilr.slot_of(fit), U, likelihood)
    print('{0}/{1}: sum loo {2:.2f} sum gauss {3:.2f} sum lpd {4:.2f} min ess_loo {5:.2f}'.format(
        proposal, likelihood, out['loo'].sum(), out['gauss'].sum(), out['lpd'].sum(),
        out['ess_loo'].min()))
    assert np.all(out['lpd'] >= out['loo'])
    assert np.all((out['ess_loo'] >= 1.0) & (out['ess_loo'] <= 64.0 * (1 + 1e-12)))
    assert 1.0 <= out['ess'] <= 64.0
    assert np.isfinite(out['gauss']).all() and np.all(out['gauss'] < 0.0)
    Up = np.zeros((130, 128))
    Up[:, :64] = U
    pad = ilr.loo_quantities(y, *ilr.slot_of(fit), Up, likelihood, n_real=64)
    for k in ('loo', 'lpd', 'ess_loo', 'gauss'):
        np.testing.assert_allclose(pad[k], out[k], rtol=1e-13, atol=1e-13)
    assert pad['logf'] == pytest.approx(out['logf'], abs=1e-12)
    # one sample: wbar = 1, so loo = lpd = log p(y_i | f_1i) and ess_loo = 1
    one = ilr.loo_quantities(y, *ilr.slot_of(fit), U[:, :1], likelihood)
    np.testing.assert_array_equal(one['loo'], one['lpd'])
    np.testing.assert_array_equal(one['loo'], one['lp'][:, 0])
    np.testing.assert_array_equal(one['ess_loo'], np.ones(130))


def test_python_class_refuses_before_any_device_call():
    import gpdemo.kernels as krn
    from gpdemo.loo import ISLeaveOneOut
    rng = np.random.RandomState(0)
    X, y = rng.normal(size=(6, 2)), np.array([1., -1., 1., 1., -1., 1.])
    kf = krn.make_kernel_func('ard', 1e-8)
    with pytest.raises(NotImplementedError):
        ISLeaveOneOut(X, y, kf, 8, proposal='ep', likelihood='logit')
    with pytest.raises(ValueError):
        ISLeaveOneOut(X, y, kf, 8, proposal='vb')
    with pytest.raises(ValueError):
        ISLeaveOneOut(X, y, kf, 8, likelihood='cloglog')
    with pytest.raises(ValueError):
        ISLeaveOneOut(X, y, kf, 0)
    with pytest.raises(ValueError):
        ISLeaveOneOut(X, y[:5], kf, 8)
    with pytest.raises(NotImplementedError):
        ISLeaveOneOut(X, y, lambda K, X, theta: None, 8)
    p = ISLeaveOneOut(X, y, kf, 8)  # (no device yet: the context comes with the first call)
    with pytest.raises(ValueError):
        p(np.zeros(3), us=np.zeros((6, 8)), seeds=[1])
    with pytest.raises(ValueError):
        p(np.zeros(3))
    with pytest.raises(ValueError):
        p(np.zeros(3), us=np.zeros((5, 8)))
    with pytest.raises(ValueError):
        p(np.zeros((2, 3)), seeds=[1])
    with pytest.raises(ValueError):
        p(np.zeros(3), seeds=[1], on_error='ignore')
    assert p._ctx is None
