"""The linear (dot-product) covariance term on the device (APM_COV_LINEAR): Gram and
cross-Gram, the four estimators' theta-calls, the three predictives with their per-row prior
variance, the leave-one-out densities, the Laplace and EP gradients, lambda = 0 against the kind
without the flag, batch neutrality, two other contexts beside a linear one, the range flags at a
large lambda and the Python layer - against tests/cov_restatement.py and the oracle's
estimators run with its kernel_func. The maxima measured on an MI355X are in DESIGN.md §25's
parity table."""
import math

import numpy as np
import pytest

import apm_oracle as orc
import cov_checks as cc
import cov_restatement as cr
import ep_restatement as ep
import epis_restatement as eis
import grad_restatement as gr
import is_loo_restatement as ilr
import is_predict_restatement as ipr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = 1e-8
TOL_NATS = 5e-4     # estimator values, no relative term
TOL = 1e-9          # fp64 against fp64 through the same factorisation (x max(1, max|ref|))
NEWTON_TOL = 1e-14  # the gradient's Newton tolerance
PROB_TOL = 1e-3     # the IS predictive's averages
FLOOR, CAP = 1e-12, 1e-6  # §19's yardstick rule for its fp64 quantities
W_TOL = 1e-3        # test_gpu_is_loo's bound on loo, lpd and log ess_loo (plus 10 Y)
G_FLOOR, G_REL = 1e-9, 2.4e-7  # and on gauss
# the thetas are (theta_0, log lambda) = (0.3, -2), (0.3, 1), (3, 1), (-1, -2), with
# log beta = 1.5 where biased.
PAIRS = ((0.3, -2.0), (0.3, 1.0), (3.0, 1.0), (-1.0, -2.0))
FAR = 50.0  # the far test row: the SE part of k* underflows to exactly 0
# (purpose, n, d, kind, bias) -> data seed, the first one from 1300 on whose labels are 30-70 %
# positive and for which, at all four thetas, the restatement cannot disagree with the device on
# an iteration or sweep count (DESIGN.md §16's margins, asserted again before each comparison):
#   'grad'    the last Newton diff <= 1e-16 and the one before >= 1e-12 at the gradient's 1e-14
#             (n = 1: >= 1.5e-14)
#   'epgrad'  the EP fit's last stop measure < 0.99 diff_tol, the one before > 1.01 diff_tol
#   'call'    a factor 3 on both sides of the Newton loop's 1e-4, and the EP margin
SEEDS = {
    ('grad', 1, 1, 'ard', False): 1300, ('grad', 1, 1, 'ard', True): 1303,
    ('grad', 64, 33, 'ard', False): 1303, ('grad', 64, 33, 'ard', True): 1302,
    ('grad', 130, 5, 'ard', False): 1304, ('grad', 130, 5, 'ard', True): 1304,
    ('grad', 200, 3, 'iso', False): 1309, ('grad', 200, 3, 'iso', True): 1309,
    ('grad', 600, 4, 'ard', False): 1300, ('grad', 600, 4, 'ard', True): 1300,
    ('epgrad', 1, 1, 'ard', False): 1300, ('epgrad', 1, 1, 'ard', True): 1300,
    ('epgrad', 64, 33, 'ard', False): 1300, ('epgrad', 64, 33, 'ard', True): 1300,
    ('epgrad', 130, 5, 'ard', False): 1300, ('epgrad', 130, 5, 'ard', True): 1300,
    ('epgrad', 200, 3, 'iso', False): 1300, ('epgrad', 200, 3, 'iso', True): 1300,
    ('epgrad', 600, 4, 'ard', False): 1300, ('epgrad', 600, 4, 'ard', True): 1300,
    ('call', 130, 5, 'ard', False): 1300, ('call', 130, 5, 'ard', True): 1300,
    ('call', 200, 3, 'iso', True): 1306, ('call', 65, 4, 'ard', True): 1303,
    ('call', 513, 4, 'ard', True): 1301, ('call', 577, 4, 'ard', True): 1302,
}
_CASES = {}


def _case(what, n, d, kind, bias):
    """Data of one (purpose, shape, kind), drawn once and left unchanged."""
    key = (what, n, d, kind, bias)
    if key not in _CASES:
        _CASES[key] = _make_case(n, d, kind, bias, SEEDS[key])
    return _CASES[key]


def _make_case(n, d, kind, bias, seed):
    rows = [(s0, 1.5, ll) if bias else (s0, ll) for s0, ll in PAIRS]
    return dict(gr.make_case(n, d, kind, seed, rows=rows), bias=bias)


def _cov(kind, bias, linear=True):
    return Cov('se', kind, bias=bias, linear=linear)


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _ctx(nat, c, n_imp=1, max_batch=4, n_slots=4, n_ubufs=4, linear=True, kind=None):
    nk = _cov(c['kind'], c['bias'], linear).native_kind if kind is None else kind
    return nat.Context(c['X'], c['y'], nk, EPS, n_imp, max_batch=max_batch, n_slots=n_slots,
                       n_ubufs=n_ubufs)


# ------------------------------------------------------------------ 1. Gram and cross-Gram


GRAM_CASES = ([(k, b, n, d) for k, b in cr.LINEAR_KINDS for n, d in ((1, 1), (129, 64))] +
              [('ard', True, 300, 7)])


@pytest.mark.parametrize('kind,bias,n,d', GRAM_CASES)
def test_gram_vs_restatement(nat, kind, bias, n, d):
    """Entry by entry within Cov.gram_bound (the base kind's bound on S plus 3u |K_ref| plus the
    fma chain's (d + 2) u lambda sum_k |x_ik x_jk|) at the four (theta_0, log lambda); K exactly
    symmetric, every entry of the caller's (n, n) array written. (129, 64) takes two LDS chunks
    of features in both sweeps. Measured on an MI355X: at most 0.74 of the bound."""
    import gpdemo.kernels as krn
    c = _make_case(n, d, kind, bias, 5 + n)
    X = c['X']
    for th in c['thetas']:
        K = np.full((n, n), np.nan)
        krn.make_kernel_func(kind, EPS, bias=bias, linear=True)(K, X, th)
        Kref = _cov(kind, bias).gram(X, th, EPS)
        err, bound = np.abs(K - Kref), _cov(kind, bias).gram_bound(X, X, th, Kref)
        print('linear gram {0}: max error / bound = {1:.3f}'.format(
            (kind, bias, n, d, th[0], th[-1]), float((err / bound).max())))
        assert np.all(err <= bound)
        assert np.array_equal(K, K.T)
        with pytest.raises(IndexError):
            nat.gram(_cov(kind, bias).native_kind, K, X, th[:-1], EPS)


@pytest.mark.parametrize('kind,bias', cr.LINEAR_KINDS)
@pytest.mark.parametrize('m,n,d', [(70, 130, 5), (1, 129, 40)])
def test_gram_cross_vs_restatement(nat, kind, bias, m, n, d):
    """The same bound for k(Xs_i, X_j); no epsilon where a test point coincides with a training
    point. Measured on an MI355X: at most 0.90 of the bound."""
    c = _make_case(n, d, kind, bias, m + n)
    X = c['X']
    Xs = np.random.RandomState(m + n + 1).normal(size=(m, d))
    Xs[0] = X[7]
    for th in c['thetas']:
        Ks = nat.gram_cross(_cov(kind, bias).native_kind, Xs, X, th)
        assert Ks.shape == (m, n)
        ref = _cov(kind, bias).gram_cross(Xs, X, th)
        err, bound = np.abs(Ks - ref), _cov(kind, bias).gram_bound(Xs, X, th, ref)
        print('linear cross-gram {0}: max error / bound = {1:.3f}'.format(
            (kind, bias, m, n, d, th[0], th[-1]), float((err / bound).max())))
        assert np.all(err <= bound)
        kss = _cov(kind, bias).prior_var(Xs[:1], th)[0]
        assert abs(Ks[0, 7] - kss) <= bound[0, 7]


# ------------------------------------------------------------------ 2. theta-calls


CALL_CASES = [(130, 5, 'ard', False), (200, 3, 'iso', True), (65, 4, 'ard', True),
              (513, 4, 'ard', True), (577, 4, 'ard', True)]


@pytest.mark.parametrize('n,d,kind,bias', CALL_CASES)
def test_estimators_vs_oracle(nat, n, d, kind, bias):
    """IS (theta-call and one cached u-call), PriorMC, Laplace and IS_EP estimates (N_imp = 8)
    against the oracle's estimators with the restatement's kernel_func, at (theta_0, log lambda)
    = (0.3, 1) and (-1, -2): 5e-4 nats (Laplace: 1e-9 max(1, |ref|)), status 0, the oracle's
    n_cubic_ops. First, on the CPU: the stop margins, and the oracle's own IS value moves by less
    than 5e-5 nats under 1-ulp noise in K."""
    c = _case('call', n, d, kind, bias)
    X, y = c['X'], c['y']
    kf = _cov(kind, bias).kernel_func(EPS)
    rng = np.random.RandomState(17)
    ns1, ns2 = rng.normal(size=(n, 8)), rng.normal(size=(n, 8))
    ctx = _ctx(nat, c, n_imp=8, max_batch=1, n_slots=2, n_ubufs=2)
    try:
        ctx.u_upload(0, ns1)
        ctx.u_upload(1, ns2)
        for th in c['thetas'][[1, 3]]:
            K = _cov(kind, bias).gram(X, th, EPS)
            cc.newton_margins(K, y, 1e-4, NEWTON_TOL)
            moves = cc.oracle_moves(X, y, ns1, K)
            assert moves < 5e-5, moves
            r1, rc, rops = orc.is_estimate(X, y, kf, ns1, th)
            r2, _, _ = orc.is_estimate(X, y, kf, ns2, None, rc)
            p1, _, pops = orc.priormc_estimate(X, y, kf, ns1, th)
            lml, lops = orc.laplace_estimate(X, y, kf, th)
            est = eis.state(K, y)
            cc.ep_margins(est)
            e1 = eis.is_consistent(y, est, ns1)
            out, st, nops = ctx.theta_eval(nat.EST_IS, th[None], [0], [0])
            out2, st2 = ctx.u_eval([0], [1])
            pm, pst, pnops = ctx.theta_eval(nat.EST_PRIORMC, th[None], [0], [1])
            lp, lst, lnops = ctx.theta_eval(nat.EST_LAPLACE, th[None])
            epv, est_st, enops = ctx.theta_eval(nat.EST_IS_EP, th[None], [0], [1])
            print('linear {0} theta {1}: IS {2:.2e} u-call {3:.2e} PriorMC {4:.2e} Laplace '
                  '{5:.2e} IS_EP {6:.2e} nats (oracle moves {7:.1e})'.format(
                      (n, d, kind, bias), (th[0], th[-1]), abs(out[0] - r1), abs(out2[0] - r2),
                      abs(pm[0] - p1), abs(lp[0] - lml), abs(epv[0] - e1), moves))
            assert st[0] == 0 and st2[0] == 0 and pst[0] == 0 and lst[0] == 0 and est_st[0] == 0
            assert nops[0] == rops and pnops[0] == pops and lnops[0] == lops
            assert int(enops[0]) == 2 * est['n_sweeps'] + 3
            assert abs(out[0] - r1) <= TOL_NATS
            assert abs(out2[0] - r2) <= TOL_NATS
            assert abs(pm[0] - p1) <= TOL_NATS
            assert abs(lp[0] - lml) <= TOL * max(1.0, abs(lml))
            assert abs(epv[0] - e1) <= TOL_NATS
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. prediction and LOO


PREDICT_CASES = [(130, 5, 'ard', True), (577, 4, 'ard', True)]


def _far_mean(c, th, Xs, a):
    """beta sum(a) + lambda x* . X^T a at the far test row (S* = 0 exactly there)."""
    cov = _cov(c['kind'], c['bias'])
    _, beta, lam = cov.split(th, c['d'])
    assert np.all(cov.base_cross(Xs[-1:], c['X'], th[:c['d'] + 1]) == 0.0)
    return beta * a.sum() + lam * Xs[-1].dot(c['X'].T.dot(a))


@pytest.mark.parametrize('n,d,kind,bias', PREDICT_CASES)
def test_laplace_and_ep_predict_vs_restatement(nat, n, d, kind, bias):
    """apm_predict and apm_ep_predict at m = 70: mean and var relative to max(1, max|ref|), prob
    absolute, at 1e-9, equal iteration / sweep counts (the margins first, on the CPU). At the far
    test row the mean is beta sum(a) + lambda x* . X^T a and the variance starts from
    k** = s + beta + lambda |x*|^2, both at the 1e-9 yardstick."""
    c = _case('call', n, d, kind, bias)
    Xs = cc.far_test_inputs(c, 70, FAR)
    ctx = _ctx(nat, c)
    try:
        lp = ctx.predict(c['thetas'], Xs)
        epd = ctx.ep_predict(c['thetas'], Xs)
    finally:
        ctx.close()
    assert not lp[3].any() and not epd[3].any()
    for t, th in enumerate(c['thetas']):
        K = _cov(kind, bias).gram(c['X'], th, EPS)
        cc.newton_margins(K, c['y'], 1e-4, NEWTON_TOL)
        ref = cr.predictive(_cov(kind, bias), c['X'], c['y'], Xs, th, EPS)
        eref = cr.ep_predictive(_cov(kind, bias), c['X'], c['y'], Xs, th, EPS)
        cc.ep_margins(ep.ep_fit(K, c['y']))
        w_l, w_e = cc.worst([x[t] for x in lp[:3]], ref), cc.worst([x[t] for x in epd[:3]], eref)
        far = _far_mean(c, th, Xs, ref['a'])
        kss = _cov(kind, bias).prior_var(Xs, th)
        mscale, vscale = max(1.0, np.abs(ref['mean']).max()), max(1.0, np.abs(ref['var']).max())
        d_far = abs(lp[0][t, -1] - far) / mscale
        print('linear predict {0} theta {1}: Laplace {2:.2e} EP {3:.2e} far mean {4:.2e} (tol '
              '{5:.0e}), k** at the far row {6:.1f} against {7:.1f} at the coinciding one'.format(
                  (n, d, kind, bias), (th[0], th[-1]), w_l, w_e, d_far, TOL, kss[-1], kss[0]))
        assert int(lp[4][t]) == ref['n_iter'] and int(epd[4][t]) == eref['n_sweeps']
        assert w_l <= TOL and w_e <= TOL
        assert d_far <= TOL and far != 0.0
        assert kss[-1] > 100.0 * kss[0]  # (a constant k** = k**_0 would be off by that much)
        assert abs(lp[1][t, -1] - ref['var'][-1]) <= TOL * vscale
        assert np.all(lp[1][t] > 0.0) and np.all(lp[1][t] <= kss * (1 + 1e-15))


@pytest.mark.parametrize('n,d,kind,bias', PREDICT_CASES)
@pytest.mark.parametrize('proposal', ['laplace', 'ep'])
def test_is_predict_vs_restatement(nat, n, d, kind, bias, proposal, monkeypatch):
    """apm_is_predict with both proposals at (theta_0, log lambda) = (0.3, 1), m = 70, S = 64.
    DESIGN.md §19's yardstick rule for the fp64 quantities c_j and v*_j (read off a one-sample
    context with a zero U column, fp64 Newton): 10x the restatement's own float64-to-longdouble
    discrepancy, floored at 1e-12, the discrepancy capped at 1e-6; prob, mean, var and ess of the
    default path at 1e-3. v*_j starts from the per-row k**."""
    c = _case('call', n, d, kind, bias)
    Xs = cc.far_test_inputs(c, 70, FAR)
    th = c['thetas'][1]
    K = _cov(kind, bias).gram(c['X'], th, EPS)
    Ks = _cov(kind, bias).gram_cross(Xs, c['X'], th)
    kss = _cov(kind, bias).prior_var(Xs, th)
    cc.newton_margins(K, c['y'], 1e-4, NEWTON_TOL)
    U = np.random.RandomState(107).normal(size=(n, 64)).astype(np.float32).astype(np.float64)
    fit = eis.state(K, c['y']) if proposal == 'ep' else eis.laplace_state(K, c['y'])
    if proposal == 'ep':
        cc.ep_margins(fit)
    ref = ipr.predictive(K, Ks, kss, c['y'], U, fit, 'probit')
    hi = ipr.h_route(K, Ks, kss, fit['W'], fit['a'], U[:, :1], dtype=np.longdouble)
    est = nat.EST_IS_EP if proposal == 'ep' else nat.EST_IS
    ctx = _ctx(nat, c, n_imp=64, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        ctx.u_upload(0, U)
        logf0, st0, _ = ctx.theta_eval(est, th[None], [0], [0])
        logf, prob, mean, var, ess, st, _ = ctx.is_predict(est, th[None], [0], [0], Xs)
    finally:
        ctx.close()
    monkeypatch.setenv('APM_MIXED', '0')
    one = _ctx(nat, c, n_imp=1, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        one.u_upload(0, np.zeros((n, 1)))
        _, _, cdev, vdev, ess1, st1, _ = one.is_predict(est, th[None], [0], [0], Xs)
    finally:
        one.close()
    assert st0[0] == 0 and st[0] == 0 and st1[0] == 0 and ess1[0] == 1.0
    assert logf[0] == logf0[0]
    for key, dev in (('c', cdev[0]), ('vstar', vdev[0])):
        scale = max(1.0, float(np.abs(ref[key]).max()))
        yard = float(np.abs(ref[key] - hi[key]).max()) / scale
        err = float(np.abs(dev - ref[key]).max()) / scale
        print('linear is_predict {0} {1} {2}: device {3:.2e} yardstick {4:.2e}'.format(
            (n, d, kind, bias), proposal, key, err, yard))
        assert yard < CAP
        assert err <= max(10.0 * yard, FLOOR)
    mscale = max(1.0, float(np.abs(ref['m']).max()))
    d_prob = float(np.abs(prob[0] - ref['prob']).max())
    d_mean = float(np.abs(mean[0] - ref['mean']).max()) / mscale
    d_var = float(np.abs(var[0] - ref['var']).max()) / max(1.0, mscale ** 2)
    d_ess = abs(ess[0] - ref['ess']) / ref['ess']
    print('linear is_predict {0} {1}: d prob {2:.2e} d mean {3:.2e} d var {4:.2e} d ess {5:.2e}'
          .format((n, d, kind, bias), proposal, d_prob, d_mean, d_var, d_ess))
    assert d_prob <= PROB_TOL and d_mean <= PROB_TOL and d_var <= PROB_TOL and d_ess <= PROB_TOL
    assert abs(cdev[0, -1] - _far_mean(c, th, Xs, fit['a'])) <= TOL * max(1.0, np.abs(ref['c']).max())


@pytest.mark.parametrize('proposal', ['laplace', 'ep'])
def test_is_loo_vs_restatement(nat, proposal):
    """apm_is_loo at (130, 5), SE-ARD + bias + linear, (theta_0, log lambda) = (0.3, 1), S = 64,
    against is_loo_restatement on this kind's K with test_gpu_is_loo's bounds: loo, lpd and
    log ess_loo within 1e-3 + 10 Y (Y the restatement's fp32 yardstick), gauss within its bound."""
    c = _case('call', 130, 5, 'ard', True)
    y, th = c['y'], c['thetas'][1]
    K = _cov('ard', True).gram(c['X'], th, EPS)
    cc.newton_margins(K, y, 1e-4, NEWTON_TOL)
    U = np.random.RandomState(107).normal(size=(130, 64)).astype(np.float32).astype(np.float64)
    fit = eis.state(K, y) if proposal == 'ep' else eis.laplace_state(K, y)
    if proposal == 'ep':
        cc.ep_margins(fit)
    slot = ilr.slot_of(fit)
    ref = ilr.loo_quantities(y, *slot, U, 'probit')

    def r32(a):
        return a.astype(np.float32).astype(np.float64)
    q32 = ilr.loo_quantities(y, slot[0], slot[1], slot[2], r32(slot[3]), slot[4], r32(U), 'probit')
    Y = max(float(np.abs(q32[k] - ref[k]).max()) for k in ('loo', 'lpd'))
    Y = max(Y, float(np.abs(np.log(q32['ess_loo'] / ref['ess_loo'])).max()))
    f, W, z, C_chol, _ = slot
    cd = (C_chol * C_chol).sum(1)
    g0 = ilr.cavity(y, f, W, z, cd, 'probit')['gauss']
    g1 = ilr.cavity(y, f, W, z, cd * (1.0 + G_REL), 'probit')['gauss']
    gbound = G_FLOOR + 10.0 * np.abs(g1 - g0)
    ctx = _ctx(nat, c, n_imp=64, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        ctx.u_upload(0, U)
        est = nat.EST_IS_EP if proposal == 'ep' else nat.EST_IS
        logf0, st0, _ = ctx.theta_eval(est, th[None], [0], [0])
        logf, loo, lpd, ess_loo, gauss, ess, st = ctx.is_loo([0], [0])
    finally:
        ctx.close()
    assert st0[0] == 0 and st[0] == 0
    bound = W_TOL + 10.0 * Y
    d_loo = float(np.abs(loo[0] - ref['loo']).max())
    d_lpd = float(np.abs(lpd[0] - ref['lpd']).max())
    d_ess = float(np.abs(np.log(ess_loo[0] / ref['ess_loo'])).max())
    d_g = np.abs(gauss[0] - ref['gauss'])
    print('linear is_loo {0}: d loo {1:.2e} d lpd {2:.2e} d log ess_loo {3:.2e} (Y {4:.1e}) '
          'gauss at most {5:.2f} of its bound'.format(proposal, d_loo, d_lpd, d_ess, Y,
                                                      float((d_g / gbound).max())))
    assert d_loo <= bound and d_lpd <= bound and d_ess <= bound
    assert np.all(d_g <= gbound)
    assert abs(logf[0] - ref['logf']) <= W_TOL and logf[0] == logf0[0]


# ------------------------------------------------------------------ 4. gradients


GRAD_CASES = [(n, d, k, b) for n, d, k in ((1, 1, 'ard'), (64, 33, 'ard'), (130, 5, 'ard'),
                                           (200, 3, 'iso'), (600, 4, 'ard'))
              for b in (False, True)]


@pytest.mark.parametrize('n,d,kind,bias', GRAD_CASES)
def test_laplace_grad_vs_restatement_and_central_differences(nat, n, d, kind, bias):
    """lml and all P gradient entries against the restatement at 1e-9 of max(1, max|ref grad|)
    with equal Newton iteration counts (the margins asserted first, on the CPU); at (130, 5)
    against central differences (h = 1e-5) of the device's own Laplace theta-call, Newton
    tolerance 1e-14, at 1e-6; lml bitwise the Laplace theta-call's at the same settings."""
    c = _case('grad', n, d, kind, bias)
    refs = [cr.laplace_grad(_cov(kind, bias), c['X'], c['y'], th, EPS, tol=NEWTON_TOL)
            for th in c['thetas']]
    for ref in refs:
        assert ref['diffs'][-1] <= NEWTON_TOL / 100.0
        assert ref['diffs'][-2] >= (1.5 if n == 1 else 100.0) * NEWTON_TOL
    worst_fd = 0.0
    ctx = _ctx(nat, c)
    try:
        ctx.set_newton(NEWTON_TOL, 1000)
        lml, grad, st, nit = ctx.laplace_grad(c['thetas'])
        val, vst, nops = ctx.theta_eval(nat.EST_LAPLACE, c['thetas'])
        if n == 130:
            th = c['thetas'][1]
            fd = gr.central_differences(
                lambda x: ctx.theta_eval(nat.EST_LAPLACE, x[None])[0][0], th)
            worst_fd = np.abs(grad[1] - fd).max() / max(1.0, np.abs(fd).max())
    finally:
        ctx.close()
    assert not st.any() and not vst.any() and grad.shape == (4, c['thetas'].shape[1])
    assert np.array_equal(val, lml) and np.array_equal(nops, nit)
    worst = 0.0
    for t, (th, ref) in enumerate(zip(c['thetas'], refs)):
        assert int(nit[t]) == ref['n_iter']
        scale = max(1.0, np.abs(ref['grad']).max())
        err = max(abs(lml[t] - ref['lml']), np.abs(grad[t] - ref['grad']).max()) / scale
        worst = max(worst, err)
        assert grad[t, -1] != 0.0
    print('linear grad parity {0}: worst {1:.3e} (tol {2:.0e}), vs the device\'s own central '
          'differences {3:.3e} (tol 1e-06)'.format((n, d, kind, bias), worst, TOL, worst_fd))
    assert worst <= TOL
    assert worst_fd <= 1e-6


@pytest.mark.parametrize('n,d,kind,bias', GRAD_CASES)
def test_ep_grad_vs_restatement_and_central_differences(nat, n, d, kind, bias):
    """log Z_EP and all P entries of its gradient against the restatement at 1e-9 of max(1,
    max|ref grad|), equal sweep counts (the stop margins asserted first, on the CPU), logz bitwise
    Context.ep's; at (130, 5) against central differences (h = 1e-5) of the device's own log Z_EP
    fitted to diff_tol = 1e-16 at 1e-6."""
    c = _case('epgrad', n, d, kind, bias)
    refs = [cr.ep_grad(_cov(kind, bias), c['X'], c['y'], th, EPS) for th in c['thetas']]
    for ref in refs:
        cc.ep_margins(ref['fit'])
    worst_fd = 0.0
    ctx = _ctx(nat, c)
    try:
        logz, grad, st, nsw = ctx.ep_grad(c['thetas'])
        ev = ctx.ep(c['thetas'])
        if n == 130:
            ctx.set_ep(0.8, 1e-16, 1000)
            th = c['thetas'][1]
            _, tight, tst, _ = ctx.ep_grad(th[None])
            assert not tst.any()
            fd = gr.central_differences(lambda x: ctx.ep(x[None])[0][0], th)
            worst_fd = np.abs(tight[0] - fd).max() / max(1.0, np.abs(fd).max())
    finally:
        ctx.close()
    assert not st.any() and grad.shape == (4, c['thetas'].shape[1])
    assert np.array_equal(ev[0], logz)
    worst = 0.0
    for t, (th, ref) in enumerate(zip(c['thetas'], refs)):
        assert int(nsw[t]) == ref['n_sweeps']
        scale = max(1.0, np.abs(ref['grad']).max())
        err = max(abs(logz[t] - ref['logz']), np.abs(grad[t] - ref['grad']).max()) / scale
        worst = max(worst, err)
    print('linear EP grad parity {0}: worst {1:.3e} (tol {2:.0e}), vs the device\'s own central '
          'differences {3:.3e} (tol 1e-06)'.format((n, d, kind, bias), worst, TOL, worst_fd))
    assert worst <= TOL
    assert worst_fd <= 1e-6


# ------------------------------------------------------------------ 5. lambda = 0


@pytest.mark.parametrize('kind,bias', cr.LINEAR_KINDS)
def test_lambda_zero_is_the_kind_without_the_flag(nat, kind, bias):
    """theta_lambda = -800 (exp gives exactly 0): Gram, cross-Gram, the IS / PriorMC / Laplace
    theta-calls, the cached u-call and apm_predict are bitwise those of the same kind without the
    flag on the same data; the other gradient entries within 1e-12 relative and lambda's own
    exactly 0."""
    n, d = (130, 5) if kind == 'ard' else (200, 3)
    c = _case('call', 130, 5, 'ard', True) if kind == 'ard' else _case('call', 200, 3, 'iso', True)
    full = c['thetas'][1]
    th0 = full[:-1] if bias else full[:-2]  # (the cases are biased ones: drop log beta too)
    c = dict(c, kind=kind, bias=bias)
    X, y = c['X'], c['y']
    Xs = cc.far_test_inputs(c, 70, FAR)
    thl = np.r_[th0, -800.0]
    nk, nk0 = _cov(kind, bias).native_kind, _cov(kind, bias, False).native_kind
    K, K0 = np.empty((n, n)), np.empty((n, n))
    nat.gram(nk, K, X, thl, EPS)
    nat.gram(nk0, K0, X, th0, EPS)
    assert np.array_equal(K, K0)
    assert np.array_equal(nat.gram_cross(nk, Xs, X, thl), nat.gram_cross(nk0, Xs, X, th0))
    ns = np.random.RandomState(29).normal(size=(n, 8))
    got = []
    for linear, th in ((True, thl), (False, th0)):
        ctx = _ctx(nat, c, n_imp=8, max_batch=1, n_slots=2, n_ubufs=2, linear=linear)
        try:
            ctx.u_upload(0, ns)
            ctx.u_upload(1, ns[:, ::-1].copy())
            r = [ctx.theta_eval(nat.EST_IS, th[None], [0], [0]), ctx.u_eval([0], [1]),
                 ctx.theta_eval(nat.EST_PRIORMC, th[None], [0], [1]),
                 ctx.theta_eval(nat.EST_LAPLACE, th[None]), ctx.predict(th[None], Xs)]
            ctx.set_newton(NEWTON_TOL, 1000)
            r.append(ctx.laplace_grad(th[None]))
            got.append(r)
        finally:
            ctx.close()
    for a, b in zip(got[0][:5], got[1][:5]):
        for x, z in zip(a, b):
            assert np.array_equal(x, z)
    assert not got[0][0][1].any() and not got[0][4][3].any() and not got[0][5][2].any()
    gl, g0 = got[0][5][1][0], got[1][5][1][0]
    assert gl.shape[0] == g0.shape[0] + 1
    assert got[0][5][0][0] == got[1][5][0][0]
    assert np.all(np.abs(gl[:-1] - g0) <= 1e-12 * np.abs(g0))
    assert gl[-1] == 0.0


# ------------------------------------------------------------------ 6. batch neutrality


def test_batches_are_bitwise_neutral(nat):
    """A biased + linear SE-ARD context (130, 5), max_batch = 4: a chain's IS theta-call, gradient
    and predictive outputs are bitwise the same alone, first of 3 and last of 4."""
    c = _case('grad', 130, 5, 'ard', True)
    Xs = cc.far_test_inputs(c, 70, FAR)
    n = c['n']
    rng = np.random.RandomState(5)
    other = c['thetas'][rng.randint(0, 4, size=3)] + rng.uniform(-0.2, 0.2, size=(3, 8))
    U = rng.normal(size=(n, 8))
    ctx = _ctx(nat, c, n_imp=8, max_batch=4, n_slots=4, n_ubufs=4)
    try:
        for q in range(4):
            ctx.u_upload(q, U)
        for th in c['thetas'][[1, 3]]:
            first_th, last_th = np.vstack([th[None], other[:2]]), np.vstack([other, th[None]])
            runs = []
            for x, i in ((th[None], 0), (first_th, 0), (last_th, 3)):
                k = x.shape[0]
                e = ctx.theta_eval(nat.EST_IS, x, list(range(k)), list(range(k)))
                g = ctx.laplace_grad(x)
                p = ctx.predict(x, Xs)
                runs.append([e[0][i], e[1][i], e[2][i], g[0][i], g[1][i], g[2][i], g[3][i],
                             p[0][i], p[1][i], p[2][i], p[3][i], p[4][i]])
            assert runs[0][1] == 0 and runs[0][5] == 0 and runs[0][10] == 0
            assert all(np.all(np.isfinite(v)) for v in runs[0])
            for other_run in runs[1:]:
                for a, b in zip(runs[0], other_run):
                    assert np.array_equal(a, b)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. other contexts


def test_other_contexts_are_unchanged_by_a_linear_one(nat):
    """A base SE-ARD context and a Matern 5/2 ARD + bias context at N = 577: the Laplace
    theta-call, predict, gradient and an IS theta-call with its slot read-back are bitwise the
    same before, while and after a linear context on the same data exists and has run each of its
    entry points."""
    c = _case('call', 577, 4, 'ard', True)
    Xs = cc.far_test_inputs(c, 70, FAR)
    n, d = c['n'], c['d']
    th_base = c['thetas'][:, :d + 1]
    th_m52 = c['thetas'][:, :d + 2]
    U = np.random.RandomState(31).normal(size=(n, 8))

    def record(ctx, thetas):
        ctx.u_upload(0, U)
        out = list(ctx.theta_eval(nat.EST_LAPLACE, thetas))
        out += list(ctx.predict(thetas, Xs)) + list(ctx.laplace_grad(thetas))
        out += list(ctx.theta_eval(nat.EST_IS, thetas[:1], [0], [0]))
        L, f, g, cst = ctx.slot_read(0)
        return out + [L, f, g, np.float64(cst)]

    def use_every_entry_point(ctx, thetas):
        out = record(ctx, thetas)
        out += list(ctx.u_eval([0], [0]))
        out += list(ctx.theta_eval(nat.EST_PRIORMC, thetas[:1], [0], [0]))
        out += list(ctx.theta_eval(nat.EST_IS_EP, thetas[:1], [0], [0]))
        out += list(ctx.is_predict(nat.EST_IS, thetas[:1], [0], [0], Xs))
        out += list(ctx.is_loo([0], [0]))
        out += [x for x in ctx.is_loo_psis([0], [0]) if isinstance(x, np.ndarray)]
        out += list(ctx.ep(thetas)) + list(ctx.ep_predict(thetas, Xs)) + list(ctx.ep_grad(thetas))
        return out
    base = _ctx(nat, c, n_imp=8, kind=nat.KERNEL_ARD)
    m52 = _ctx(nat, c, n_imp=8, kind=nat.KERNEL_M52_ARD | nat.COV_BIAS)
    try:
        before = record(base, th_base) + record(m52, th_m52)
        lin = _ctx(nat, c, n_imp=8)
        try:
            used = use_every_entry_point(lin, c['thetas'])
            while_ = record(base, th_base) + record(m52, th_m52)
            used += use_every_entry_point(lin, c['thetas'])
        finally:
            lin.close()
        after = record(base, th_base) + record(m52, th_m52)
    finally:
        base.close()
        m52.close()
    assert all(np.all(np.isfinite(v)) for v in used[:len(before) // 2])  # (its record() part)
    for a, b, z in zip(before, while_, after):
        assert np.array_equal(a, b) and np.array_equal(a, z)


# ------------------------------------------------------------------ 8. range flags


def test_large_lambda_without_inverse_panels(nat):
    """(130, 5) SE-ARD + linear, theta_0 = 3: log lambda = 8 makes 1 + K_ii,max = 1 + s +
    lambda max|x|^2 + eps exceed 2^15 (no explicit-inverse panels for that chain) while s itself
    would not; beside a (theta_0, log lambda) = (-1, -2) chain each is bitwise what it is alone,
    and the large one is within 5e-4 nats of the oracle or within 10x the oracle's own spread under
    1-ulp noise in K over 8 draws, whichever is larger (measured on the CPU: spread 5.1e-09 nats,
    so 5e-4 decides)."""
    c = _case('call', 130, 5, 'ard', False)
    X, y, n = c['X'], c['y'], c['n']
    th_small = c['thetas'][3]
    th_big = np.r_[c['thetas'][2][:-1], 8.0]
    assert th_big[0] == 3.0 and th_small[-1] == -2.0
    x2 = (X * X).sum(1).max()
    assert 1.0 + math.exp(3.0) + math.exp(8.0) * x2 >= 2.0 ** 15 > 1.0 + math.exp(3.0) + x2
    assert math.log(math.exp(3.0) + math.exp(8.0) * x2) < 19.0
    ns = np.random.RandomState(23).normal(size=(n, 8))
    K = _cov('ard', False).gram(X, th_big, EPS)
    cc.newton_margins(K, y, 1e-4, NEWTON_TOL)
    spread = max(cc.oracle_moves(X, y, ns, K, seed) for seed in range(1, 9))
    ref, _, rops = orc.is_estimate(X, y, _cov('ard', False).kernel_func(EPS), ns, th_big)
    ctx = _ctx(nat, c, n_imp=8, max_batch=2, n_slots=2, n_ubufs=2)
    try:
        ctx.u_upload(0, ns)
        ctx.u_upload(1, ns)
        alone = ctx.theta_eval(nat.EST_IS, th_big[None], [0], [0])
        small = ctx.theta_eval(nat.EST_IS, th_small[None], [0], [1])
        both = ctx.theta_eval(nat.EST_IS, np.vstack([th_small, th_big]), [1, 0], [1, 0])
    finally:
        ctx.close()
    print('linear log lambda 8: |IS - oracle| {0:.2e} nats, oracle spread {1:.2e}'.format(
        abs(alone[0][0] - ref), spread))
    assert alone[1][0] == 0 and small[1][0] == 0 and not both[1].any()
    assert alone[2][0] == rops
    assert abs(alone[0][0] - ref) <= max(TOL_NATS, 10.0 * spread)
    assert both[0][1] == alone[0][0] and both[2][1] == alone[2][0]
    assert both[0][0] == small[0][0] and both[2][0] == small[2][0]


# ------------------------------------------------------------------ 9. Python


def test_python_classes_return_the_native_bits(nat):
    """make_kernel_func('ard', eps, bias=True, linear=True) through the IS estimator,
    LaplacePredictor and LaplaceGradient: the kind comes from kernel_func and the values are the
    binding's own bits."""
    import gpdemo.estimators as est
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    from gpdemo.gradients import LaplaceGradient
    from gpdemo.predict import LaplacePredictor
    c = _case('call', 130, 5, 'ard', True)
    X, y, th = c['X'], c['y'], c['thetas'][1]
    Xs = cc.far_test_inputs(c, 70, FAR)
    kf = krn.make_kernel_func('ard', EPS, bias=True, linear=True)
    assert kf.native_kind == 81
    ns = np.random.RandomState(41).normal(size=(130, 8))
    e = est.LogMarginalLikelihoodApproxPosteriorISEstimator(X, y, kf, lpa.laplace_approximation)
    v, _ = e(ns, th)
    pred = LaplacePredictor(X, y, kf, Xs, max_batch=2)
    gradient = LaplaceGradient(X, y, kf, max_batch=2)
    try:
        mean, var, prob = pred(th)
        lml, grad = gradient(th)
    finally:
        pred.close()
        gradient.close()
    ctx = _ctx(nat, c, n_imp=8, max_batch=2, n_slots=1, n_ubufs=1)
    try:
        ctx.u_upload(0, ns)
        out, st, _ = ctx.theta_eval(nat.EST_IS, th[None], [0], [0])
        p = ctx.predict(th[None], Xs)
        ctx.set_newton(NEWTON_TOL, 1000)
        g = ctx.laplace_grad(th[None])
    finally:
        ctx.close()
    assert st[0] == 0 and v == out[0]
    assert np.array_equal(mean, p[0]) and np.array_equal(var, p[1]) and np.array_equal(prob, p[2])
    assert np.array_equal(lml, g[0]) and np.array_equal(grad, g[1]) and grad.shape == (1, 8)


def test_batched_ess_mh_with_linear(nat):
    """BatchedAPMEllSSPlusMHSampler(kernel='ard', linear=True), 4 chains x 3 iterations at
    N = 65, S = 16: log_f is finite and chain 0's trajectory is bitwise the one it has alone."""
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler as S
    c = _case('call', 65, 4, 'ard', True)
    X, y, d = c['X'], c['y'], c['d']
    prior = dict(a_tau=1., b_tau=1. / d ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(d, np.log(2.)), -1.0], (4, 1))

    def run(chains):
        smp = S(X, y, chains, 16, prior, prop_scales=0.1, seed=31, kernel='ard', linear=True)
        try:
            assert smp.ctx.kind == (nat.KERNEL_ARD | nat.COV_LINEAR) and smp.P == d + 2
            smp.initialise(th0[:chains])
            trace = []
            for it in range(3):
                smp.step()
                trace.append((smp.theta.copy(), smp.log_f.copy()))
            assert not smp.failed.any()
            return trace
        finally:
            smp.ctx.close()
    full, alone = run(4), run(1)
    for (tha, lfa), (thb, lfb) in zip(full, alone):
        assert np.all(np.isfinite(lfa))
        assert np.array_equal(tha[0], thb[0]) and lfa[0] == lfb[0]
    with pytest.raises(ValueError):
        S(X, y, 1, 16, prior, prop_scales=0.1, seed=31, kernel='matern52_ard', linear=True)
