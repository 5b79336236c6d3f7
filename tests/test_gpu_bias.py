"""The constant (bias) covariance term on the device (APM_COV_BIAS): Gram and
cross-Gram, the four estimators' theta-calls, the range flags at a large beta, the three
predictives, the Laplace and EP gradients, beta = 0 against the base kind, batch neutrality, a
base-kind context beside a biased one and a batched sampler - against tests/cov_restatement.py
and the oracle's estimators run with its kernel_func. The maxima measured on an MI355X are in
DESIGN.md §22's parity table."""
import math

import numpy as np
import pytest

import apm_oracle as orc
import cov_checks as cc
import cov_restatement as cr
import epis_restatement as eis
import grad_restatement as gr
import is_predict_restatement as ipr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = 1e-8
TOL_NATS = 5e-4     # estimator values, no relative term
TOL = 1e-9          # fp64 against fp64 through the same factorisation (x max(1, max|ref|))
NEWTON_TOL = 1e-14  # the gradient's Newton tolerance
PROB_TOL = 1e-3     # the IS predictive's averages (2 x the 5e-4 nats of the weights)
FLOOR, CAP = 1e-12, 1e-6  # §19's yardstick rule for its fp64 quantities
# the thetas are drawn for (theta_0, log beta) in (0.3, 3, -1) x (-2, 1.5); the tests use four of
# them (max_batch <= 4): (0.3, -2), (0.3, 1.5), (3, 1.5), (-1, -2)
ROWS = [(s0, lb) for s0 in (0.3, 3.0, -1.0) for lb in (-2.0, 1.5)]
SEL = [0, 1, 3, 4]
FAR = 1000.0  # the far test row: S* underflows to exactly 0 for the Matern kinds too
# (purpose, family, n, d, kind) -> data seed, the first one from 1200 on whose labels are 60-95 %
# positive and for which, at all four thetas, the restatement cannot disagree with the device on
# an iteration count:
#   'grad'    the last Newton diff <= 1e-16 and the one before >= 1e-12 at the gradient's 1e-14
#             (n = 1: >= 1.5e-14), asserted again in the test (test_gpu_grad.test_newton_margins)
#   'epgrad'  the EP fit's last stop measure < 0.99 diff_tol, the one before > 1.01 diff_tol
#   'call'    a factor 3 on both sides of the Newton loop's 1e-4, and the EP margin
SEEDS = {
    ('grad', 'se', 1, 1, 'ard'): 1200, ('grad', '32', 1, 1, 'ard'): 1200,
    ('grad', '52', 1, 1, 'ard'): 1200, ('grad', 'se', 64, 33, 'ard'): 1234,
    ('grad', '32', 64, 33, 'ard'): 1234, ('grad', '52', 64, 33, 'ard'): 1234,
    ('grad', 'se', 130, 5, 'ard'): 1266, ('grad', '32', 130, 5, 'ard'): 1289,
    ('grad', '52', 130, 5, 'ard'): 1354, ('grad', 'se', 200, 3, 'iso'): 1200,
    ('grad', '32', 200, 3, 'iso'): 1201, ('grad', '52', 200, 3, 'iso'): 1202,
    ('grad', 'se', 600, 4, 'ard'): 1207, ('grad', '52', 600, 4, 'ard'): 1207,
    ('epgrad', 'se', 1, 1, 'ard'): 1200, ('epgrad', '52', 64, 33, 'ard'): 1200,
    ('epgrad', 'se', 130, 5, 'ard'): 1200, ('epgrad', '32', 200, 3, 'iso'): 1200,
    ('epgrad', 'se', 600, 4, 'ard'): 1200,
    ('call', 'se', 130, 5, 'ard'): 1201, ('call', '32', 200, 3, 'iso'): 1205,
    ('call', 'se', 65, 4, 'ard'): 1255, ('call', 'se', 513, 4, 'ard'): 1202,
    ('call', 'se', 577, 4, 'ard'): 1200,
}
_CASES = {}


def _case(what, family, n, d, kind):
    """Data of one (purpose, family, shape), drawn once and left unchanged."""
    key = (what, family, n, d, kind)
    if key not in _CASES:
        c = gr.make_case(n, d, kind, SEEDS[key], rows=ROWS, offset=1.0)
        c['family'], c['thetas'] = family, c['thetas'][SEL]
        _CASES[key] = c
    return _CASES[key]


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _cov(family, kind, bias=True):
    return Cov(family, kind, bias=bias)


def _ctx(nat, c, n_imp=1, max_batch=4, n_slots=4, n_ubufs=4, bias=True):
    return nat.Context(c['X'], c['y'], _cov(c['family'], c['kind'], bias).native_kind, EPS, n_imp,
                       max_batch=max_batch, n_slots=n_slots, n_ubufs=n_ubufs)


# ------------------------------------------------------------------ 1. Gram and cross-Gram


def _gram_inputs(n, d, kind, dup, log_beta):
    rng = np.random.RandomState(11 if dup else 5 + n)
    nl = d if kind == 'ard' else 1
    if dup:  # the construction of test_gram_near_duplicate_rows_vs_c_oracle
        base = rng.normal(size=(n // 2, d))
        X = np.concatenate([base, base + 1e-4 * rng.normal(size=base.shape)])[rng.permutation(n)]
        th = np.r_[0.2, rng.normal(scale=0.5, size=nl), log_beta]
    else:
        X = rng.normal(size=(n, d))
        th = np.r_[0.3, rng.normal(size=nl), log_beta]
    return X, th


GRAM_CASES = ([(f, k, n, d, False) for f, k in cr.FAMILY_KINDS for n, d in ((1, 1), (129, 64))] +
              [(f, k, 300, 7, False) for f, k in (('se', 'ard'), ('52', 'iso'))] +
              [(f, k, 200, 3, True) for f, k in (('se', 'ard'), ('52', 'iso'))])


@pytest.mark.parametrize('family,kind,n,d,dup', GRAM_CASES)
def test_gram_vs_restatement(nat, family, kind, n, d, dup):
    """Entry by entry within Cov.gram_bound (the base kind's bound on S plus 3u |K_ref|), log beta
    -2 and 1.5; K exactly symmetric, its diagonal s + beta + eps within 3 ulp, every entry of the
    caller's (n, n) array written (the identity padding stays inside the library)."""
    import gpdemo.kernels as krn
    for log_beta in (-2.0, 1.5):
        X, th = _gram_inputs(n, d, kind, dup, log_beta)
        K = np.full((n, n), np.nan)
        krn.make_kernel_func(_cov(family, kind).name, EPS, bias=True)(K, X, th)
        Kref = _cov(family, kind).gram(X, th, EPS)
        err, bound = np.abs(K - Kref), _cov(family, kind).gram_bound(X, X, th, Kref)
        print('bias gram {0}: max error / bound = {1:.3f}'.format(
            (family, kind, n, d, dup, log_beta), float((err / bound).max())))
        assert np.all(err <= bound)
        assert np.array_equal(K, K.T)
        dg = math.exp(th[0]) + math.exp(log_beta) + EPS
        assert np.all(np.abs(K.diagonal() - dg) <= 3 * np.spacing(dg))
        assert np.all(K >= math.exp(log_beta) * (1 - 1e-15))  # beta everywhere, no padding zeros
        with pytest.raises(IndexError):
            nat.gram(_cov(family, kind).native_kind, K, X, th[:-1], EPS)


@pytest.mark.parametrize('family,kind', cr.FAMILY_KINDS)
@pytest.mark.parametrize('m,n,d', [(70, 130, 5), (1, 129, 40)])
def test_gram_cross_vs_restatement(nat, family, kind, m, n, d):
    """The same bound for k(Xs_i, X_j) + beta; no epsilon where a test point coincides with a
    training point (s + beta of the host's two exps within 1 ulp)."""
    rng = np.random.RandomState(m + n)
    X, Xs = rng.normal(size=(n, d)), rng.normal(size=(m, d))
    Xs[0] = X[7]
    for log_beta in (-2.0, 1.5):
        th = np.r_[0.3, 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=d if kind == 'ard' else 1),
                   log_beta]
        Ks = nat.gram_cross(_cov(family, kind).native_kind, Xs, X, th)
        assert Ks.shape == (m, n)
        ref = _cov(family, kind).gram_cross(Xs, X, th)
        err, bound = np.abs(Ks - ref), _cov(family, kind).gram_bound(Xs, X, th, ref)
        print('bias cross-gram {0}: max error / bound = {1:.3f}'.format(
            (family, kind, m, n, d, log_beta), float((err / bound).max())))
        assert np.all(err <= bound)
        kss = math.exp(th[0]) + math.exp(log_beta)
        assert abs(Ks[0, 7] - kss) <= np.spacing(kss)


# ------------------------------------------------------------------ 2. theta-calls


CALL_CASES = [('se', 130, 5, 'ard'), ('32', 200, 3, 'iso'), ('se', 65, 4, 'ard'),
              ('se', 513, 4, 'ard'), ('se', 577, 4, 'ard')]


@pytest.mark.parametrize('family,n,d,kind', CALL_CASES)
def test_estimators_vs_oracle(nat, family, n, d, kind):
    """IS (theta-call and one cached u-call), PriorMC, Laplace and IS_EP estimates (N_imp = 8)
    against the oracle's estimators with the restatement's kernel_func, at (theta_0, log beta) =
    (0.3, 1.5) and (-1, -2): 5e-4 nats, status 0, the oracle's n_cubic_ops. First, on the CPU: the
    oracle's own IS value moves by less than 5e-5 nats under 1-ulp noise in K."""
    c = _case('call', family, n, d, kind)
    X, y = c['X'], c['y']
    kf = _cov(family, kind).kernel_func(EPS)
    rng = np.random.RandomState(17)
    ns1, ns2 = rng.normal(size=(n, 8)), rng.normal(size=(n, 8))
    ctx = _ctx(nat, c, n_imp=8, max_batch=1, n_slots=2, n_ubufs=2)
    try:
        ctx.u_upload(0, ns1)
        ctx.u_upload(1, ns2)
        for th in c['thetas'][[1, 3]]:
            K = _cov(family, kind).gram(X, th, EPS)
            moves = cc.oracle_moves(X, y, ns1, K)
            assert moves < 5e-5, moves
            r1, rc, rops = orc.is_estimate(X, y, kf, ns1, th)
            r2, _, _ = orc.is_estimate(X, y, kf, ns2, None, rc)
            p1, _, pops = orc.priormc_estimate(X, y, kf, ns1, th)
            lml, lops = orc.laplace_estimate(X, y, kf, th)
            est = eis.state(K, y)
            e1 = eis.is_consistent(y, est, ns1)
            out, st, nops = ctx.theta_eval(nat.EST_IS, th[None], [0], [0])
            out2, st2 = ctx.u_eval([0], [1])
            pm, pst, pnops = ctx.theta_eval(nat.EST_PRIORMC, th[None], [0], [1])
            lp, lst, lnops = ctx.theta_eval(nat.EST_LAPLACE, th[None])
            ep, est_st, enops = ctx.theta_eval(nat.EST_IS_EP, th[None], [0], [1])
            print('bias {0} theta {1}: IS {2:.2e} u-call {3:.2e} PriorMC {4:.2e} Laplace {5:.2e} '
                  'IS_EP {6:.2e} nats (oracle moves {7:.1e})'.format(
                      (family, n, d, kind), (th[0], th[-1]), abs(out[0] - r1), abs(out2[0] - r2),
                      abs(pm[0] - p1), abs(lp[0] - lml), abs(ep[0] - e1), moves))
            assert st[0] == 0 and st2[0] == 0 and pst[0] == 0 and lst[0] == 0 and est_st[0] == 0
            assert nops[0] == rops and pnops[0] == pops and lnops[0] == lops
            assert int(enops[0]) == 2 * est['n_sweeps'] + 3
            assert abs(out[0] - r1) <= TOL_NATS
            assert abs(out2[0] - r2) <= TOL_NATS
            assert abs(pm[0] - p1) <= TOL_NATS
            assert abs(lp[0] - lml) <= TOL_NATS
            assert abs(ep[0] - e1) <= TOL_NATS
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. range flags


def test_large_beta_without_inverse_panels(nat):
    """log beta = 10.6 at theta_0 = 0.3 (1 + K_ii >= 2^15: no explicit-inverse panels) on (130, 5)
    SE-ARD: against the oracle at 5e-4 (its own value moves by less than 5e-5 under 1-ulp noise in
    K), bitwise the same alone and beside a log beta = 1.5 chain, which its neighbour leaves
    bitwise unchanged."""
    c = _case('call', 'se', 130, 5, 'ard')
    X, y, n = c['X'], c['y'], c['n']
    th_big = np.r_[c['thetas'][1][:-1], 10.6]
    th_mid = c['thetas'][1]
    assert th_big[0] == 0.3 and th_mid[-1] == 1.5
    assert 1.0 + math.exp(0.3) + math.exp(10.6) >= 2.0 ** 15
    ns = np.random.RandomState(23).normal(size=(n, 8))
    moves = cc.oracle_moves(X, y, ns, _cov('se', 'ard').gram(X, th_big, EPS))
    assert moves < 5e-5, moves
    ref, _, rops = orc.is_estimate(X, y, _cov('se', 'ard').kernel_func(EPS), ns, th_big)
    ctx = _ctx(nat, c, n_imp=8, max_batch=2, n_slots=2, n_ubufs=2)
    try:
        ctx.u_upload(0, ns)
        ctx.u_upload(1, ns)
        alone = ctx.theta_eval(nat.EST_IS, th_big[None], [0], [0])
        mid = ctx.theta_eval(nat.EST_IS, th_mid[None], [0], [1])
        both = ctx.theta_eval(nat.EST_IS, np.vstack([th_mid, th_big]), [1, 0], [1, 0])
    finally:
        ctx.close()
    print('bias log beta 10.6: |IS - oracle| {0:.2e} nats (oracle moves {1:.1e})'.format(
        abs(alone[0][0] - ref), moves))
    assert alone[1][0] == 0 and mid[1][0] == 0 and not both[1].any()
    assert alone[2][0] == rops
    assert abs(alone[0][0] - ref) <= TOL_NATS
    assert both[0][1] == alone[0][0] and both[2][1] == alone[2][0]
    assert both[0][0] == mid[0][0] and both[2][0] == mid[2][0]


def test_huge_beta_takes_fp32_operands(nat):
    """log beta = 19.5 (the sigma = e^18.5 rule of DESIGN.md §3.3: K_ii >= e^19, fp32 operands):
    status 0, a finite value, and within 10x the oracle's own spread under 1-ulp noise in K,
    measured here on the CPU over 8 noise draws."""
    c = _case('call', 'se', 130, 5, 'ard')
    X, y, n = c['X'], c['y'], c['n']
    th = np.r_[c['thetas'][1][:-1], 19.5]
    ns = np.random.RandomState(23).normal(size=(n, 8))
    K = _cov('se', 'ard').gram(X, th, EPS)
    spread = max(cc.oracle_moves(X, y, ns, K, seed) for seed in range(1, 9))
    ref, _, _ = orc.is_estimate(X, y, _cov('se', 'ard').kernel_func(EPS), ns, th)
    ctx = _ctx(nat, c, n_imp=8, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        ctx.u_upload(0, ns)
        out, st, _ = ctx.theta_eval(nat.EST_IS, th[None], [0], [0])
    finally:
        ctx.close()
    print('bias log beta 19.5: |IS - oracle| {0:.2e} nats, oracle spread {1:.2e}'.format(
        abs(out[0] - ref), spread))
    assert st[0] == 0 and np.isfinite(out[0])
    assert abs(out[0] - ref) <= 10.0 * spread


# ------------------------------------------------------------------ 4. prediction


PREDICT_CASES = [('se', 130, 5, 'ard'), ('se', 577, 4, 'ard')]


def _far_row(c, th, ref, mean_far, prob_far):
    """The far test row is not the prior: k* = beta there, so the restatement's mean is
    beta sum(a) (the device's is within the parity tolerance of it), and the class probability is
    on the majority's side of 0.5."""
    beta, a = math.exp(th[-1]), ref['a']
    assert (c['y'] > 0).mean() > 0.5
    assert abs(ref['mean'][-1] - beta * a.sum()) <= 1e-12 * max(1.0, beta * np.abs(a).sum())
    assert mean_far != 0.0 and prob_far > 0.5 and ref['prob'][-1] > 0.5


@pytest.mark.parametrize('family,n,d,kind', PREDICT_CASES)
def test_laplace_and_ep_predict_vs_restatement(nat, family, n, d, kind):
    """apm_predict and apm_ep_predict at m = 70: mean and var relative to max(1, max|ref|), prob
    absolute, at 1e-9, equal iteration / sweep counts; the far test row equals the restatement and
    is not the prior."""
    c = _case('call', family, n, d, kind)
    Xs = cc.far_test_inputs(c, 70, FAR)
    ctx = _ctx(nat, c)
    try:
        lp = ctx.predict(c['thetas'], Xs)
        epd = ctx.ep_predict(c['thetas'], Xs)
    finally:
        ctx.close()
    assert not lp[3].any() and not epd[3].any()
    for t, th in enumerate(c['thetas']):
        ref = cr.predictive(_cov(family, kind), c['X'], c['y'], Xs, th, EPS)
        eref = cr.ep_predictive(_cov(family, kind), c['X'], c['y'], Xs, th, EPS)
        w_l, w_e = cc.worst([x[t] for x in lp[:3]], ref), cc.worst([x[t] for x in epd[:3]], eref)
        print('bias predict {0} theta {1}: Laplace {2:.2e} EP {3:.2e} (tol {4:.0e}), far prob '
              '{5:.4f}'.format((family, n, d, kind), (th[0], th[-1]), w_l, w_e, TOL, lp[2][t, -1]))
        assert int(lp[4][t]) == ref['n_iter'] and int(epd[4][t]) == eref['n_sweeps']
        assert w_l <= TOL and w_e <= TOL
        _far_row(c, th, ref, lp[0][t, -1], lp[2][t, -1])
        assert epd[0][t, -1] != 0.0 and epd[2][t, -1] > 0.5
        kss = math.exp(th[0]) + math.exp(th[-1])
        assert np.all(lp[1][t] > 0.0) and np.all(lp[1][t] <= kss)


@pytest.mark.parametrize('family,n,d,kind', PREDICT_CASES)
@pytest.mark.parametrize('proposal', ['laplace', 'ep'])
def test_is_predict_vs_restatement(nat, family, n, d, kind, proposal, monkeypatch):
    """apm_is_predict with both proposals at (theta_0, log beta) = (0.3, 1.5), m = 70, S = 64.
    DESIGN.md §19's yardstick rule for the fp64 quantities c_j and v*_j (read off a one-sample
    context with a zero U column, fp64 Newton): 10x the restatement's own float64-to-longdouble
    discrepancy, floored at 1e-12, the discrepancy capped at 1e-6; prob, mean, var and ess of the
    default path at 1e-3. The far test row's mean is beta sum(a)-sized, not 0."""
    c = _case('call', family, n, d, kind)
    Xs = cc.far_test_inputs(c, 70, FAR)
    th = c['thetas'][1]
    K = _cov(family, kind).gram(c['X'], th, EPS)
    Ks = _cov(family, kind).gram_cross(Xs, c['X'], th)
    kss = _cov(family, kind).prior_var(Xs, th)
    U = np.random.RandomState(107).normal(size=(n, 64)).astype(np.float32).astype(np.float64)
    fit = eis.state(K, c['y']) if proposal == 'ep' else eis.laplace_state(K, c['y'])
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
        print('bias is_predict {0} {1} {2}: device {3:.2e} yardstick {4:.2e}'.format(
            (family, n, d, kind), proposal, key, err, yard))
        assert yard < CAP
        assert err <= max(10.0 * yard, FLOOR)
    mscale = max(1.0, float(np.abs(ref['m']).max()))
    d_prob = float(np.abs(prob[0] - ref['prob']).max())
    d_mean = float(np.abs(mean[0] - ref['mean']).max()) / mscale
    d_var = float(np.abs(var[0] - ref['var']).max()) / max(1.0, mscale ** 2)
    d_ess = abs(ess[0] - ref['ess']) / ref['ess']
    print('bias is_predict {0} {1}: d prob {2:.2e} d mean {3:.2e} d var {4:.2e} d ess {5:.2e}'
          .format((family, n, d, kind), proposal, d_prob, d_mean, d_var, d_ess))
    assert d_prob <= PROB_TOL and d_mean <= PROB_TOL and d_var <= PROB_TOL and d_ess <= PROB_TOL
    assert np.all(Ks[-1] == math.exp(th[-1]))  # k* = beta exactly at the far test row
    assert cdev[0, -1] != 0.0 and prob[0, -1] > 0.5


# ------------------------------------------------------------------ 5. gradients


GRAD_CASES = [(f, 1, 1, 'ard') for f in cr.FAMILIES] + [(f, 64, 33, 'ard') for f in cr.FAMILIES] + \
             [(f, 130, 5, 'ard') for f in cr.FAMILIES] + [(f, 200, 3, 'iso') for f in cr.FAMILIES] + \
             [('se', 600, 4, 'ard'), ('52', 600, 4, 'ard')]


@pytest.mark.parametrize('family,n,d,kind', GRAD_CASES)
def test_laplace_grad_vs_restatement_and_central_differences(nat, family, n, d, kind):
    """lml and all P gradient entries against the restatement at 1e-9 of max(1, max|ref grad|)
    with equal Newton iteration counts (the margins asserted first, on the CPU); against central
    differences (h = 1e-5) of the restatement's converged LML at 1e-6 for one theta of each beta
    (n = 600: the first theta);
    lml bitwise the Laplace theta-call's at the same Newton settings."""
    c = _case('grad', family, n, d, kind)
    refs = [cr.laplace_grad(_cov(family, kind), c['X'], c['y'], th, EPS, tol=NEWTON_TOL)
            for th in c['thetas']]
    for ref in refs:
        assert ref['diffs'][-1] <= NEWTON_TOL / 100.0
        assert ref['diffs'][-2] >= (1.5 if n == 1 else 100.0) * NEWTON_TOL
    ctx = _ctx(nat, c)
    try:
        ctx.set_newton(NEWTON_TOL, 1000)
        lml, grad, st, nit = ctx.laplace_grad(c['thetas'])
        val, vst, nops = ctx.theta_eval(nat.EST_LAPLACE, c['thetas'])
    finally:
        ctx.close()
    assert not st.any() and not vst.any() and grad.shape == (4, c['thetas'].shape[1])
    assert np.array_equal(val, lml) and np.array_equal(nops, nit)
    worst = worst_fd = 0.0
    for t, (th, ref) in enumerate(zip(c['thetas'], refs)):
        assert int(nit[t]) == ref['n_iter']
        scale = max(1.0, np.abs(ref['grad']).max())
        err = max(abs(lml[t] - ref['lml']), np.abs(grad[t] - ref['grad']).max()) / scale
        worst = max(worst, err)
        if t < (1 if n >= 600 else 2):
            fd = gr.central_differences(
                lambda x: cr.lml(_cov(family, kind), c['X'], c['y'], x, EPS, tol=1e-24), th)
            worst_fd = max(worst_fd, np.abs(grad[t] - fd).max() / max(1.0, np.abs(fd).max()))
        assert grad[t, -1] != 0.0
    print('bias grad parity {0}: worst {1:.3e} (tol {2:.0e}), vs fd {3:.3e} (tol 1e-06)'
          .format((family, n, d, kind), worst, TOL, worst_fd))
    assert worst <= TOL
    assert worst_fd <= 1e-6


EP_GRAD_CASES = [('se', 1, 1, 'ard'), ('52', 64, 33, 'ard'), ('se', 130, 5, 'ard'),
                 ('32', 200, 3, 'iso'), ('se', 600, 4, 'ard')]


@pytest.mark.parametrize('family,n,d,kind', EP_GRAD_CASES)
def test_ep_grad_vs_restatement_and_central_differences(nat, family, n, d, kind):
    """log Z_EP and all P entries of its gradient against the restatement at 1e-9 of max(1,
    max|ref grad|), equal sweep counts (the stop margins asserted first, on the CPU); against
    central differences (h = 1e-5) of log Z_EP fitted to diff_tol = 1e-16 at 1e-6, for one theta
    of each beta (n = 600: the first theta) with the device fitted as tightly."""
    c = _case('epgrad', family, n, d, kind)
    refs = [cr.ep_grad(_cov(family, kind), c['X'], c['y'], th, EPS) for th in c['thetas']]
    for ref in refs:
        m = ref['fit']['m_hist']
        assert m[-1] < 0.99e-8 and (len(m) < 2 or m[-2] > 1.01e-8)
    ctx = _ctx(nat, c)
    try:
        logz, grad, st, nsw = ctx.ep_grad(c['thetas'])
        ctx.set_ep(0.8, 1e-16, 1000)
        _, tight, tst, _ = ctx.ep_grad(c['thetas'][:2])
    finally:
        ctx.close()
    assert not st.any() and not tst.any() and grad.shape == (4, c['thetas'].shape[1])
    worst = worst_fd = 0.0
    for t, (th, ref) in enumerate(zip(c['thetas'], refs)):
        assert int(nsw[t]) == ref['n_sweeps']
        scale = max(1.0, np.abs(ref['grad']).max())
        err = max(abs(logz[t] - ref['logz']), np.abs(grad[t] - ref['grad']).max()) / scale
        worst = max(worst, err)
        if t < (1 if n >= 600 else 2):
            fd = gr.central_differences(
                lambda x: cr.ep_logz(_cov(family, kind), c['X'], c['y'], x, EPS, diff_tol=1e-16,
                                     max_sweeps=1000), th)
            worst_fd = max(worst_fd, np.abs(tight[t] - fd).max() / max(1.0, np.abs(fd).max()))
    print('bias EP grad parity {0}: worst {1:.3e} (tol {2:.0e}), vs fd {3:.3e} (tol 1e-06)'
          .format((family, n, d, kind), worst, TOL, worst_fd))
    assert worst <= TOL
    assert worst_fd <= 1e-6


# ------------------------------------------------------------------ 6. beta = 0


@pytest.mark.parametrize('family,kind', cr.FAMILY_KINDS)
def test_beta_zero_is_the_base_kind(nat, family, kind):
    """theta_b = -800 (exp gives exactly 0): Gram, cross-Gram, the IS / PriorMC / Laplace
    theta-calls, the cached u-call and apm_predict are bitwise the base kind's on the same data;
    the first P0 gradient entries within 1e-12 relative of the base kind's and the last one
    exactly 0."""
    n, d = (130, 5) if kind == 'ard' else (200, 3)
    c = _case('call', 'se', 130, 5, 'ard') if kind == 'ard' else _case('call', '32', 200, 3, 'iso')
    c = dict(c, family=family)
    X, y = c['X'], c['y']
    Xs = cc.far_test_inputs(c, 70, FAR)
    th0 = c['thetas'][1][:-1]
    thb = np.r_[th0, -800.0]
    nk, nk0 = _cov(family, kind).native_kind, _cov(family, kind, False).native_kind
    K, K0 = np.empty((n, n)), np.empty((n, n))
    nat.gram(nk, K, X, thb, EPS)
    nat.gram(nk0, K0, X, th0, EPS)
    assert np.array_equal(K, K0)
    assert np.array_equal(nat.gram_cross(nk, Xs, X, thb), nat.gram_cross(nk0, Xs, X, th0))
    ns = np.random.RandomState(29).normal(size=(n, 8))
    got = []
    for bias, th in ((True, thb), (False, th0)):
        ctx = _ctx(nat, c, n_imp=8, max_batch=1, n_slots=2, n_ubufs=2, bias=bias)
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
    gb, g0 = got[0][5][1][0], got[1][5][1][0]
    assert gb.shape[0] == g0.shape[0] + 1
    assert got[0][5][0][0] == got[1][5][0][0]
    assert np.all(np.abs(gb[:-1] - g0) <= 1e-12 * np.abs(g0))
    assert gb[-1] == 0.0


# ------------------------------------------------------------------ 7. batch neutrality


def test_batches_are_bitwise_neutral(nat):
    """A biased Matern 5/2 ARD context (130, 5), max_batch = 4: a chain's IS theta-call, gradient
    and predictive outputs are bitwise the same alone, first of 3 and last of 4."""
    c = _case('grad', '52', 130, 5, 'ard')
    Xs = cc.far_test_inputs(c, 70, FAR)
    n = c['n']
    rng = np.random.RandomState(5)
    other = c['thetas'][rng.randint(0, 4, size=3)] + rng.uniform(-0.2, 0.2, size=(3, 7))
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


# ------------------------------------------------------------------ 8. a base-kind context


def test_base_kind_context_is_unchanged_by_a_biased_one(nat):
    """A base SE-ARD context's Laplace theta-call, predict, gradient and IS theta-call with its
    slot read-back are bitwise the same before and after a biased context on the same data is
    created and used in the same process."""
    c = _case('call', 'se', 130, 5, 'ard')
    Xs = cc.far_test_inputs(c, 70, FAR)
    n = c['n']
    th0 = c['thetas'][:, :-1]
    U = np.random.RandomState(31).normal(size=(n, 8))

    def record(ctx, thetas):
        ctx.u_upload(0, U)
        out = list(ctx.theta_eval(nat.EST_LAPLACE, thetas))
        out += list(ctx.predict(thetas, Xs)) + list(ctx.laplace_grad(thetas))
        out += list(ctx.theta_eval(nat.EST_IS, thetas[:1], [0], [0]))
        L, f, g, cst = ctx.slot_read(0)
        return out + [L, f, g, np.float64(cst)]
    base = _ctx(nat, c, n_imp=8, bias=False)
    try:
        before = record(base, th0)
        biased = _ctx(nat, c, n_imp=8)
        try:
            used = record(biased, c['thetas'])
            after = record(base, th0)
        finally:
            biased.close()
        again = record(base, th0)
    finally:
        base.close()
    assert all(np.all(np.isfinite(v)) for v in used)
    for a, b, z in zip(before, after, again):
        assert np.array_equal(a, b) and np.array_equal(a, z)


# ------------------------------------------------------------------ 9. batched sampler


def test_batched_ess_mh_with_bias(nat, tmp_path):
    """BatchedAPMEllSSPlusMHSampler(kernel='ard', bias=True), 4 chains x 5 iterations at N = 130,
    S = 16: every chain's trajectory is bitwise the same chain run alone, predict() leaves the
    trajectory unchanged, and a checkpoint -> restore continues bitwise."""
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler as S
    c = _case('call', 'se', 130, 5, 'ard')
    X, y, d = c['X'], c['y'], c['d']
    Xs = cc.far_test_inputs(c, 70, FAR)
    prior = dict(a_tau=1., b_tau=1. / d ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(d, np.log(2.)), 0.5], (4, 1))

    def run(chains, first_chain=0, with_predict=False, split=None):
        smp = S(X, y, chains, 16, prior, prop_scales=0.1, seed=31, kernel='ard', bias=True,
                first_chain=first_chain)
        try:
            assert smp.ctx.kind == (nat.KERNEL_ARD | nat.COV_BIAS) and smp.P == d + 2
            smp.initialise(th0[first_chain:first_chain + chains])
            trace, ck = [], None
            for it in range(5):
                smp.step()
                if with_predict:
                    prob, ess = smp.predict(Xs)
                    assert np.all(np.isfinite(prob)) and np.all(prob[:, -1] != 0.5)
                trace.append((smp.theta.copy(), smp.log_f.copy()))
                if split == it:
                    np.savez(tmp_path / 'ck.npz', **smp.checkpoint())
            assert not smp.failed.any()
            return trace
        finally:
            smp.ctx.close()
    full = run(4, split=1)
    for ch in range(4):
        alone = run(1, first_chain=ch)
        for (tha, lfa), (thb, lfb) in zip(full, alone):
            assert np.array_equal(tha[ch], thb[0]) and lfa[ch] == lfb[0]
    for (tha, lfa), (thb, lfb) in zip(full, run(4, with_predict=True)):
        assert np.array_equal(tha, thb) and np.array_equal(lfa, lfb)
    smp = S(X, y, 4, 16, prior, prop_scales=0.1, seed=31, kernel='ard', bias=True)
    try:
        with np.load(tmp_path / 'ck.npz') as z:
            assert smp.restore({k: z[k] for k in z.files}) == 0.
        for it in range(2, 5):
            smp.step()
            assert np.array_equal(smp.theta, full[it][0]) and np.array_equal(smp.log_f, full[it][1])
    finally:
        smp.ctx.close()
