"""The importance-sampling predictive on the device (apm_is_predict; is_predict.hip,
host_is_predict.cpp) against the numpy restatement (is_predict_restatement.py) on
the C oracle's Gram, plus what needs no restatement: log f bitwise the theta-call's, batch
independence, that such a call leaves every other path's bits alone, failure handling, refusals,
the logit and the batched sampler's predict()."""
import math

import numpy as np
import pytest

import epis_restatement as eis
import is_predict_restatement as ipr
import logit_restatement as lr
from cov_restatement import Cov
from test_gpu_ep import _other_paths, kind_code
from test_gpu_predict import _make_case

pytestmark = pytest.mark.gpu

EPS = 1e-8
# prob: the weights ride on the fp32 C_chol.U, whose estimator tolerance is 5e-4 nats (DESIGN.md
# §3.3); a relative weight change delta moves a [0, 1]-valued self-normalised average by at most
# 2 delta. The same bound scales mean by max(1, max_s |m_sj|); ess is relative.
PROB_TOL = 1e-3
# the fp64 quantities (c, v*, m_sj): 10x the restatement's own float64-to-longdouble discrepancy
# (the factor allows for the blocked solves' other summation order), floored at FLOOR, and the
# discrepancy itself capped at CAP, both x max(1, max|ref|)
FLOOR, CAP = 1e-12, 1e-6
N_PROBE = 3  # sample columns whose m_sj the single-sample contexts expose

# (name, n, d, m, kind, family, theta index, S, seed): test_gpu_predict's three shapes with their
# three thetas (theta_0 = 0.3, 3, -1), the panel edges at d = 4 (nb = 2, 9, 10) and one Matern 5/2
CASES = [('130x5', 130, 5, 70, 'ard', None, t, 64, 100) for t in range(3)] + \
        [('129x40', 129, 40, 1, 'ard', None, t, 100, 101) for t in range(3)] + \
        [('200x3', 200, 3, 70, 'iso', None, t, 100, 102) for t in range(3)] + \
        [('N65', 65, 4, 70, 'ard', None, 0, 64, 365), ('N513', 513, 4, 1, 'ard', None, 1, 100, 813),
         ('N577', 577, 4, 70, 'ard', None, 2, 64, 877),
         ('N513-m52', 513, 4, 70, 'ard', '52', 0, 64, 813)]
# (case index, proposal, likelihood) of every parity run
RUNS = [(i, 'laplace', 'probit') for i in range(len(CASES))] + \
       [(i, 'ep', 'probit') for i in (0, 1, 2, 9)] + [(i, 'laplace', 'logit') for i in (0, 1, 2)]


def _draws(n, S, seed):
    """N(0, 1) draws that fp32 holds exactly (the device keeps U in both precisions)."""
    return np.random.RandomState(seed).normal(size=(n, S)).astype(np.float32).astype(np.float64)


def _grams(c, family, th):
    """K (with epsilon) and k* (without) on the C oracle's Gram; the Matern ones from their
    restatement (the oracle's C Gram knows the SE family only)."""
    import apm_oracle as orc
    n, m = c['n'], c['m']
    if family:
        return (Cov(family, c['kind']).gram(c['X'], th, EPS),
                Cov(family, c['kind']).gram_cross(c['Xs'], c['X'], th))
    G = np.empty((n + m, n + m))
    orc.c_gram(c['kind'], G, np.concatenate([c['X'], c['Xs']]), th, EPS)
    return G[:n, :n].copy(), G[n:, :n].copy()


def _fit(K, y, proposal, likelihood):
    if likelihood == 'logit':
        return lr.is_state(K, y)
    return eis.state(K, y) if proposal == 'ep' else eis.laplace_state(K, y)


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


@pytest.fixture(scope='module')
def refs():
    """Per run: the case, the restatement in float64 and the long double yardstick of its fp64
    quantities, computed once and left unchanged. The cap on the yardstick is checked here."""
    data, out = {}, []
    for i, prop, lik in RUNS:
        name, n, d, m, kind, family, t, S, seed = CASES[i]
        if (n, d, m, kind, seed) not in data:
            data[n, d, m, kind, seed] = _make_case(n, d, m, kind, seed)
        c = data[n, d, m, kind, seed]
        th = c['thetas'][t]
        K, Ks = _grams(c, family, th)
        s = math.exp(th[0])
        U = _draws(n, S, seed + 7)
        fit = _fit(K, c['y'], prop, lik)
        ref = ipr.predictive(K, Ks, s, c['y'], U, fit, lik)
        hi = ipr.h_route(K, Ks, s, fit['W'], fit['a'], U[:, :N_PROBE], dtype=np.longdouble)
        yard = {}
        for key, a64 in (('c', ref['c']), ('vstar', ref['vstar']), ('m', ref['m'][:, :N_PROBE])):
            scale = max(1.0, float(np.abs(a64).max()))
            yard[key] = float(np.abs(a64 - hi[key]).max()) / scale
            assert yard[key] < CAP, (name, key, yard[key])
        out.append(dict(c=c, th=th, U=U, ref=ref, yard=yard, fit=fit, S=S, family=family, Ks=Ks,
                        label='{0} theta_0 {1} {2}/{3}'.format(name, th[0], prop, lik)))
    return out


def _kind(nat, c, family):
    if family == '52':
        return nat.KERNEL_M52_ARD
    return kind_code(nat, c['kind'])


def _est(nat, proposal):
    return nat.EST_IS_EP if proposal == 'ep' else nat.EST_IS


@pytest.mark.parametrize('ri', range(len(RUNS)))
def test_fp64_quantities_vs_restatement(nat, refs, ri, monkeypatch):
    """c_j, v*_j and m_sj, fp64 against fp64. The C-ABI returns averages, so they are read off
    contexts with ONE sample (wbar = 1 exactly): chain q < 3 carries column q of U (mean = m_qj),
    the fourth chain a zero column (mean = c_j, var = v*_j). The Laplace proposal's fit runs with
    its fp64 Newton factorisation here (APM_MIXED=0), so that the comparison sees the tail alone:
    the mixed-precision Newton's a and W differ from the restatement's by its own solve
    tolerance, which the prob / mean / ess test below covers on the default path.
    Measured on an MI355X (DESIGN.md §19 has every case): the device's figure is 0.7 to 23 times
    the yardstick where the floor decides (at most 1.1e-13 there) and at most 6.6 times the
    yardstick where that decides; the largest, m_sj at (200, 3) theta_0 = 3: device 1.1e-07,
    yardstick 3.2e-08."""
    r = refs[ri]
    _, prop, lik = RUNS[ri]
    c, n = r['c'], r['c']['n']
    monkeypatch.setenv('APM_MIXED', '0')
    ctx = nat.Context(c['X'], c['y'], _kind(nat, c, r['family']), EPS, 1, max_batch=4, n_slots=4,
                      n_ubufs=4, likelihood=lik)
    try:
        for q in range(N_PROBE):
            ctx.u_upload(q, r['U'][:, q:q + 1])
        ctx.u_upload(N_PROBE, np.zeros((n, 1)))
        _, _, mean, var, ess, st, _ = ctx.is_predict(_est(nat, prop), np.tile(r['th'], (4, 1)),
                                                     np.arange(4), np.arange(4), c['Xs'])
    finally:
        ctx.close()
    assert not st.any() and np.all(ess == 1.0)
    ref = r['ref']
    for key, dev, a64 in (('c', mean[3], ref['c']), ('vstar', var[3], ref['vstar']),
                          ('m', mean[:3].T, ref['m'][:, :N_PROBE])):
        scale = max(1.0, float(np.abs(a64).max()))
        err = float(np.abs(dev - a64).max()) / scale
        bound = max(10.0 * r['yard'][key], FLOOR)
        print('{0} {1}: device {2:.2e} yardstick {3:.2e} bound {4:.2e}'.format(
            r['label'], key, err, r['yard'][key], bound))
        assert err <= bound, (key, err, bound)


@pytest.mark.parametrize('ri', range(len(RUNS)))
def test_prob_mean_ess_vs_restatement(nat, refs, ri):
    """The default (mixed-precision) path at S = 64 / 100 against the restatement, and log f
    bitwise the theta-call's on the same context, theta, U buffer and slot. Measured on an MI355X
    (DESIGN.md §19): worst |d prob| 1.8e-07, |d mean| 3.6e-07, |d var| 4.3e-08, ess 1.2e-06
    relative, log f within 5.1e-06 nats of the restatement's."""
    r = refs[ri]
    _, prop, lik = RUNS[ri]
    c, ref = r['c'], r['ref']
    ctx = nat.Context(c['X'], c['y'], _kind(nat, c, r['family']), EPS, r['S'], max_batch=1,
                      n_slots=1, n_ubufs=1, likelihood=lik)
    try:
        ctx.u_upload(0, r['U'])
        logf0, st0, nops0 = ctx.theta_eval(_est(nat, prop), r['th'][None], [0], [0])
        logf, prob, mean, var, ess, st, nops = ctx.is_predict(_est(nat, prop), r['th'][None], [0],
                                                              [0], c['Xs'])
        U_after = ctx.u_download(0)
    finally:
        ctx.close()
    assert st0[0] == 0 and st[0] == 0
    assert logf[0] == logf0[0]                       # bitwise
    assert int(nops[0]) == int(nops0[0]) + 2         # the tail's two factorisations
    np.testing.assert_array_equal(U_after, r['U'])   # the U buffer is not modified
    mscale = max(1.0, float(np.abs(ref['m']).max()))
    d_prob = float(np.abs(prob[0] - ref['prob']).max())
    d_mean = float(np.abs(mean[0] - ref['mean']).max()) / mscale
    d_var = float(np.abs(var[0] - ref['var']).max()) / max(1.0, mscale ** 2)
    d_ess = abs(ess[0] - ref['ess']) / ref['ess']
    print('{0}: d logf {1:.2e} d prob {2:.2e} d mean {3:.2e} d var {4:.2e} d ess {5:.2e} (ess '
          '{6:.1f} of {7})'.format(r['label'], abs(logf[0] - ref['logf']), d_prob, d_mean, d_var,
                                   d_ess, ess[0], r['S']))
    assert d_prob <= PROB_TOL and d_mean <= PROB_TOL and d_var <= PROB_TOL and d_ess <= PROB_TOL
    assert 1.0 <= ess[0] <= r['S']
    if c['m'] >= 3 and not r['Ks'][-1].any():  # the far test point where k* = 0 exactly (SE)
        assert abs(prob[0, -1] - 0.5) <= 1e-15 and mean[0, -1] == 0.0
        assert var[0, -1] == math.exp(r['th'][0])


def _three(nat):
    """(case, context) with one U in three buffers: three thetas of (130, 5) whose fits take
    different iteration counts."""
    c = _make_case(130, 5, 70, 'ard', 100)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 100, max_batch=4, n_slots=4, n_ubufs=4)
    U = _draws(130, 100, 5)
    for q in range(3):
        ctx.u_upload(q, U)
    return c, ctx


@pytest.mark.parametrize('proposal', ['laplace', 'ep'])
def test_batch_independence(nat, proposal):
    """Three thetas in one call (max_batch = 4) and one by one: the same bits in every output."""
    est = _est(nat, proposal)
    c, ctx = _three(nat)
    try:
        idx = np.arange(3)
        together = ctx.is_predict(est, c['thetas'], idx, idx, c['Xs'])
        alone = [ctx.is_predict(est, c['thetas'][q:q + 1], [q], [q], c['Xs']) for q in range(3)]
    finally:
        ctx.close()
    assert not together[5].any()
    assert len(set(int(x) for x in together[6])) > 1  # (different Newton / sweep counts)
    for q in range(3):
        for a, b in zip(together, alone[q]):
            np.testing.assert_array_equal(a[q], b[0])


def test_other_paths_keep_their_bits(nat):
    """N = 577: the Laplace theta-call, predict, laplace_grad, an IS theta-call with its u-call
    and slot read-back, and apm_ep_eval, before and after an apm_is_predict (both proposals) on
    the same context: bitwise the same."""
    c = _make_case(577, 4, 3, 'ard', 300 + 577)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=2, n_slots=2, n_ubufs=2)
    try:
        before = _other_paths(nat, ctx, c) + list(ctx.ep(c['thetas'][:2]))
        for est in (nat.EST_IS, nat.EST_IS_EP):
            st = ctx.is_predict(est, c['thetas'][:2], [0, 1], [0, 1], c['Xs'])[5]
            assert not st.any()
        after = _other_paths(nat, ctx, c) + list(ctx.ep(c['thetas'][:2]))
    finally:
        ctx.close()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('proposal', ['laplace', 'ep'])
def test_failed_fit_gives_its_status_and_nan_rows(nat, proposal):
    """max_iters / max_sweeps = 2: theta_0 = 3 cannot converge, theta_0 = -14 (K ~ 1e-6) does. The
    failed chain returns APM_STATUS_MAXITER and NaN rows; the other one the bits of a call of
    its own."""
    est = _est(nat, proposal)
    c, ctx = _three(nat)
    try:
        if proposal == 'ep':
            ctx.set_ep(0.8, 1e-8, 2)
        else:
            ctx.set_newton(1e-4, 2)
        th = np.stack([c['thetas'][1], np.r_[-14.0, c['thetas'][1][1:]]])
        both = ctx.is_predict(est, th, [0, 1], [0, 1], c['Xs'])
        good = ctx.is_predict(est, th[1:], [1], [1], c['Xs'])
    finally:
        ctx.close()
    assert both[5][0] == nat.STATUS_MAXITER and both[5][1] == 0 and good[5][0] == 0
    for k in (1, 2, 3):
        assert np.isnan(both[k][0]).all()
    assert np.isnan(both[4][0])
    for a, b in zip(both, good):
        np.testing.assert_array_equal(a[1], b[0])
    assert np.isfinite(good[1]).all()


def test_refusals(nat):
    c = _make_case(130, 5, 70, 'ard', 100)
    lib = nat.load_library()
    th = np.ascontiguousarray(c['thetas'][:1])
    idx = np.zeros(1, dtype=np.int64)
    out, st = np.zeros(1), np.zeros(1, dtype=np.int32)

    def call(ctx, est, count=1, Xs=c['Xs']):
        Xs = np.ascontiguousarray(Xs)
        return lib.apm_is_predict(ctx._h, est, count, th.ctypes.data, th.shape[1],
                                  idx.ctypes.data, idx.ctypes.data, Xs.ctypes.data, Xs.shape[0],
                                  Xs.shape[1], out.ctypes.data, None, None, None, Xs.shape[0],
                                  None, st.ctypes.data, None)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        assert call(ctx, nat.EST_PRIORMC) == nat.APM_E_INVALID
        assert call(ctx, nat.EST_LAPLACE) == nat.APM_E_INVALID
        assert call(ctx, nat.EST_IS, count=2) == nat.APM_E_INVALID  # count > max_batch
        ctx.u_upload(0, _draws(130, 8, 1))
        assert call(ctx, nat.EST_IS) == 0 and st[0] == 0            # every output may be NULL
    finally:
        ctx.close()
    ctx = nat.Context(None, c['y'], nat.KERNEL_PRECOMPUTED, EPS, 8, max_batch=1, n_slots=1,
                      n_ubufs=1)
    try:
        assert call(ctx, nat.EST_IS) == nat.APM_E_INVALID
    finally:
        ctx.close()
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=1, n_slots=1, n_ubufs=1,
                      likelihood='logit')
    try:
        assert call(ctx, nat.EST_IS_EP) == nat.APM_E_INVALID
    finally:
        ctx.close()


def test_batched_sampler_predict(nat):
    """BatchedAPMEllSSPlusMHSampler, 4 chains, N = 130, S = 64: six steps with predict() after
    every step give bitwise the theta and log f trajectories of six steps without it, and the
    returned prob is ISPredictor's on the downloaded (theta, u)."""
    import gpdemo.kernels as krn
    import gpdemo.predict as prd
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler
    c = _make_case(130, 5, 70, 'ard', 100)
    prior = dict(a_tau=1., b_tau=1. / 5 ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(5, np.log(2.))], (4, 1))

    def run(with_predict):
        smp = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 4, 64, prior, prop_scales=0.1, seed=31)
        smp.initialise(th0)
        trace, last = [], None
        for _ in range(6):
            smp.step()
            if with_predict:
                last = smp.predict(c['Xs'])
            trace.append((smp.theta.copy(), smp.log_f.copy()))
        return smp, trace, last
    plain, t0, _ = run(False)
    plain.ctx.close()
    smp, t1, (prob, ess) = run(True)
    try:
        for (tha, lfa), (thb, lfb) in zip(t0, t1):
            np.testing.assert_array_equal(tha, thb)
            np.testing.assert_array_equal(lfa, lfb)
        assert not smp.failed.any() and prob.shape == (4, 70)
        us = np.stack([smp.ctx.u_download(smp.ub_u[q]) for q in range(4)])
        theta = smp.theta.copy()
    finally:
        smp.ctx.close()
    p = prd.ISPredictor(c['X'], c['y'], krn.make_kernel_func('ard', EPS), c['Xs'], 64, max_batch=4)
    try:
        prob2, _, _, ess2, _ = p(theta, us=us)
        # the averages over the states follow LaplacePredictor's, from prob alone
        ylab = np.where(np.arange(70) % 2 == 0, 1.0, -1.0)
        avg = p.posterior_average(theta, us=us, burn=1)
        lpd = p.log_predictive_density(theta, ylab, us=us)
        np.testing.assert_array_equal(avg, prob2[1:].mean(0))
        pl = np.where(ylab[None] > 0, prob2, 1.0 - prob2)
        assert lpd == pytest.approx(np.mean(np.log(pl.mean(0))), abs=1e-12)
        # device draws by seed: the same call twice gives the same bits
        a = p(theta[:2], seeds=[7, 8])
        b = p(theta[:2], seeds=[7, 8])
        np.testing.assert_array_equal(a[0], b[0])
        assert np.isfinite(a[0]).all() and np.all((a[3] >= 1.0) & (a[3] <= 64.0))
    finally:
        p.close()
    print('sampler predict vs ISPredictor: d prob {0:.2e} d ess {1:.2e}'.format(
        np.abs(prob - prob2).max(), np.abs(ess / ess2 - 1).max()))
    assert np.abs(prob - prob2).max() <= PROB_TOL
    assert np.abs(ess / ess2 - 1).max() <= PROB_TOL
    other = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 2, 8, prior, prop_scales=0.1, seed=1,
                                         estimator='priormc')
    try:
        with pytest.raises(ValueError):
            other.predict(c['Xs'])
    finally:
        other.ctx.close()
