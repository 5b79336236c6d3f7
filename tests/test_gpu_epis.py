"""The IS estimator with the EP importance distribution on the device (APM_EST_IS_EP; ep.hip
k_ep_handoff, host_theta.cpp) against the numpy restatement
(tests/epis_restatement.py), plus what needs no restatement: batch neutrality, that such a call
leaves every other path's results alone, failure mapping, the Python estimator, the batched
samplers and the spread of the estimate against the Laplace proposal's."""
import math

import numpy as np
import pytest

import ep_restatement as ep
import epis_restatement as eis
from cov_restatement import Cov
from test_gpu_ep import _other_paths, assert_stop_margin, kind_code, oracle_K
from test_gpu_predict import SHAPES, _make_case

pytestmark = pytest.mark.gpu

EPS = 1e-8
N_IMP = 64
IS_TOL = 5e-4      # |delta log f| of an IS theta- or u-call, nats, absolute
FIT_TOL = 1e-9     # the fp64 fit against the restatement, relative
GUARD = (1.0, 1e-6, 5e-2, 1e-4)  # the guard's bounds r1 .. r4
EDGE_N = (65, 512, 513, 577)


def _draws(n, seed):
    """N(0, 1) draws that fp32 holds exactly (the device keeps U in both precisions)."""
    u = np.random.RandomState(seed).normal(size=(n, N_IMP))
    return u.astype(np.float32).astype(np.float64)


def _with_refs(c, grams, seed):
    """The restatement's state and its theta- / u-call values per theta, on the case."""
    c['ns'], c['ns2'] = _draws(c['n'], seed + 1), _draws(c['n'], seed + 2)
    c['K'] = grams
    c['st'] = [eis.state(K, c['y']) for K in grams]
    c['ref_theta'] = [eis.is_consistent(c['y'], st, c['ns']) for st in c['st']]
    c['ref_u'] = [eis.is_consistent(c['y'], st, c['ns2']) for st in c['st']]
    return c


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


@pytest.fixture(scope='module')
def cases():
    """Data and restatement values per shape of test_gpu_predict (test_gpu_ep's seeds), computed
    once and left unchanged."""
    out = []
    for i, (n, d, m, kind) in enumerate(SHAPES):
        c = _make_case(n, d, m, kind, 100 + i)
        out.append(_with_refs(c, [oracle_K(c, th) for th in c['thetas']], 100 + i))
    return out


def _calls(nat, c, kind, thetas, max_batch=None):
    """One EST_IS_EP theta-call at `thetas` (draws ns), the guard residuals, the u-call on its
    slots (draws ns2) and the slots' read-back."""
    T = len(thetas)
    ctx = nat.Context(c['X'], c['y'], kind, EPS, N_IMP, max_batch=max_batch or T, n_slots=T,
                      n_ubufs=2)
    try:
        ctx.u_upload(0, c['ns'])
        ctx.u_upload(1, c['ns2'])
        r = dict(theta=ctx.theta_eval(nat.EST_IS_EP, thetas, [0] * T, list(range(T))))
        r['guard'] = ctx.guard_read(T)
        r['u'] = ctx.u_eval(list(range(T)), [1] * T)
        r['slots'] = [ctx.slot_read(s) for s in range(T)]
    finally:
        ctx.close()
    return r


def _assert_parity(c, r, idx, label):
    """The assertions of the parity test for thetas `idx` of case c; returns the worst |d log f|."""
    out, st, nops = r['theta']
    worst = 0.0
    for q, t in enumerate(idx):
        ref = c['st'][t]
        assert_stop_margin(ref)
        assert st[q] == 0 and r['u'][1][q] == 0
        assert int(nops[q]) == 2 * ref['n_sweeps'] + 3
        d_theta, d_u = abs(out[q] - c['ref_theta'][t]), abs(r['u'][0][q] - c['ref_u'][t])
        _, f, _, cst = r['slots'][q]
        e_f = np.abs(f - ref['mu']).max() / np.abs(ref['mu']).max()
        e_c = abs(cst - eis.cst(ref)) / max(1.0, abs(eis.cst(ref)))
        print('{0} theta_0 {1}: sweeps {2} d theta-call {3:.2e} u-call {4:.2e} f_post {5:.2e} '
              'cst {6:.2e} guard {7}'.format(label, c['thetas'][t][0], ref['n_sweeps'], d_theta,
                                             d_u, e_f, e_c, r['guard'][q]))
        assert d_theta <= IS_TOL and d_u <= IS_TOL
        assert e_f <= FIT_TOL and e_c <= FIT_TOL
        assert all(r['guard'][q][k] <= GUARD[k] for k in range(4))
        worst = max(worst, d_theta, d_u)
    return worst


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_theta_and_u_call_vs_restatement(nat, cases, ci):
    c = cases[ci]
    r = _calls(nat, c, kind_code(nat, c['kind']), c['thetas'])
    worst = _assert_parity(c, r, range(3), 'shape {0}'.format(SHAPES[ci]))
    print('EP-IS parity shape {0}: worst {1:.3e} nats (tol {2:.0e})'.format(SHAPES[ci], worst,
                                                                            IS_TOL))


@pytest.mark.parametrize('n', EDGE_N)
def test_panel_edges(nat, n):
    """d = 4, ARD, theta_0 = 0.3 at the tile and outer-panel boundaries (nb = 2, 8, 9, 10)."""
    c = _make_case(n, 4, 3, 'ard', 300 + n)
    _with_refs(c, [oracle_K(c, c['thetas'][0])], 300 + n)
    r = _calls(nat, c, nat.KERNEL_ARD, c['thetas'][:1])
    _assert_parity(c, r, [0], 'N = {0}'.format(n))


def test_panel_edge_matern52(nat):
    c = _make_case(513, 4, 3, 'ard', 300 + 513)
    _with_refs(c, [Cov('52', 'ard').gram(c['X'], c['thetas'][0], EPS)], 300 + 513)
    r = _calls(nat, c, nat.KERNEL_M52_ARD, c['thetas'][:1])
    _assert_parity(c, r, [0], 'Matern 5/2 N = 513')


def test_theta_eval_K(nat, cases):
    """apm_theta_eval_K with the oracle's K at (130, 5): the apm_theta_eval value of the same
    theta, and the restatement's."""
    c = cases[0]
    dev = _calls(nat, c, nat.KERNEL_ARD, c['thetas'][:1])['theta'][0][0]
    ctx = nat.Context(None, c['y'], nat.KERNEL_PRECOMPUTED, EPS, N_IMP, max_batch=1, n_slots=1,
                      n_ubufs=2)
    try:
        ctx.u_upload(0, c['ns'])
        ctx.u_upload(1, c['ns2'])
        out, st, nops = ctx.theta_eval_K(nat.EST_IS_EP, c['K'][0], 0, 0)
        u, ust = ctx.u_eval([0], [1])
    finally:
        ctx.close()
    assert st[0] == 0 and ust[0] == 0 and int(nops[0]) == 2 * c['st'][0]['n_sweeps'] + 3
    print('theta_eval_K {0:.8f} theta_eval {1:.8f} restatement {2:.8f}'.format(
        out[0], dev, c['ref_theta'][0]))
    assert abs(out[0] - dev) <= IS_TOL
    assert abs(out[0] - c['ref_theta'][0]) <= IS_TOL and abs(dev - c['ref_theta'][0]) <= IS_TOL
    assert abs(u[0] - c['ref_u'][0]) <= IS_TOL


def test_follow_ups_after_the_read_back(nat, cases, monkeypatch):
    """What follows an APM_EST_IS theta-call's first read-back follows this one too, forced at
    (130, 5) by the library's knobs: the fp64 rerun of the fp32 bottom block
    (APM_POST32_Q=0), wide slots with their fp64 factor (APM_WIDE_Q=0) and the reference-route
    check of chol(C) from the EP's S^1/2 (APM_ICM_Q=1: the two chains it can reach at this size).
    Each keeps status 0 and the restatement's value; the fit's f_post and cst keep their bits, and
    the check, which writes nothing the estimate reads, keeps every bit."""
    c = cases[0]
    ref = _calls(nat, c, nat.KERNEL_ARD, c['thetas'])
    for knob, value, kind in (('APM_POST32_Q', '0', nat.PROF_POST64_RERUNS),
                              ('APM_WIDE_Q', '0', nat.PROF_POST64_RERUNS),
                              ('APM_ICM_Q', '1', nat.PROF_ICM_CHECKS)):
        monkeypatch.setenv(knob, value)
        ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, N_IMP, max_batch=3, n_slots=3,
                          n_ubufs=2)
        monkeypatch.delenv(knob)
        try:
            ctx.u_upload(0, c['ns'])
            ctx.u_upload(1, c['ns2'])
            pad = ctx.padded_n
            ctx.prof_read(kind, reset=True)
            out, st, nops = ctx.theta_eval(nat.EST_IS_EP, c['thetas'], [0] * 3, [0, 1, 2])
            count = ctx.prof_read(kind, reset=True)[1]
            u, ust = ctx.u_eval([0, 1, 2], [1] * 3)
            slots = [ctx.slot_read(s) for s in range(3)]
        finally:
            ctx.close()
        print('{0}={1}: count {2}, d theta-call {3}, d u-call {4}'.format(
            knob, value, count, np.abs(out - c['ref_theta']), np.abs(u - c['ref_u'])))
        # the check takes a chain whose trace(C), padded rows' unit diagonal included, is below
        # n K_ii / APM_ICM_Q: at APM_ICM_Q=1 every chain but the one at theta_0 = -1, where the
        # 62 padded rows alone exceed n K_ii = 48; the other knobs take every chain
        want = 3
        if knob == 'APM_ICM_Q':
            tr = [np.sum(t['C_chol'] ** 2) + pad - c['n'] for t in c['st']]
            thr = [c['n'] * (math.exp(th[0]) + EPS) for th in c['thetas']]
            print('trace(C) + padding', tr, 'thresholds', thr)
            assert all(abs(a - b) > 0.05 * b for a, b in zip(tr, thr))
            want = sum(a < b for a, b in zip(tr, thr))
            assert want == 2
        assert not st.any() and not ust.any() and count == want
        assert np.array_equal(nops, ref['theta'][2])
        assert np.abs(out - c['ref_theta']).max() <= IS_TOL
        assert np.abs(u - c['ref_u']).max() <= IS_TOL
        for t in range(3):
            assert np.array_equal(slots[t][1], ref['slots'][t][1])
            assert slots[t][3] == ref['slots'][t][3]
        if knob == 'APM_ICM_Q':
            assert np.array_equal(out, ref['theta'][0]) and np.array_equal(u, ref['u'][0])


def test_batch_neutrality(nat, cases):
    """Three thetas with different sweep counts in one call (max_batch = 4), then one by one:
    every output bitwise equal."""
    c = cases[0]
    assert len(set(st['n_sweeps'] for st in c['st'])) == 3
    full = _calls(nat, c, nat.KERNEL_ARD, c['thetas'], max_batch=4)
    assert not full['theta'][1].any() and len(set(full['theta'][2].tolist())) == 3
    for t in range(3):
        one = _calls(nat, c, nat.KERNEL_ARD, c['thetas'][t:t + 1], max_batch=4)
        for key in ('theta', 'u'):
            for a, b in zip(full[key], one[key]):
                assert a[t] == b[0], (key, t)
        assert np.array_equal(full['guard'][t], one['guard'][0])
        for a, b in zip(full['slots'][t], one['slots'][0]):
            assert np.array_equal(a, b)


def test_epis_leaves_the_other_paths_alone(nat):
    """N = 577: the Laplace theta-call, predict, laplace_grad, an IS theta-call with its u-call
    and slot read-back, and ep, before and after an EST_IS_EP theta-call on the same context, and
    on a fresh context: all bitwise the same."""
    c = _make_case(577, 4, 3, 'ard', 300 + 577)

    def make():
        return nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=2, n_slots=2,
                           n_ubufs=2)

    def paths(ctx):
        return _other_paths(nat, ctx, c) + list(ctx.ep(c['thetas'][:2]))
    ctx = make()
    before = paths(ctx)
    assert not np.any(before[1]) and not np.any(before[13])  # (Laplace and IS statuses)
    out, st, _ = ctx.theta_eval(nat.EST_IS_EP, c['thetas'][:2], [0, 1], [0, 1])
    assert not st.any() and np.isfinite(out).all()
    after = paths(ctx)
    ctx.close()
    ctx = make()
    fresh = paths(ctx)
    ctx.close()
    assert len(before) == len(after) == len(fresh)
    for i, (a, b, f) in enumerate(zip(before, after, fresh)):
        assert np.array_equal(a, b, equal_nan=True), i
        assert np.array_equal(a, f, equal_nan=True), i


def test_failure_mapping(nat, cases):
    c = cases[0]
    easy = c['thetas'][0].copy()
    easy[0] = -16.0  # (test_gpu_ep: converges in the second sweep)
    assert ep.ep_fit(oracle_K(c, easy), c['y'])['n_sweeps'] == 2
    thetas = np.array([easy, c['thetas'][0]])
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, N_IMP, max_batch=2, n_slots=2,
                      n_ubufs=1)
    ctx.u_upload(0, c['ns'])
    ctx.set_ep(0.8, 1e-8, 2)
    out, st, nops = ctx.theta_eval(nat.EST_IS_EP, thetas, [0, 0], [0, 1])
    assert list(st) == [nat.STATUS_OK, nat.STATUS_MAXITER] and list(nops) == [7, 7]
    alone = ctx.theta_eval(nat.EST_IS_EP, thetas[:1], [0], [1])
    assert alone[1][0] == 0 and alone[0][0] == out[0] and np.isfinite(out[0])
    ctx.set_ep()  # the defaults
    good = ctx.theta_eval(nat.EST_IS_EP, thetas, [0, 0], [0, 1])
    assert list(good[1]) == [0, 0] and good[0][0] == out[0]
    with pytest.raises(nat.NativeError):  # no estimator 4
        ctx.theta_eval(4, thetas, [0, 0], [0, 1])
    ctx.close()
    lg = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, N_IMP, max_batch=2, n_slots=2,
                     n_ubufs=1, likelihood='logit')
    o = np.zeros(2)
    s2 = np.zeros(2, dtype=np.int32)
    idx = np.zeros(2, dtype=np.int64)
    th = np.ascontiguousarray(thetas)
    assert lg.lib.apm_theta_eval(lg._h, nat.EST_IS_EP, 2, th.ctypes.data, th.shape[1],
                                 idx.ctypes.data, idx.ctypes.data, o.ctypes.data,
                                 s2.ctypes.data, None) == nat.APM_E_INVALID
    K = np.ascontiguousarray(c['K'][0])
    assert lg.lib.apm_theta_eval_K(lg._h, nat.EST_IS_EP, K.ctypes.data, K.shape[1], 0, 0,
                                   o.ctypes.data, s2.ctypes.data, None) == nat.APM_E_INVALID
    lg.close()


def test_python_estimator(nat, cases):
    import gpdemo.estimators as est
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    c = cases[0]
    th = c['thetas'][0]
    r = _calls(nat, c, nat.KERNEL_ARD, c['thetas'][:1])
    kf = krn.make_kernel_func('ard', EPS)
    e = est.LogMarginalLikelihoodApproxPosteriorISEstimator(c['X'], c['y'], kf,
                                                            lpa.ep_approximation)
    v, cache = e(c['ns'], th)
    assert isinstance(cache, est.DeviceCache) and cache.kind == nat.EST_IS_EP
    assert v == r['theta'][0][0]
    assert e.n_cubic_ops == 2 * c['st'][0]['n_sweeps'] + 3
    v2, cache2 = e(c['ns2'], cached_results=cache)
    assert cache2 is cache and v2 == r['u'][0][0]
    assert e.n_cubic_ops == 2 * c['st'][0]['n_sweeps'] + 3
    mu = c['st'][0]['mu']
    assert np.abs(cache.read()[1] - mu).max() <= FIT_TOL * np.abs(mu).max()
    with pytest.raises(NotImplementedError):
        est.LogMarginalLikelihoodApproxPosteriorISEstimator(c['X'], c['y'], kf,
                                                            lpa.ep_approximation,
                                                            likelihood='logit')
    e2 = est.LogMarginalLikelihoodApproxPosteriorISEstimator(c['X'], c['y'], kf,
                                                             lpa.ep_approximation, max_sweeps=2)
    with pytest.raises(lpa.MaximumIterationsExceededError):
        e2(c['ns'], th)
    # the Laplace proposal's estimator is the one it was
    e3 = est.LogMarginalLikelihoodApproxPosteriorISEstimator(c['X'], c['y'], kf,
                                                             lpa.laplace_approximation)
    assert e3(c['ns'], th)[1].kind == nat.EST_IS


def test_batched_samplers_run_is_ep_and_are_batch_invariant(nat):
    """estimator='is_ep' through E-SS + MH and PM-MH: n = 65, 4 chains x 5 samples, finite log_f,
    and chain 0's trajectory bitwise the one it has alone."""
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler, BatchedPMMHSampler
    c = _make_case(65, 4, 3, 'ard', 300 + 65)
    prior = dict(a_tau=1., b_tau=1. / c['d'] ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(c['d'], 0.5 * math.log(c['d']))], (4, 1))
    for cls, kw in ((BatchedAPMEllSSPlusMHSampler, {}), (BatchedPMMHSampler, dict(kernel='ard'))):
        kw = dict(kw, prop_scales=0.1, seed=71, estimator='is_ep',
                  ep_settings=dict(damping=0.8, diff_tol=1e-8, max_sweeps=100))
        smp = cls(c['X'], c['y'], 4, 16, prior, **kw)
        assert smp.est == nat.EST_IS_EP
        th, nrej = smp.get_samples(5, th0)
        assert np.isfinite(th).all() and not smp.failed.any() and np.isfinite(smp.log_f).all()
        assert (smp.n_cubic_ops >= 2 * 2 + 3).all()
        one = cls(c['X'], c['y'], 1, 16, prior, **kw)
        th1, nrej1 = one.get_samples(5, th0[:1])
        assert np.array_equal(th1[0], th[0]) and nrej1[0] == nrej[0]
        assert one.log_f[0] == smp.log_f[0]
    # a chain whose fit fails is masked like any failed chain
    bad = BatchedPMMHSampler(c['X'], c['y'], 2, 16, prior, prop_scales=0.1, seed=71, kernel='ard',
                             estimator='is_ep', ep_settings=dict(max_sweeps=2))
    bad.initialise(th0[:2])
    assert bad.failed.all() and (bad.fail_status == nat.STATUS_MAXITER).all()
    pm = BatchedPMMHSampler(c['X'], c['y'], 2, 16, prior, prop_scales=0.1, seed=71, kernel='ard')
    pm.set_estimator('is_ep')
    assert pm.est == nat.EST_IS_EP


def test_spread_on_the_device(nat, cases):
    """(130, 5), theta_0 = 3: the standard deviation of the estimate over 32 draw matrices through
    u-calls on one slot of each kind. The restatement's ratio is about 0.2; only "smaller" is
    asserted."""
    c = cases[0]
    th = c['thetas'][1:2]
    assert th[0][0] == 3.0
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, N_IMP, max_batch=2, n_slots=2,
                      n_ubufs=1)
    try:
        ctx.u_upload(0, c['ns'])
        assert ctx.theta_eval(nat.EST_IS, th, [0], [0])[1][0] == 0
        assert ctx.theta_eval(nat.EST_IS_EP, th, [0], [1])[1][0] == 0
        vals = []
        for k in range(32):
            ctx.u_upload(0, _draws(c['n'], 5000 + k))
            out, st = ctx.u_eval([0, 1], [0, 0])
            assert not st.any()
            vals.append(out)
    finally:
        ctx.close()
    sd = np.array(vals).std(0)
    print('device spread at theta_0 = 3: sd EST_IS {0:.4f} EST_IS_EP {1:.4f} ratio {2:.3f}'.format(
        sd[0], sd[1], sd[1] / sd[0]))
    assert sd[1] < sd[0]
