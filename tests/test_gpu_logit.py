"""The logistic likelihood on the device (apm_set_likelihood / apm_laplace_lik)
against the float64 restatement of tests/logit_restatement.py - importance sampling and PriorMC
theta- and u-calls, the Laplace estimator, apm_laplace_lik, the predictive and the gradient - plus
what needs no restatement: exact values at an uninformed test point, batch neutrality, the cubic-op
accounting, a probit context that a logit one in the same process leaves bitwise alone, and a
batched sampler run."""
import math

import numpy as np
import pytest

import edge_cases as ec
import grad_restatement as gr
import logit_restatement as lr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = 1e-8
N_IMP = 64
# The project's stated tolerances, not new ones:
IS_TOL = 5e-4                 # |delta log f| of an IS / PriorMC theta- or u-call, nats, absolute
FP64_TOL = 1e-9               # Laplace f and LML, predictive mean / var, lml / grad: relative
PROB_TOL = 1e-9 + lr.GH_BOUND  # predictive prob, absolute: the yardstick + the quadrature bound
GRAD_NEWTON_TOL = 1e-14       # test_gpu_grad's
# (n, d, m, kind, Matern family, seed). The smallest sizes that reach each path: nb = 2; a ragged
# last panel of nb = 3; the iso kind; np = 576 - a second outer panel, the inverse-panel route of
# the mixed Newton and the rank-256 update of the test rows - with SE and with Matern 5/2. Three
# thetas each, theta_0 = 0.3, 3.0, -1.0. The seeds are the first from 7065, 7130, 7200, 7513 and
# 8513 upwards at which the restatement's Newton run keeps the margins of DESIGN.md §13 at every
# theta (edge_cases.margins_hold: a factor 3 around 1e-4, a factor 100 around 1e-14;
# test_newton_margins), so device and restatement cannot disagree on an iteration count.
SHAPES = [(65, 4, 70, 'ard', None, 7081), (130, 5, 70, 'ard', None, 7141),
          (200, 3, 65, 'iso', None, 7210), (513, 4, 70, 'ard', None, 7519),
          (513, 4, 70, 'ard', '52', 8698)]
I_130, I_513 = 1, 3
I_FAR = 3  # the last test row is far from this training row


def _cov(c):
    return Cov(c['family'] or 'se', c['kind'])


def _gram(c, theta, X=None):
    return _cov(c).gram(c['X'] if X is None else X, theta, EPS)


def _gram_cross(c, theta):
    if c['family'] is not None:
        return _cov(c).gram_cross(c['Xs'], c['X'], theta)
    n = c['n']
    return _gram(c, theta, np.concatenate([c['X'], c['Xs']]))[n:, :n].copy()


def _dK(c, theta, K):
    return _cov(c).dK(c['X'], theta, EPS, K=K)


def _draws(n, seed):
    """N(0, 1) draws that fp32 holds exactly (the device keeps U in both precisions)."""
    u = np.random.RandomState(seed).normal(size=(n, N_IMP))
    return u.astype(np.float32).astype(np.float64)


def _make_case(n, d, m, kind, family, seed):
    c = gr.make_case(n, d, kind, seed)
    c['family'], c['m'] = family, m
    Xs = np.random.RandomState(90000 + seed).normal(size=(m, d))
    # far in every coordinate: k* underflows to exactly 0 (the Matern kinds decay exponentially
    # only and need 1000, as test_gpu_matern)
    Xs[-1] = c['X'][I_FAR] + (50.0 if family is None else 1000.0)
    c['Xs'] = Xs
    c['ns'], c['ns2'] = _draws(n, seed + 1), _draws(n, seed + 2)
    return c


@pytest.fixture(scope='module')
def cases():
    """Data and restatement results per shape, computed once and left unchanged."""
    out = []
    for shape in SHAPES:
        c = _make_case(*shape)
        c['ref'] = []
        for th in c['thetas']:
            K = _gram(c, th)
            st = lr.is_state(K, c['y'], 1e-4)
            c['ref'].append(dict(
                K=K, n_iter=st['n_iter'], f=st['f'], lml=st['lml'],
                is_theta=lr.is_consistent(c['y'], st, c['ns']),
                is_u=lr.is_consistent(c['y'], st, c['ns2']),
                mc_theta=lr.priormc(K, c['y'], c['ns']), mc_u=lr.priormc(K, c['y'], c['ns2']),
                pred=lr.predictive(K, _gram_cross(c, th), c['y'], math.exp(th[0]), 1e-4),
                grad=lr.laplace_grad(K, _dK(c, th, K), c['y'], GRAD_NEWTON_TOL)))
        out.append(c)
    return out


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _kind(nat, c):
    if c['family'] == '52':
        return nat.KERNEL_M52_ARD
    return nat.KERNEL_ISO if c['kind'] == 'iso' else nat.KERNEL_ARD


def _context(nat, c, likelihood='logit', max_batch=4):
    return nat.Context(c['X'], c['y'], _kind(nat, c), EPS, N_IMP, max_batch=max_batch,
                       n_slots=2 * max_batch, n_ubufs=2, likelihood=likelihood)


def _run_all(nat, ctx, c, thetas):
    """Every context call of the issue at `thetas` (up to max_batch): IS and PriorMC theta- and
    u-calls (draws ns / ns2 in U buffers 0 / 1), slot read-back, Laplace estimator, predictive at
    the Newton tolerance 1e-4, gradient at 1e-14. The context's Newton settings are left at 1e-4."""
    T = len(thetas)
    ctx.set_newton(1e-4, 1000)
    ctx.u_upload(0, c['ns'])
    ctx.u_upload(1, c['ns2'])
    r = {}
    sl_is, sl_mc = list(range(T)), list(range(T, 2 * T))
    r['is_theta'] = ctx.theta_eval(nat.EST_IS, thetas, [0] * T, sl_is)
    r['is_u'] = ctx.u_eval(sl_is, [1] * T)
    r['slots'] = [ctx.slot_read(s) for s in sl_is]
    r['mc_theta'] = ctx.theta_eval(nat.EST_PRIORMC, thetas, [0] * T, sl_mc)
    r['mc_u'] = ctx.u_eval(sl_mc, [1] * T)
    r['laplace'] = ctx.theta_eval(nat.EST_LAPLACE, thetas)
    r['pred'] = ctx.predict(thetas, c['Xs'])
    ctx.set_newton(GRAD_NEWTON_TOL, 1000)
    r['grad'] = ctx.laplace_grad(thetas)
    ctx.set_newton(1e-4, 1000)
    return r


def _flat(r):
    """Every array and scalar of _run_all's result, in a fixed order."""
    out = []
    for key in ('is_theta', 'is_u', 'mc_theta', 'mc_u', 'laplace', 'pred', 'grad'):
        out.extend(np.asarray(a) for a in r[key])
    for s in r['slots']:
        out.extend(np.asarray(a) for a in s)
    return out


def _assert_bitwise(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb)
    for x, y in zip(fa, fb):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


@pytest.fixture(scope='module')
def device(nat, cases):
    """Device results per shape: one logit context each, three thetas per call."""
    out = []
    for c in cases:
        ctx = _context(nat, c)
        assert ctx.lib.apm_likelihood(ctx._h) == nat.LIK_LOGIT
        out.append(_run_all(nat, ctx, c, c['thetas']))
        ctx.close()
    return out


def test_newton_margins(cases):
    """The condition the seeds were chosen by, on the logit's own Newton runs."""
    for c in cases:
        for ref in c['ref']:
            diffs = ref['grad']['diffs']
            assert ec.margins_hold(diffs)
            assert ec.fit_iterations(diffs) == ref['n_iter'] == ref['pred']['n_iter']


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_estimators_vs_restatement(cases, device, ci):
    """IS and PriorMC theta- and u-calls to 5e-4 nats, the Laplace estimator's LML to 1e-9
    relative, equal Newton iteration counts, and the reference's cubic-op accounting (the
    probit's: IS n_iter + 1 + 2, PriorMC 1, Laplace n_iter)."""
    c, dev = cases[ci], device[ci]
    worst_is, worst_lml = 0.0, 0.0
    for t, ref in enumerate(c['ref']):
        for key in ('is_theta', 'is_u', 'mc_theta', 'mc_u'):
            assert dev[key][1][t] == 0
            err = abs(dev[key][0][t] - ref[key])
            worst_is = max(worst_is, err)
            print('logit {0} shape {1} theta {2}: device {3:.6f} restatement {4:.6f} ({5:.2e})'
                  .format(key, SHAPES[ci][:5], t, dev[key][0][t], ref[key], err))
        assert dev['laplace'][1][t] == 0
        err = abs(dev['laplace'][0][t] - ref['lml']) / max(1.0, abs(ref['lml']))
        worst_lml = max(worst_lml, err)
        assert int(dev['is_theta'][2][t]) == ref['n_iter'] + 1 + 2
        assert int(dev['mc_theta'][2][t]) == 1
        assert int(dev['laplace'][2][t]) == ref['n_iter']
        f_dev = dev['slots'][t][1]
        ferr = np.abs(f_dev - ref['f']).max() / np.abs(ref['f']).max()
        print('logit f_post shape {0} theta {1}: {2:.2e} of max|f|'.format(SHAPES[ci][:5], t, ferr))
        assert ferr <= 1e-8  # (§3.3: f_post within 1e-8 of its maximum, the mixed Newton's)
    print('logit estimators shape {0}: worst IS / PriorMC {1:.2e} nats (tol {2:.0e}), LML {3:.2e} '
          '(tol {4:.0e})'.format(SHAPES[ci][:5], worst_is, IS_TOL, worst_lml, FP64_TOL))
    assert worst_is <= IS_TOL
    assert worst_lml <= FP64_TOL


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_laplace_lik_vs_restatement(nat, cases, ci):
    """apm_laplace_lik (gpdemo's laplace_approximation(likelihood='logit')) on the restatement's
    K: f and the LML to 1e-9 relative, the covariance to 1e-9 of its largest entry, equal
    iteration counts; apm_laplace on the same K stays the probit."""
    import gpdemo.latent_posterior_approximations as lpa
    c = cases[ci]
    for t, ref in enumerate(c['ref'][:1 if c['n'] > 500 else 3]):
        f, C, lml, n_ops = lpa.laplace_approximation(ref['K'], c['y'], calc_cov=True,
                                                     calc_lml=True, likelihood='logit')
        assert n_ops == ref['n_iter'] + 1
        nw = lr.newton(ref['K'], c['y'], 1e-4)
        Cref = lr.covariance(ref['K'], nw)
        errs = (np.abs(f - ref['f']).max() / np.abs(ref['f']).max(),
                abs(lml - ref['lml']) / max(1.0, abs(ref['lml'])),
                np.abs(C - Cref).max() / np.abs(Cref).max())
        print('apm_laplace_lik shape {0} theta {1}: f {2:.2e} lml {3:.2e} C {4:.2e}'
              .format(SHAPES[ci][:5], t, *errs))
        np.testing.assert_allclose(f, ref['f'], rtol=FP64_TOL,
                                   atol=FP64_TOL * np.abs(ref['f']).max())
        assert errs[1] <= FP64_TOL and errs[2] <= FP64_TOL
        fp, lmlp, _ = lpa.laplace_approximation(ref['K'], c['y'], calc_cov=False, calc_lml=True)
        assert abs(lmlp - lml) > 1e-3
        # apm_laplace_lik(APM_LIK_PROBIT) is apm_laplace, bit for bit
        n = c['n']
        K, y = np.ascontiguousarray(ref['K']), np.ascontiguousarray(c['y'])
        f2, l2 = np.empty(n), np.zeros(1)
        it2, st2 = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)
        assert nat.load_library().apm_laplace_lik(
            nat.default_device(), nat.LIK_PROBIT, K.ctypes.data, n, n, y.ctypes.data, 0, 1, 1e-4,
            1000, f2.ctypes.data, None, n, l2.ctypes.data, it2.ctypes.data, st2.ctypes.data) == 0
        assert st2[0] == 0 and np.array_equal(fp, f2) and lmlp == l2[0]


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_predict_vs_restatement(cases, device, ci):
    c, dev = cases[ci], device[ci]
    mean, var, prob, st, nit = dev['pred']
    worst = {}
    for t, ref in enumerate(c['ref']):
        p = ref['pred']
        assert st[t] == 0 and int(nit[t]) == p['n_iter']
        for key, got in (('mean', mean[t]), ('var', var[t]), ('prob', prob[t])):
            scale = 1.0 if key == 'prob' else max(1.0, np.abs(p[key]).max())
            err = np.abs(got - p[key]).max() / scale
            worst[key] = max(worst.get(key, 0.0), err)
            print('logit predict shape {0} theta {1} {2}: {3:.3e}'
                  .format(SHAPES[ci][:5], t, key, err))
        sigma = math.exp(c['thetas'][t][0])
        # the far row: k* = 0 exactly, so the prior comes back untouched, bit for bit
        assert mean[t, -1] == 0.0 and var[t, -1] == sigma and prob[t, -1] == 0.5
        assert np.all(var[t] > 0.0) and np.all(var[t] <= sigma)
        assert np.all(prob[t] > 0.0) and np.all(prob[t] < 1.0)
    print('logit predict shape {0}: worst {1}'.format(SHAPES[ci][:5], worst))
    assert worst['mean'] <= FP64_TOL and worst['var'] <= FP64_TOL
    assert worst['prob'] <= PROB_TOL


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_grad_vs_restatement(cases, device, ci):
    """lml and grad to test_gpu_grad's tolerance: 1e-9 x max(1, max|ref grad|)."""
    c, dev = cases[ci], device[ci]
    lml, grad, st, nit = dev['grad']
    worst = 0.0
    for t, ref in enumerate(c['ref']):
        g = ref['grad']
        assert st[t] == 0 and int(nit[t]) == g['n_iter']
        scale = max(1.0, np.abs(g['grad']).max())
        err = max(abs(lml[t] - g['lml']), np.abs(grad[t] - g['grad']).max()) / scale
        worst = max(worst, err)
        print('logit grad shape {0} theta {1}: {2:.3e} (max|grad| {3:.3e})'
              .format(SHAPES[ci][:5], t, err, np.abs(g['grad']).max()))
    print('logit grad shape {0}: worst {1:.3e} (tol {2:.0e})'.format(SHAPES[ci][:5], worst,
                                                                    FP64_TOL))
    assert worst <= FP64_TOL


@pytest.mark.parametrize('ci', [I_130, I_513])
def test_batch_position_is_bitwise_neutral(nat, cases, device, ci):
    """A chain's logit outputs - IS theta-call and u-call, slot, predictive, gradient - alone
    (count 1) and as the last of 4 with other thetas in front: the same bits, which are also the
    bits of the three-theta call of the `device` fixture."""
    c = cases[ci]
    rng = np.random.RandomState(17)
    other = c['thetas'][[1, 2, 0]] + rng.uniform(-0.2, 0.2, size=c['thetas'].shape)
    ctx = _context(nat, c)
    for t, th in enumerate(c['thetas']):
        alone = _run_all(nat, ctx, c, th[None])
        four = _run_all(nat, ctx, c, np.vstack([other, th[None]]))
        for key in ('is_theta', 'is_u', 'mc_theta', 'mc_u', 'laplace', 'pred', 'grad'):
            for a, b, d in zip(alone[key], four[key], device[ci][key]):
                assert np.array_equal(np.asarray(a)[0], np.asarray(b)[3]), (key, t)
                assert np.array_equal(np.asarray(a)[0], np.asarray(d)[t]), (key, t)
        for a, b in zip(alone['slots'][0], four['slots'][3]):
            assert np.array_equal(a, b)
    ctx.close()


def test_probit_is_untouched_by_a_logit_context(nat, cases, device):
    """In one process: a probit context at n = 130 and n = 513 (IS theta-call, u-call, slot_read,
    PriorMC, Laplace, predict, grad), then a logit context created and used, then the probit calls
    again on the old context and on a fresh one: every value, status and slot array bitwise
    equal. The logit values at the same thetas differ from the probit's by more than 1e-3 nats:
    the switch does something."""
    for ci in (I_130, I_513):
        c = cases[ci]
        old = _context(nat, c, 'probit')
        assert old.lib.apm_likelihood(old._h) == nat.LIK_PROBIT
        before = _run_all(nat, old, c, c['thetas'])
        logit = _context(nat, c, 'logit')
        lg = _run_all(nat, logit, c, c['thetas'])
        _assert_bitwise(lg, device[ci])  # (and the logit context is itself reproducible)
        again = _run_all(nat, old, c, c['thetas'])
        fresh_ctx = _context(nat, c, 'probit')
        fresh = _run_all(nat, fresh_ctx, c, c['thetas'])
        _assert_bitwise(before, again)
        _assert_bitwise(before, fresh)
        # a context created without the keyword is the probit
        default = nat.Context(c['X'], c['y'], _kind(nat, c), EPS, N_IMP, max_batch=4, n_slots=8,
                              n_ubufs=2)
        _assert_bitwise(before, _run_all(nat, default, c, c['thetas']))
        for key in ('is_theta', 'is_u', 'mc_theta', 'laplace', 'grad'):
            gap = np.abs(np.asarray(lg[key][0]) - np.asarray(before[key][0]))
            print('probit vs logit {0} n = {1}: differ by {2}'.format(key, c['n'], gap))
            assert np.all(gap > 1e-3)
        assert np.abs(lg['pred'][2] - before['pred'][2]).max() > 1e-3
        # the C entry point: switching an existing context there and back
        assert old.lib.apm_set_likelihood(old._h, 7) == nat.APM_E_INVALID
        assert old.lib.apm_likelihood(old._h) == nat.LIK_PROBIT
        assert old.lib.apm_set_likelihood(old._h, nat.LIK_LOGIT) == 0
        _assert_bitwise(lg, _run_all(nat, old, c, c['thetas']))
        assert old.lib.apm_set_likelihood(old._h, nat.LIK_PROBIT) == 0
        _assert_bitwise(before, _run_all(nat, old, c, c['thetas']))
        for ctx in (old, logit, fresh_ctx, default):
            ctx.close()


def test_python_classes_carry_the_likelihood(nat, cases, device):
    """The estimator classes, LaplacePredictor and LaplaceGradient with likelihood='logit' return
    the context-level values of the `device` fixture (same library calls, count 1)."""
    import gpdemo.estimators as est
    import gpdemo.gradients as gd
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    import gpdemo.predict as prd
    c, dev = cases[I_130], device[I_130]
    kf = krn.make_kernel_func('ard', EPS)
    th = c['thetas'][0]
    e = est.LogMarginalLikelihoodApproxPosteriorISEstimator(
        c['X'], c['y'], kf, lpa.laplace_approximation, likelihood='logit')
    v, cache = e(c['ns'], th)
    v2, _ = e(c['ns2'], cached_results=cache)
    assert v == dev['is_theta'][0][0] and v2 == dev['is_u'][0][0]
    assert e.n_cubic_ops == dev['is_theta'][2][0]
    m = est.LogMarginalLikelihoodPriorMCEstimator(c['X'], c['y'], kf, likelihood='logit')
    assert m(c['ns'], th)[0] == dev['mc_theta'][0][0]
    la = est.LogMarginalLikelihoodLaplaceEstimator(c['X'], c['y'], kf, likelihood='logit')
    assert la(th) == dev['laplace'][0][0]
    p = prd.LaplacePredictor(c['X'], c['y'], kf, c['Xs'], likelihood='logit')
    mean, var, prob = p(c['thetas'])
    assert np.array_equal(prob, dev['pred'][2]) and np.array_equal(mean, dev['pred'][0])
    ys = np.where(np.arange(c['m']) % 2 == 0, 1.0, -1.0)
    lp = np.where(ys[None] > 0, np.log(prob), np.log1p(-prob))
    want = float(np.mean(lp.max(0) + np.log(np.mean(np.exp(lp - lp.max(0)[None]), axis=0))))
    assert p.log_predictive_density(c['thetas'], ys) == want
    p.close()
    g = gd.LaplaceGradient(c['X'], c['y'], kf, likelihood='logit')
    lml, grad = g(c['thetas'])
    assert np.array_equal(lml, dev['grad'][0]) and np.array_equal(grad, dev['grad'][1])
    g.close()


def test_batched_sampler_runs_the_logit_and_is_batch_invariant(nat, cases):
    """likelihood='logit' through E-SS + MH: 4 chains x 5 iterations at n = 130; every chain's
    trajectory and rejection count bitwise equal to the same chain run alone (four batches of 1),
    and not the probit sampler's."""
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler
    c = cases[I_130]
    prior = dict(a_tau=1., b_tau=1. / c['d'] ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(c['d'], 0.5 * math.log(c['d']))], (4, 1))
    kw = dict(prop_scales=0.1, seed=71)
    smp = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 4, 16, prior, likelihood='logit', **kw)
    assert smp.ctx.likelihood == 'logit'
    th, nrej = smp.get_samples(6, th0)
    assert np.isfinite(th).all() and not smp.failed.any()
    for k in range(4):
        one = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 1, 16, prior, likelihood='logit',
                                           first_chain=k, **kw)
        th1, nrej1 = one.get_samples(6, th0[k:k + 1])
        assert np.array_equal(th1[0], th[k]) and nrej1[0] == nrej[k]
    pro = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 4, 16, prior, **kw)
    pro.initialise(th0)
    lg = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 4, 16, prior, likelihood='logit', **kw)
    lg.initialise(th0)
    assert np.all(np.abs(lg.log_f - pro.log_f) > 1e-3)
