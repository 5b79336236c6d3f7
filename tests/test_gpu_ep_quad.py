"""EP with the tilted moments by quadrature on the device (apm_set_ep_quadrature, apm_ep_lik;
k_ep_sites_q in ep.hip) against the numpy restatement
(tests/ep_quad_restatement.py) on the C oracle's Gram: the logit fit, its predictive, gradient
and IS theta- / u-calls, the probit by quadrature against the probit's closed form, and what
needs no restatement - batch neutrality, that the switch leaves every other path alone, and the
batched samplers. Every parity bound is 1e-9 x max(1, max|ref|), the fp64-against-fp64 yardstick
of DESIGN.md §16, and sweep counts must be equal."""
import math

import numpy as np
import pytest

import ep_grad_restatement as eg
import ep_quad_restatement as eq
import ep_restatement as ep
import grad_restatement as gr
import logit_restatement as lr
import apm_oracle as orc
from cov_restatement import Cov
from test_gpu_ep import KEYS, assert_stop_margin, kind_code, oracle_K, parity
from test_gpu_predict import I_EQ, SHAPES, _make_case

pytestmark = pytest.mark.gpu

EPS = 1e-8
TOL = 1e-9
DIFF_TOL = 1e-8
IS_TOL = 5e-4   # |delta log f| of an IS theta- or u-call, nats, absolute
N_IMP = 64
FIT_SHAPES = (0, 3, 2)  # (130, 5, ard), (64, 33, ard), (200, 3, iso) of test_gpu_predict.SHAPES
EDGE_N = (65, 513, 577)
BOTH_SEED = 102         # (200, 3, iso) at theta_0 = 6: 93 narrow and 107 wide sites at the stop


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _ctx(nat, c, likelihood='logit', max_batch=3, n_imp=1, quadrature=True, **kw):
    kw.setdefault('n_slots', 1)
    kw.setdefault('n_ubufs', 1)
    return nat.Context(c['X'], c['y'], kind_code(nat, c['kind']), EPS, n_imp, max_batch=max_batch,
                       likelihood=likelihood, ep_quadrature=quadrature, **kw)


def assert_restatement_ok(fit, diff_tol=DIFF_TOL):
    """Conditions on the restatement alone: the stop margins of test_gpu_ep and every site of
    every sweep inside the rule's covered region."""
    assert_stop_margin(fit, diff_tol)
    assert fit['covered']


@pytest.fixture(scope='module')
def cases():
    """Data and the restatement's logit fits per shape (test_gpu_ep's recipe and seeds), computed
    once and left unchanged."""
    out = {}
    for ci in FIT_SHAPES:
        n, d, m, kind = SHAPES[ci]
        c = _make_case(n, d, m, kind, 100 + ci)
        c['K'] = [oracle_K(c, th) for th in c['thetas']]
        c['fit'] = [eq.ep_fit(K, c['y'], eq.LOGIT) for K in c['K']]
        out[ci] = c
    return out


@pytest.fixture(scope='module')
def device(nat, cases):
    """apm_ep_eval on a logit context with the switch on: one call, three thetas per shape."""
    out = {}
    for ci, c in cases.items():
        ctx = _ctx(nat, c)
        assert ctx.lib.apm_ep_quadrature(ctx._h) == 1
        out[ci] = ctx.ep(c['thetas'])
        ctx.close()
    return out


@pytest.mark.parametrize('ci', FIT_SHAPES)
def test_logit_fit_vs_restatement(cases, device, ci):
    c, dev = cases[ci], device[ci]
    worst = 0.0
    for t, fit in enumerate(c['fit']):
        assert_restatement_ok(fit)
        assert dev[5][t] == 0
        print('shape {0} theta_0 {1}: sweeps {2}, narrow / wide sites {3} / {4}'.format(
            SHAPES[ci], c['thetas'][t][0], fit['n_sweeps'], fit['n_narrow'], fit['n_wide']))
        assert int(dev[6][t]) == fit['n_sweeps']
        worst = max(worst, parity(dev, t, fit))
    print('logit EP parity shape {0}: worst {1:.3e} (tol {2:.0e})'.format(SHAPES[ci], worst, TOL))
    assert worst <= TOL


@pytest.mark.parametrize('n', EDGE_N)
def test_panel_edges(nat, n):
    """d = 4, ARD, theta_0 = 0.3: the four-rows-per-workgroup tail (N = 65, 513, 577 are 1 mod 4)
    and the padded rows (nb = 2, 9, 10)."""
    c = _make_case(n, 4, 3, 'ard', 300 + n)
    th = c['thetas'][0]
    fit = eq.ep_fit(oracle_K(c, th), c['y'], eq.LOGIT)
    assert_restatement_ok(fit)
    ctx = _ctx(nat, c, max_batch=1)
    dev = ctx.ep(th)
    ctx.close()
    assert dev[5][0] == 0 and int(dev[6][0]) == fit['n_sweeps']
    worst = parity(dev, 0, fit)
    print('logit EP parity N = {0}: worst {1:.3e}'.format(n, worst))
    assert worst <= TOL


def test_both_branches_in_one_fit(nat):
    """(200, 3, iso) at theta_0 = 6: the restatement counts sites on each side of v0 in the final
    sweep (a condition on the inputs; the seed is chosen for it)."""
    c = _make_case(200, 3, 65, 'iso', BOTH_SEED)
    th = c['thetas'][0].copy()
    th[0] = 6.0
    fit = eq.ep_fit(oracle_K(c, th), c['y'], eq.LOGIT)
    assert_restatement_ok(fit)
    print('theta_0 = 6: {0} narrow and {1} wide sites, cavity variances {2:.3g} .. {3:.3g}'.format(
        fit['n_narrow'], fit['n_wide'], fit['var_c'].min(), fit['var_c'].max()))
    assert fit['n_narrow'] >= 1 and fit['n_wide'] >= 1
    ctx = _ctx(nat, c, max_batch=1)
    dev = ctx.ep(th)
    ctx.close()
    assert dev[5][0] == 0 and int(dev[6][0]) == fit['n_sweeps']
    worst = parity(dev, 0, fit)
    print('logit EP parity theta_0 = 6: worst {0:.3e}'.format(worst))
    assert worst <= TOL


def test_probit_by_quadrature_vs_closed_form(nat, cases):
    """(130, 5, ard), the three thetas: the restatement's two probit fits differ by some Delta
    (measured 2.2e-14 of max(1, max|ref|)); the device's pair may differ by Delta + the parity
    bound, with equal sweep counts."""
    c = cases[0]
    ctx = _ctx(nat, c, likelihood='probit', quadrature=False)
    closed = ctx.ep(c['thetas'])
    ctx.set_ep_quadrature(True)
    quad = ctx.ep(c['thetas'])
    ctx.close()
    assert not closed[5].any() and not quad[5].any()
    for t, K in enumerate(c['K']):
        a, b = ep.ep_fit(K, c['y']), eq.ep_fit(K, c['y'], eq.PROBIT)
        assert_restatement_ok(b)
        assert a['n_sweeps'] == b['n_sweeps'] == int(closed[6][t]) == int(quad[6][t])
        for k, key in enumerate(KEYS):
            scale = max(1.0, float(np.max(np.abs(a[key]))))
            delta = float(np.max(np.abs(a[key] - b[key]))) / scale
            got = float(np.max(np.abs(closed[k][t] - quad[k][t]))) / scale
            print('probit theta_0 {0} {1}: restatement Delta {2:.3e}, device {3:.3e}'.format(
                c['thetas'][t][0], key, delta, got))
            assert got <= delta + TOL


def test_ep_predict_under_the_logit(nat, cases):
    """(130, 5, m = 70): mean, var and the Gauss-Hermite prob against the restatement; the far
    test row returns bitwise (0, e^theta_0, 0.5)."""
    c = cases[0]
    assert c['m'] == 70
    ctx = _ctx(nat, c)
    mean, var, prob, st, nsw = ctx.ep_predict(c['thetas'], c['Xs'])
    ctx.close()
    worst = 0.0
    for t, (th, fit) in enumerate(zip(c['thetas'], c['fit'])):
        assert st[t] == 0 and int(nsw[t]) == fit['n_sweeps']
        G = np.empty((c['n'] + 70, c['n'] + 70))
        orc.c_gram(c['kind'], G, np.concatenate([c['X'], c['Xs']]), th, EPS)
        sigma = math.exp(th[0])
        ref = eq.at_test_inputs(G[c['n']:, :c['n']], sigma, fit, eq.LOGIT)
        for key, got in (('mean', mean), ('var', var), ('prob', prob)):
            scale = 1.0 if key == 'prob' else max(1.0, float(np.abs(ref[key]).max()))
            worst = max(worst, float(np.abs(got[t] - ref[key]).max()) / scale)
        assert (mean[t, -1], var[t, -1], prob[t, -1]) == (0.0, sigma, 0.5)
        assert abs(mean[t, 0] - fit['mu'][I_EQ]) <= 10 * EPS * np.abs(fit['a']).max()
    print('logit EP predict parity: worst {0:.3e}'.format(worst))
    assert worst <= TOL


def _restated_grad(c, th, K, **settings):
    """R&W 5.27 on the restatement's logit fit (ep_grad_restatement's contraction)."""
    fit = eq.ep_fit(K, c['y'], eq.LOGIT, **settings)
    fit['grad'] = eg.grad_of_fit(fit, Cov('se', c['kind']).dK(c['X'], th, EPS, K=K))
    return fit


def test_ep_grad_under_the_logit(nat, cases):
    """(130, 5, ard) at theta_0 = 0.3, fitted at diff_tol = 1e-16. The device's logz is bitwise
    apm_ep_eval's. Its gradient is held twice: to the restatement's own gradient of the same fit
    with test_gpu_ep_grad's tolerance, 1e-9 x max(1, max|grad|); and to central differences
    (h = 1e-5) of the restatement's log Z_EP fitted at 1e-22 with the finite-difference bound that
    test_ep_grad_host and test_gpu_grad apply, 1e-6 x max(1, max|fd|): the differences themselves
    carry ~1e-8 (rounding of log Z over 2 h) and a fit stopped at 1e-16 a few 1e-8 more
    (include/apm.h), so the 1e-9 yardstick cannot be asked of that comparison."""
    c = cases[0]
    th, K = c['thetas'][0], c['K'][0]
    ref = _restated_grad(c, th, K, diff_tol=1e-16, max_sweeps=1000)
    assert_restatement_ok(ref, 1e-16)
    ctx = _ctx(nat, c)
    ctx.set_ep(0.8, 1e-16, 1000)
    assert ctx.ep_quadrature  # (set_ep leaves the switch alone)
    logz, grad, st, nsw = ctx.ep_grad(th)
    fit = ctx.ep(th)
    ctx.close()
    assert st[0] == 0 and int(nsw[0]) == ref['n_sweeps']
    assert logz[0] == fit[0][0]
    scale = max(1.0, float(np.abs(ref['grad']).max()))
    err = max(abs(logz[0] - ref['logz']), float(np.abs(grad[0] - ref['grad']).max())) / scale
    fd = gr.central_differences(
        lambda x: eq.ep_fit(oracle_K(c, x), c['y'], eq.LOGIT, diff_tol=1e-22,
                            max_sweeps=2000)['logz'], th)
    err_fd = float(np.abs(grad[0] - fd).max()) / max(1.0, float(np.abs(fd).max()))
    print('logit EP grad: vs restatement {0:.3e}, vs central differences {1:.3e} '
          '(max|grad| {2:.3e}, {3} sweeps)'.format(err, err_fd, np.abs(fd).max(), ref['n_sweeps']))
    assert err <= TOL
    assert err_fd <= 1e-6


def _draws(n, seed):
    """N(0, 1) draws that fp32 holds exactly (the device keeps U in both precisions)."""
    u = np.random.RandomState(seed).normal(size=(n, N_IMP))
    return u.astype(np.float32).astype(np.float64)


def test_is_ep_theta_and_u_call_under_the_logit(nat, cases):
    """N = 130, S = 64, the three thetas: the theta-call and the u-call against log w_s restated
    at the device's own slot read-back (its f_post and its fp32-rounded factor of C; W = tau~,
    z = nu~ and log|B| from the restatement's fit), within 5e-4 nats; the slot's f_post within
    1e-8 of mu; n_cubic_ops = 2 n_sweeps + 3."""
    c = cases[0]
    ns, ns2 = _draws(c['n'], 11), _draws(c['n'], 12)
    ctx = _ctx(nat, c, n_imp=N_IMP, n_slots=3, n_ubufs=2)
    ctx.u_upload(0, ns)
    ctx.u_upload(1, ns2)
    out, st, nops = ctx.theta_eval(nat.EST_IS_EP, c['thetas'], [0] * 3, [0, 1, 2])
    out_u, st_u = ctx.u_eval([0, 1, 2], [1] * 3)
    slots = [ctx.slot_read(s) for s in range(3)]
    ctx.close()
    for t, fit in enumerate(c['fit']):
        assert st[t] == 0 and st_u[t] == 0
        assert int(nops[t]) == 2 * fit['n_sweeps'] + 3
        L, f, _, cst = slots[t]
        assert np.abs(f - fit['mu']).max() <= 1e-8
        state = dict(f=f, W=fit['tau'], a=fit['nu'] - fit['tau'] * f,
                     logdet_B=2.0 * np.log(fit['L'].diagonal()).sum())
        d_theta = abs(out[t] - lr.is_consistent(c['y'], state, ns, C_chol=L))
        d_u = abs(out_u[t] - lr.is_consistent(c['y'], state, ns2, C_chol=L))
        want_cst = 0.5 * fit['mu'].dot(fit['nu']) - 0.5 * state['logdet_B']
        print('logit IS-EP theta_0 {0}: d theta-call {1:.2e}, u-call {2:.2e}, cst {3:.2e}'.format(
            c['thetas'][t][0], d_theta, d_u, abs(cst - want_cst)))
        assert d_theta <= IS_TOL and d_u <= IS_TOL
        assert abs(cst - want_cst) <= TOL * max(1.0, abs(want_cst))


def test_batch_neutrality(nat, cases, device):
    """Three thetas with three different sweep counts in one call (max_batch = 4) and one by
    one: the fit, the predictive, the gradient and the IS theta-call give the same bits."""
    c = cases[0]
    assert len(set(f['n_sweeps'] for f in c['fit'])) == 3
    ctx = _ctx(nat, c, max_batch=4, n_imp=N_IMP, n_slots=4, n_ubufs=1)
    ctx.u_upload(0, _draws(c['n'], 11))
    full = [ctx.ep(c['thetas']), ctx.ep_predict(c['thetas'], c['Xs']), ctx.ep_grad(c['thetas']),
            ctx.theta_eval(nat.EST_IS_EP, c['thetas'], [0] * 3, [0, 1, 2])]
    for a, b in zip(full[0], device[0]):  # (and max_batch = 3 on another context)
        assert np.array_equal(a, b)
    for t in range(3):
        th = c['thetas'][t]
        one = [ctx.ep(th), ctx.ep_predict(th, c['Xs']), ctx.ep_grad(th),
               ctx.theta_eval(nat.EST_IS_EP, th[None], [0], [3])]
        for fa, fb in zip(full, one):
            for a, b in zip(fa, fb):
                assert np.array_equal(a[t], b[0])
    ctx.close()


def _other_paths(nat, ctx, c):
    """A probit EP fit, a Laplace theta-call and an IS theta-call with its slot, as a flat list."""
    th = c['thetas'][:2]
    out = list(ctx.ep(th))
    out += list(ctx.theta_eval(nat.EST_LAPLACE, th))
    ctx.u_normal([0, 1], [5, 5], [0, 1])
    out += list(ctx.theta_eval(nat.EST_IS, th, [0, 1], [0, 1]))
    for slot in (0, 1):
        L, f, g, cst = ctx.slot_read(slot)
        out += [L, f, g, np.array(cst)]
    return out


def test_the_switch_leaves_the_other_paths_alone(nat):
    """N = 577, a probit context: switch on -> fit -> switch off leaves a following probit fit,
    Laplace theta-call and IS theta-call bitwise equal to a fresh context's. A value other than
    0 / 1 is refused and changes nothing."""
    c = _make_case(577, 4, 3, 'ard', 300 + 577)

    def make():
        return nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=2, n_slots=2,
                           n_ubufs=2)
    ctx = make()
    assert ctx.lib.apm_ep_quadrature(ctx._h) == 0
    before = _other_paths(nat, ctx, c)
    ctx.set_ep_quadrature(True)
    assert ctx.lib.apm_set_ep_quadrature(ctx._h, 2) == nat.APM_E_INVALID
    assert ctx.lib.apm_ep_quadrature(ctx._h) == 1
    assert not ctx.ep(c['thetas'][:2])[5].any()
    ctx.set_ep_quadrature(False)
    assert ctx.lib.apm_ep_quadrature(ctx._h) == 0
    after = _other_paths(nat, ctx, c)
    ctx.close()
    ctx = make()
    fresh = _other_paths(nat, ctx, c)
    ctx.close()
    assert len(before) == len(after) == len(fresh)
    for i, (a, b, f) in enumerate(zip(before, after, fresh)):
        assert np.array_equal(a, b, equal_nan=True), i
        assert np.array_equal(a, f, equal_nan=True), i


def test_refusals_follow_the_switch(nat, cases):
    """A logit context: refused with the switch off as before, accepted with it on, refused again
    once it is off; apm_ep_lik fits the logit stand-alone to apm_ep_eval's values."""
    c = cases[0]
    ctx = _ctx(nat, c, quadrature=False)
    with pytest.raises(nat.NativeError):
        ctx.ep(c['thetas'])
    assert ctx.lib.apm_set_ep(ctx._h, 0.8, 1e-8, 100) == nat.APM_E_INVALID
    ctx.set_ep(0.8, 1e-8, 100, quadrature=True)
    dev = ctx.ep(c['thetas'][0])
    ctx.set_ep_quadrature(False)
    with pytest.raises(nat.NativeError):
        ctx.ep(c['thetas'])
    ctx.close()
    mu, var, tau, nu, C, logz, nsw, st = nat.ep(c['K'][0], c['y'], True, 0.8, DIFF_TOL, 100,
                                                likelihood='logit')
    assert st == 0 and nsw == int(dev[6][0])
    for got, k in ((logz, 0), (mu, 1), (var, 2), (tau, 3), (nu, 4)):
        scale = max(1.0, float(np.max(np.abs(dev[k][0]))))
        assert np.max(np.abs(got - dev[k][0])) <= TOL * scale
    assert np.max(np.abs(np.diag(C) - var) / var) <= 1e-12
    # the stand-alone probit stays the closed form, whatever ran before it on the cached context
    p = nat.ep(c['K'][0], c['y'], False, 0.8, DIFF_TOL, 100)
    q = ep.ep_fit(c['K'][0], c['y'])
    assert p[7] == 0 and p[6] == q['n_sweeps'] and abs(p[5] - q['logz']) <= TOL * abs(q['logz'])


def test_python_classes_run_the_logit(nat, cases, device):
    import gpdemo.estimators as est
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    import gpdemo.predict as prd
    c, dev = cases[0], device[0]
    kf = krn.make_kernel_func('ard', EPS)
    e = est.LogMarginalLikelihoodEPEstimator(c['X'], c['y'], kf, likelihood='logit',
                                             quadrature=True)
    assert e(c['thetas'][0]) == dev[0][0] and e.n_cubic_ops == 2 * int(dev[6][0])
    p = prd.EPPredictor(c['X'], c['y'], kf, c['Xs'], likelihood='logit', quadrature=True)
    prob = p(c['thetas'])[2]
    assert np.array_equal(p.n_iter, dev[6]) and np.all((prob > 0.0) & (prob < 1.0))
    p.close()
    ise = est.LogMarginalLikelihoodApproxPosteriorISEstimator(
        c['X'], c['y'], kf, lpa.ep_approximation, likelihood='logit', quadrature=True)
    v, cache = ise(_draws(c['n'], 11), c['thetas'][0])
    assert np.isfinite(v) and cache.kind == nat.EST_IS_EP


def test_batched_samplers_run_is_ep_under_the_logit(nat):
    """estimator='is_ep', likelihood='logit', ep_settings={'quadrature': True}: two chains, three
    transitions, N = 130; the two chains together and each alone give the same bits;
    sampler.predict and sampler.loo() return finite values."""
    from auxpm.batched import BatchedPMMHSampler
    c = _make_case(130, 5, 70, 'ard', 100)
    prior = dict(a_tau=1., b_tau=1. / c['d'] ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(c['d'], 0.5 * math.log(c['d']))], (2, 1))
    th0[1, 0] = 0.5
    kw = dict(prop_scales=0.1, seed=71, kernel='ard', estimator='is_ep', likelihood='logit',
              ep_settings=dict(quadrature=True))
    both = BatchedPMMHSampler(c['X'], c['y'], 2, 16, prior, **kw)
    assert both.est == nat.EST_IS_EP and both.ctx.ep_quadrature
    th, nrej = both.get_samples(3, th0)
    assert np.isfinite(th).all() and not both.failed.any() and np.isfinite(both.log_f).all()
    prob, ess = both.predict(c['Xs'])
    loo = both.loo()
    assert np.isfinite(prob).all() and np.isfinite(ess).all()
    assert all(np.isfinite(loo[k]).all() for k in ('loo', 'lpd', 'ess_loo', 'gauss', 'ess'))
    for ch in range(2):
        one = BatchedPMMHSampler(c['X'], c['y'], 1, 16, prior, first_chain=ch, **kw)
        th1, nrej1 = one.get_samples(3, th0[ch:ch + 1])
        assert np.array_equal(th1[0], th[ch]) and nrej1[0] == nrej[ch]
        assert one.log_f[0] == both.log_f[ch]
