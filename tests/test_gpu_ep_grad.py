"""Gradient of log Z_EP with respect to theta on the device (apm_ep_grad; host_laplace.cpp's
ep_grad_block on gradient.hip's kernels) against the numpy restatement
(tests/ep_grad_restatement.py), plus the properties that need no oracle: the logz identity, batch
neutrality, that a call leaves every other path's results alone, failure mapping, refusals, the
epsilon rule and the Python class with its L-BFGS fit."""
import math

import numpy as np
import pytest

import cov_restatement as cr
from cov_restatement import Cov
from test_gpu_ep import EDGE_N, assert_stop_margin
from test_gpu_predict import SHAPES, _make_case

pytestmark = pytest.mark.gpu

EPS = 1e-8
# device-to-restatement tolerance of logz and grad (x max(1, max|ref grad|)): fp64 against fp64
# through the same algebra, the yardstick of DESIGN.md §12, §13 and §16. The measured maxima are
# in DESIGN.md §18.
TOL = 1e-9
# Every parity case runs the default EP settings on test_gpu_ep's data (test_gpu_predict's
# recipe and seeds), so that file's stop-margin property carries over: the restatement's last
# stop measure is below 0.99 diff_tol and the one before above 1.01 diff_tol (asserted per case),
# and device and restatement cannot disagree on the sweep count.
KINDS = {('se', 'iso'): 'KERNEL_ISO', ('se', 'ard'): 'KERNEL_ARD',
         ('32', 'iso'): 'KERNEL_M32_ISO', ('52', 'ard'): 'KERNEL_M52_ARD'}


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


@pytest.fixture(scope='module')
def cases():
    """Data and restatement gradients per shape of test_gpu_predict (three thetas each),
    computed once, left unchanged."""
    out = []
    for i, (n, d, m, kind) in enumerate(SHAPES):
        c = _make_case(n, d, m, kind, 100 + i)
        c['ref'] = [cr.ep_grad(Cov('se', kind), c['X'], c['y'], th, EPS) for th in c['thetas']]
        out.append(c)
    return out


def _context(nat, c, family='se', eps=EPS, max_batch=3, likelihood='probit', **kw):
    kw.setdefault('n_slots', 1)
    kw.setdefault('n_ubufs', 1)
    return nat.Context(c['X'], c['y'], getattr(nat, KINDS[family, c['kind']]), eps,
                       kw.pop('n_imp', 1), max_batch=max_batch, likelihood=likelihood, **kw)


def _device(nat, c, thetas, family='se', eps=EPS):
    ctx = _context(nat, c, family, eps)
    out = ctx.ep_grad(thetas)
    ctx.close()
    return out


def _parity(dev, t, ref):
    """max of |logz - ref| and |grad - ref| over max(1, max|ref grad|); status 0 and the
    restatement's sweep count first."""
    logz, grad, st, nsw = dev
    assert_stop_margin(ref)
    assert st[t] == 0 and int(nsw[t]) == ref['n_sweeps']
    scale = max(1.0, float(np.abs(ref['grad']).max()))
    return max(abs(logz[t] - ref['logz']), float(np.abs(grad[t] - ref['grad']).max())) / scale


@pytest.fixture(scope='module')
def device(nat, cases):
    """apm_ep_grad per shape: one call, three thetas."""
    return [_device(nat, c, c['thetas']) for c in cases]


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_ep_grad_vs_restatement(cases, device, ci):
    c = cases[ci]
    worst = 0.0
    for t, ref in enumerate(c['ref']):
        err = _parity(device[ci], t, ref)
        print('EP grad parity shape {0} theta_0 {1}: {2:.3e} (max|grad| {3:.3e}, {4} sweeps)'
              .format(SHAPES[ci], c['thetas'][t][0], err, np.abs(ref['grad']).max(),
                      ref['n_sweeps']))
        worst = max(worst, err)
    print('EP grad parity shape {0}: worst {1:.3e} (tol {2:.0e})'.format(SHAPES[ci], worst, TOL))
    assert worst <= TOL


@pytest.mark.parametrize('n', EDGE_N)
def test_panel_edges(nat, n):
    """d = 4, ARD, theta_0 = 0.3 at the tile and outer-panel boundaries (nb = 2, 8, 9, 10)."""
    c = _make_case(n, 4, 3, 'ard', 300 + n)
    th = c['thetas'][0]
    ref = cr.ep_grad(Cov('se', 'ard'), c['X'], c['y'], th, EPS)
    err = _parity(_device(nat, c, th), 0, ref)
    print('EP grad parity N = {0}: {1:.3e}'.format(n, err))
    assert err <= TOL


@pytest.mark.parametrize('family,kind,n,d,seed', [('52', 'ard', 513, 4, 300 + 513),
                                                  ('32', 'iso', 130, 3, 501)])
def test_matern(nat, family, kind, n, d, seed):
    """The Matern families on cov_restatement's own Gram (the C oracle builds SE only): the
    two-pass instantiation of the contraction kernel, ARD at a panel edge and iso."""
    c = _make_case(n, d, 3, kind, seed)
    th = c['thetas'][0]
    ref = cr.ep_grad(Cov(family, kind), c['X'], c['y'], th, EPS)
    err = _parity(_device(nat, c, th, family), 0, ref)
    print('EP grad parity Matern {0} {1} N = {2}: {3:.3e}'.format(family, kind, n, err))
    assert err <= TOL


def test_logz_is_ep_evals_and_batches_are_bitwise_neutral(nat, cases, device):
    """logz is bitwise Context.ep's; three thetas with three different sweep counts give the same
    bits in one call (max_batch = 4) and one by one."""
    c = cases[0]
    assert len(set(r['n_sweeps'] for r in c['ref'])) == 3
    ctx = _context(nat, c, max_batch=4)
    full = ctx.ep_grad(c['thetas'])
    fit = ctx.ep(c['thetas'])
    assert len(set(full[3].tolist())) == 3 and not full[2].any()
    assert np.array_equal(full[0], fit[0]) and np.array_equal(full[3], fit[6])
    for t in range(3):
        one = ctx.ep_grad(c['thetas'][t])
        for a, b in zip(full, one):
            assert np.array_equal(a[t], b[0])
    ctx.close()
    for a, b in zip(full, device[0]):  # (and max_batch = 3 on another context)
        assert np.array_equal(a, b)


def _other_paths(nat, ctx, c):
    """Everything the other paths return on one context, as a flat list of arrays."""
    th = c['thetas'][:2]
    out = list(ctx.laplace_grad(th))
    out += list(ctx.theta_eval(nat.EST_LAPLACE, th))
    out += list(ctx.predict(th, c['Xs']))
    out += list(ctx.ep(th))
    for est in (nat.EST_IS, nat.EST_IS_EP):
        ctx.u_normal([0, 1], [5, 5], [0, 1])
        out += list(ctx.theta_eval(est, th, [0, 1], [0, 1]))
        out += list(ctx.u_eval([0, 1], [1, 0]))
        for slot in (0, 1):
            L, f, g, cst = ctx.slot_read(slot)
            out += [L, f, g, np.array(cst)]
    return out


def test_ep_grad_leaves_the_other_paths_alone(nat):
    """N = 577: laplace_grad, the Laplace theta-call, predict, ep, and an EST_IS and an EST_IS_EP
    theta-call each with its u-call and slot read-back, before and after an ep_grad call on the
    same context, and on a fresh context: all bitwise the same."""
    c = _make_case(577, 4, 3, 'ard', 300 + 577)

    def make():
        return _context(nat, c, max_batch=2, n_imp=8, n_slots=2, n_ubufs=2)
    ctx = make()
    before = _other_paths(nat, ctx, c)
    st = ctx.ep_grad(c['thetas'][:2])[2]
    assert not st.any()
    after = _other_paths(nat, ctx, c)
    ctx.close()
    ctx = make()
    fresh = _other_paths(nat, ctx, c)
    ctx.close()
    assert len(before) == len(after) == len(fresh)
    for i, (a, b, f) in enumerate(zip(before, after, fresh)):
        assert np.all(np.isfinite(a)), i
        assert np.array_equal(a, b), i
        assert np.array_equal(a, f), i


def test_failures_and_refusals(nat, cases, device):
    import ep_restatement as ep
    c = cases[0]
    P = c['thetas'].shape[1]
    easy = c['thetas'][0].copy()
    easy[0] = -16.0  # mu ~ n e^-16: the second sweep already moves it by less than the tolerance
    assert ep.ep_fit(Cov('se', 'ard').gram(c['X'], easy, EPS), c['y'])['n_sweeps'] == 2
    thetas = np.array([easy, c['thetas'][0]])
    ctx = _context(nat, c, max_batch=2)
    alone = ctx.ep_grad(easy)
    ctx.set_ep(0.8, 1e-8, 2)
    bad = ctx.ep_grad(thetas)
    assert list(bad[2]) == [nat.STATUS_OK, nat.STATUS_MAXITER] and list(bad[3]) == [2, 2]
    assert np.isnan(bad[0][1]) and np.all(np.isnan(bad[1][1]))
    assert bad[0][0] == alone[0][0] and np.array_equal(bad[1][0], alone[1][0])
    assert np.all(np.isfinite(bad[1][0]))
    ctx.set_ep()  # the defaults
    good = ctx.ep_grad(thetas)
    assert list(good[2]) == [0, 0]
    assert good[0][1] == device[0][0][0] and np.array_equal(good[1][1], device[0][1][0])

    th = np.ascontiguousarray(np.vstack([thetas, thetas[:1]]))
    grad = np.full((3, P), 7.25)
    st = np.full(3, -1, dtype=np.int32)

    def call(h, count, ldt, ldg, g=grad):
        return ctx.lib.apm_ep_grad(h, count, th.ctypes.data, ldt, None,
                                   None if g is None else g.ctypes.data, ldg, st.ctypes.data,
                                   None)
    bad_rc = nat.APM_E_INVALID
    assert call(ctx._h, 3, P, P) == bad_rc and b'max_batch' in ctx.lib.apm_last_error(ctx._h)
    assert call(ctx._h, 0, P, P) == bad_rc
    assert call(ctx._h, 2, P, P - 1) == bad_rc and b'ldg' in ctx.lib.apm_last_error(ctx._h)
    assert call(ctx._h, 2, P - 1, P) == bad_rc and b'ldt' in ctx.lib.apm_last_error(ctx._h)
    assert call(ctx._h, 2, P, P, g=None) == bad_rc
    assert np.all(grad == 7.25) and np.all(st == -1)
    # logz and n_sweeps may be NULL; a wider ldg leaves its padding alone
    wide = np.full((2, P + 2), 7.25)
    assert call(ctx._h, 2, P, P + 2, g=wide) == 0
    assert np.array_equal(wide[:, :P], good[1]) and np.all(wide[:, P:] == 7.25)
    assert list(st) == [0, 0, -1]
    ctx.close()
    lg = _context(nat, c, max_batch=2, likelihood='logit')
    assert call(lg._h, 2, P, P) == bad_rc and b'probit' in lg.lib.apm_last_error(lg._h)
    with pytest.raises(nat.NativeError):
        lg.ep_grad(thetas)
    lg.close()
    pre = nat.Context(None, c['y'], nat.KERNEL_PRECOMPUTED, EPS, 1)
    assert call(pre._h, 1, P, P) == bad_rc and b'ISO or ARD' in pre.lib.apm_last_error(pre._h)
    pre.close()
    assert np.all(grad == 7.25)


def test_epsilon_rule(nat, cases):
    """Contexts with epsilon = 1e-2: dK/dtheta_0's diagonal is s, not s + epsilon; the wrong
    reading moves the restatement's grad[0] by epsilon * trace(M), which must be visible."""
    c = cases[0]
    thetas = c['thetas'][[0, 2]]
    dev = _device(nat, c, thetas, eps=1e-2)
    for t, th in enumerate(thetas):
        ref = cr.ep_grad(Cov('se', 'ard'), c['X'], c['y'], th, 1e-2)
        wrong = cr.ep_grad(Cov('se', 'ard'), c['X'], c['y'], th, 1e-2, wrong='eps_in_dk0')
        err = _parity(dev, t, ref)
        off = np.abs(dev[1][t] - wrong['grad']).max() / max(1.0, np.abs(ref['grad']).max())
        print('epsilon rule theta_0 {0}: parity {1:.3e}, wrong reading off by {2:.3e}'
              .format(th[0], err, off))
        assert err <= TOL
        assert off > 1e-6


def test_ep_gradient_class_and_maximise(nat, cases):
    """EPGradient returns Context.ep_grad's bits at the same settings; its MAP fit on
    (130, 3, ard) from theta_0 = 0, length scales 1/2 log d, under a N(0, 3^2) prior: L-BFGS-B
    reports success, the device gradient of the log posterior at x is within gtol in the
    max-norm, and log Z_EP does not end below its start."""
    import gpdemo.gradients as gd
    import gpdemo.kernels as krn
    from gpdemo.latent_posterior_approximations import MaximumIterationsExceededError
    c = cases[0]
    kf = krn.make_kernel_func('ard', EPS)
    p = gd.EPGradient(c['X'], c['y'], kf, max_batch=2)
    logz, grad = p(c['thetas'])
    ctx = _context(nat, c)
    ctx.set_ep(0.8, 1e-16, 1000)
    want = ctx.ep_grad(c['thetas'])
    ctx.close()
    assert np.array_equal(logz, want[0]) and np.array_equal(grad, want[1])
    assert np.array_equal(p.n_sweeps, want[3]) and not p.status.any()
    p.close()
    p2 = gd.EPGradient(c['X'], c['y'], kf, max_sweeps=2)
    with pytest.raises(MaximumIterationsExceededError):
        p2(c['thetas'][0])
    got = p2(c['thetas'][0], on_error='nan')
    assert np.isnan(got[0][0]) and list(p2.status) == [nat.STATUS_MAXITER]
    p2.close()

    m = _make_case(130, 3, 3, 'ard', 130)
    p = gd.EPGradient(m['X'], m['y'], kf)
    theta0 = np.r_[0.0, np.full(3, 0.5 * math.log(3))]
    start, _ = p(theta0)
    res = p.maximise(theta0, prior_mean=0.0, prior_std=3.0, gtol=1e-5)
    val, g = p.log_posterior(res.x, 0.0, 3.0)
    end, _ = p(res.x)
    p.close()
    print('EP maximise: {0} evaluations, {1} iterations, log Z_EP {2:.6f} -> {3:.6f}, '
          'max|grad| {4:.2e}'.format(res.nfev, res.nit, start[0], end[0], np.abs(g).max()))
    assert res.success
    assert np.abs(g[0]).max() <= 1e-5
    assert end[0] >= start[0]
    assert res.logz == end[0] and res.value == val[0] and np.array_equal(res.grad, g[0])
    assert 'lml' not in res
