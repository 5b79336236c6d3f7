"""Laplace predictive distribution on the device (apm_predict / apm_gram_cross, predict.hip)
against a numpy/scipy restatement, plus the properties that need no oracle: exact values at a
far and at a coinciding test point, block / batch independence, failure mapping, and that a
predict call leaves cache slots alone."""
import math

import numpy as np
import pytest

import apm_oracle as orc
from predict_restatement import predictive

pytestmark = pytest.mark.gpu

EPS = 1e-8
# device-to-oracle tolerance of mean / var (x max(1, max|ref|)) and prob (absolute): fp64 against
# fp64 through the same factorisation, the Laplace-mode yardstick of DESIGN.md §5 (f to 1e-9
# relative, test_laplace_vs_golden). The measured maximum over all cases below is 4.5e-14
# (DESIGN.md §12), more than 10x below it, so the yardstick stands.
TOL = 1e-9
# (n, d, m, kind): tiles that are not full, d across two LDS chunks, one test point, full tiles;
# the last one (predict parity only) has more than one outer panel (nb = 10 > 8), so its test
# rows also take the rank-256 trailing update
SHAPES = [(130, 5, 70, 'ard'), (129, 40, 1, 'ard'), (200, 3, 65, 'iso'), (64, 33, 64, 'ard'),
          (600, 4, 70, 'ard')]
SIGMAS = (0.3, 3.0, -1.0)  # theta_0 of the three thetas per shape
I_EQ = 7                   # test row 0 coincides with this training row (m >= 3)


def _assert_gram_close(K, Kref):
    """exp(-s/2) carries the exponent's relative rounding (x s) into K: bound the error relative
    to the exponent, 2e-15 * max(1, |log K|), i.e. a few ulp of s."""
    scale = np.maximum(1.0, np.abs(np.log(np.maximum(Kref, 1e-300))))
    bad = np.abs(K - Kref) > 2e-15 * scale * np.abs(Kref) + 1e-300
    assert not bad.any(), (np.abs(K - Kref)[bad].max(), bad.sum())


_oracle = predictive  # (the restatement, shared with test_gpu_laplace_edges.py)


def _make_case(n, d, m, kind, seed):
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) > 0, 1.0, -1.0)
    Xs = rng.normal(size=(m, d))
    if m >= 3:
        Xs[0] = X[I_EQ]        # coincides with a training point: k* = sigma there, no epsilon
        Xs[-1] = X[3] + 50.0   # 50 units away in every coordinate: k* underflows to 0
    # length scales around sqrt(d) (at most 1.11 sqrt(d): the far row's exponent is >= ~890)
    nl = d if kind == 'ard' else 1
    thetas = np.array([np.r_[s0, 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=nl)]
                       for s0 in SIGMAS])
    return dict(n=n, d=d, m=m, kind=kind, X=X, y=y, Xs=Xs, thetas=thetas)


@pytest.fixture(scope='module')
def cases():
    """Data and oracle results per shape, computed once and left unchanged."""
    out = []
    for i, (n, d, m, kind) in enumerate(SHAPES):
        c = _make_case(n, d, m, kind, 100 + i)
        c['ref'] = []
        for th in c['thetas']:
            G = np.empty((n + m, n + m))
            orc.c_gram(kind, G, np.concatenate([c['X'], c['Xs']]), th, EPS)
            ref = _oracle(G[:n, :n].copy(), G[n:, :n].copy(), c['y'], math.exp(th[0]))
            ref['Ks'] = G[n:, :n].copy()
            c['ref'].append(ref)
        out.append(c)
    return out


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _kind(nat, kind):
    return nat.KERNEL_ISO if kind == 'iso' else nat.KERNEL_ARD


def _predictor(c, Xs=None, **kw):
    import gpdemo.kernels as krn
    import gpdemo.predict as prd
    return prd.LaplacePredictor(c['X'], c['y'], krn.make_kernel_func(c['kind'], EPS),
                                c['Xs'] if Xs is None else Xs, **kw)


@pytest.fixture(scope='module')
def device(nat, cases):
    """Device predictions per shape (one predictor call each, three thetas)."""
    out = []
    for c in cases:
        p = _predictor(c)
        mean, var, prob = p(c['thetas'])
        out.append(dict(mean=mean, var=var, prob=prob, n_iter=p.n_iter.copy()))
        p.close()
    return out


@pytest.mark.parametrize('ci', range(4))  # (the extra shape is there for the solve's update path)
def test_gram_cross_vs_c_oracle(nat, cases, ci):
    c = cases[ci]
    for th, ref in zip(c['thetas'], c['ref']):
        Ks = nat.gram_cross(_kind(nat, c['kind']), c['Xs'], c['X'], th)
        assert Ks.shape == (c['m'], c['n'])
        _assert_gram_close(Ks, ref['Ks'])
        if c['m'] >= 3:
            assert Ks[0, I_EQ] == math.exp(th[0])  # coinciding point: sigma, not sigma + epsilon
            assert np.all(Ks[-1] == 0.0)           # the far row underflows to exactly 0


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_predict_vs_oracle(cases, device, ci):
    c, dev = cases[ci], device[ci]
    worst = 0.0
    for t, ref in enumerate(c['ref']):
        assert int(dev['n_iter'][t]) == ref['n_iter']
        for key in ('mean', 'var', 'prob'):
            scale = 1.0 if key == 'prob' else max(1.0, np.abs(ref[key]).max())
            err = np.abs(dev[key][t] - ref[key]).max() / scale
            worst = max(worst, err)
            print('predict parity shape {0} theta {1} {2}: {3:.3e}'.format(SHAPES[ci], t, key, err))
    print('predict parity shape {0}: worst {1:.3e} (tol {2:.0e})'.format(SHAPES[ci], worst, TOL))
    assert worst <= TOL


@pytest.mark.parametrize('ci', [i for i, s in enumerate(SHAPES) if s[2] >= 3])
def test_exact_properties(nat, cases, device, ci):
    c, dev = cases[ci], device[ci]
    n = c['n']
    for t, th in enumerate(c['thetas']):
        sigma = math.exp(th[0])
        # the far row: k* = 0 exactly, so the prior comes back untouched
        assert dev['mean'][t, -1] == 0.0
        assert dev['var'][t, -1] == sigma
        assert dev['prob'][t, -1] == 0.5
        # the coinciding row: k* = K[i, :] - epsilon e_i, so mu* = f_i - epsilon a_i
        K = np.empty((n, n))
        nat.gram(_kind(nat, c['kind']), K, c['X'], th, EPS)
        f = nat.laplace(K, c['y'], False, False, 1e-4, 1000)[0]
        amax = np.abs(c['ref'][t]['a']).max()
        assert abs(dev['mean'][t, 0] - f[I_EQ]) <= 10 * EPS * amax
        assert np.all(dev['var'][t] > 0.0) and np.all(dev['var'][t] <= sigma)


def test_blocks_and_batches_are_bitwise_neutral(nat):
    """n = 130 (np = 192) with m = 200: two passes over the free rows; max_batch = 2 with three
    thetas: two chunks. Each theta alone, and the test points in two calls of 100, give the same
    bits."""
    c = _make_case(130, 5, 200, 'ard', 7)
    p = _predictor(c, max_batch=2)
    full = p(c['thetas'])
    for t in range(3):
        one = p(c['thetas'][t])
        for a, b in zip(full, one):
            assert np.array_equal(a[t], b[0])
    p.close()
    halves = []
    for lo in (0, 100):
        q = _predictor(c, Xs=c['Xs'][lo:lo + 100], max_batch=2)
        halves.append(q(c['thetas']))
        q.close()
    for k in range(3):
        assert np.array_equal(full[k], np.concatenate([halves[0][k], halves[1][k]], axis=1))


def test_failure_mapping(nat):
    from gpdemo.latent_posterior_approximations import MaximumIterationsExceededError
    c = _make_case(130, 5, 70, 'ard', 8)
    easy = c['thetas'][0].copy()
    easy[0] = -12.0  # |f| ~ n sigma: the first Newton step already moves f by less than the tol
    thetas = np.array([easy, c['thetas'][0], easy + 0.01])
    p = _predictor(c)
    good = p(thetas)
    assert list(p.n_iter[[0, 2]]) == [1, 1] and p.n_iter[1] > 1
    p.close()
    p1 = _predictor(c, max_iters=1)
    with pytest.raises(MaximumIterationsExceededError):
        p1(thetas)
    got = p1(thetas, on_error='nan')
    assert list(p1.status) == [nat.STATUS_OK, nat.STATUS_MAXITER, nat.STATUS_OK]
    for g, r in zip(got, good):
        assert np.all(np.isnan(g[1]))
        assert np.array_equal(g[[0, 2]], r[[0, 2]])
    p1.close()


def test_invalid_arguments(nat):
    c = _make_case(64, 3, 5, 'ard', 9)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 1, max_batch=2, n_slots=1, n_ubufs=1)
    th = np.ascontiguousarray(c['thetas'])
    out = np.empty((3, 5))
    st = np.zeros(3, dtype=np.int32)

    def call(count, m, ldo, h=ctx._h):
        return ctx.lib.apm_predict(h, count, th.ctypes.data, th.shape[1], c['Xs'].ctypes.data, m,
                                   3, out.ctypes.data, None, None, ldo, st.ctypes.data, None)
    assert call(2, 0, 5) == nat.APM_E_INVALID and b'm <= 0' in ctx.lib.apm_last_error(ctx._h)
    assert call(3, 5, 5) == nat.APM_E_INVALID and b'max_batch' in ctx.lib.apm_last_error(ctx._h)
    assert call(2, 5, 4) == nat.APM_E_INVALID and b'ldo' in ctx.lib.apm_last_error(ctx._h)
    assert call(2, 5, 5) == 0 and list(st[:2]) == [0, 0] and np.all(np.isfinite(out[:2]))
    ctx.close()
    pre = nat.Context(None, c['y'], nat.KERNEL_PRECOMPUTED, EPS, 1)
    assert call(1, 5, 5, pre._h) == nat.APM_E_INVALID
    assert b'ISO or ARD' in pre.lib.apm_last_error(pre._h)
    pre.close()


def test_predict_leaves_cache_slots_alone(nat):
    """An IS theta-call into a slot, a predict call on the same context (it shares the work
    matrix), then the slot's u-call: the same bits as before the predict call."""
    c = _make_case(130, 5, 70, 'ard', 10)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=2, n_slots=2, n_ubufs=2)
    ctx.u_normal([0, 1], [5, 5], [0, 1])
    slot = ctx.slots.acquire()
    _, st, _ = ctx.theta_eval(nat.EST_IS, c['thetas'][:1], [0], [slot])
    assert st[0] == 0
    before, st = ctx.u_eval([slot], [1])
    assert st[0] == 0
    mean, _, _, pst, _ = ctx.predict(c['thetas'], c['Xs'])
    assert list(pst) == [0, 0, 0] and np.all(np.isfinite(mean))
    after, st = ctx.u_eval([slot], [1])
    assert st[0] == 0 and np.array_equal(before, after)
    ctx.close()
