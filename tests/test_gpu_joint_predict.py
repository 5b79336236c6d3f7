"""The joint Laplace / EP predictive on the device (apm_predict_joint, predict_joint.hip; DESIGN.md
§31) against tests/joint_predict_restatement.py: mean, covariance, draws and the joint log
predictive density over the covariance kinds, both likelihoods and both fits, at every block
size that takes another path through the tiles; batch neutrality with a failing chain beside the
others, NULL outputs, the refusals, the factor's failure status and the Python layer.

Figures measured on an MI355X are in DESIGN.md §31."""
import math

import numpy as np
import pytest

import apm_oracle as orc
import joint_predict_restatement as jr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = 1e-8
TOL = 1e-9          # fp64 against fp64 through the same factorisation (x max(1, max|ref|))
FLOOR = 1e-12       # the floor of the yardstick rule for draws and lpd (x scale)
YARD = 16.0         # ... and its multiple of the fp64 / long-double gap
MS = (1, 63, 64, 65, 130)
S = 100             # draws per chain: two draw tiles, the second one partly filled
# Both fits run to a state that does not depend on where exactly a stop measure crosses its
# tolerance. Newton: diff_f_tol = 1e-16 with the last diff of the restatement <= 1e-18 and the one
# before > 1.1e-16 (quadratic convergence: the step after a diff of 1e-16 is rounding), so the
# device stops at the same iteration. EP: diff_tol with the restatement's last stop measure < 0.9
# and the one before > 1.1 of it. A stop measure is a mean of squared steps of ~1e-8, which the
# device and numpy form to ~1e-7 relative. Both margins are asserted when the references are built.
NEWTON_TOL, EP_TOL = 1e-16, 1e-16
# (n, d, covariance, likelihood, fit): n = 130 and 161 both pad to two 64-tiles and a remainder
CASES = [
    (130, 3, Cov('se', 'iso'), 'probit', 'laplace'),
    (130, 5, Cov('se', 'ard'), 'logit', 'laplace'),
    (161, 5, Cov('52', 'ard'), 'probit', 'ep'),
    (161, 4, Cov('se', 'ard', bias=True, linear=True), 'logit', 'ep'),
    (161, 4, Cov('se', 'ard', bias=True, linear=True), 'probit', 'laplace'),
    (130, 5, Cov('52', 'ard'), 'logit', 'laplace'),
]
IDS = ['{0}-{2.family}-{2.kind}{3}-{4}-{5}'.format(n, d, c, '-bias-linear' if c.linear else '',
                                                   lik, fit) for n, d, c, lik, fit in CASES]
SIGMAS = (0.3, 1.0)  # theta_0 of the two thetas per case


def make_case(n, d, cov, lik, fit, seed):
    """Inputs, labels, two thetas, test inputs and test labels. The test inputs are drawn twice
    as wide as the training inputs, so that they lie away from them and from each other and
    Sigma + eps I is well conditioned."""
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=n) > 0, 1.0, -1.0)
    Xs = 2.0 * rng.normal(size=(max(MS), d))
    ys = np.where(Xs[:, 0] + 0.5 * rng.normal(size=max(MS)) > 0, 1.0, -1.0)
    nl = d if cov.kind == 'ard' else 1
    thetas = np.array([np.r_[s0, 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=nl),
                             [0.5] * cov.bias, [-2.0] * cov.linear] for s0 in SIGMAS])
    return dict(n=n, d=d, cov=cov, lik=lik, fit=fit, X=X, y=y, Xs=Xs, ys=ys, thetas=thetas)


def fit_state(c, th):
    """The restatement's fit at the tests' tolerances, its margin asserted."""
    if c['fit'] == 'ep':
        st = jr.ep_state(c['cov'], c['X'], c['y'], th, EPS, lik=c['lik'],
                         quadrature=c['lik'] == 'logit', diff_tol=EP_TOL, max_sweeps=400)
        assert st['diffs'][-1] < 0.9 * EP_TOL and st['diffs'][-2] > 1.1 * EP_TOL, st['diffs'][-2:]
    else:
        st = jr.laplace_state(c['cov'], c['X'], c['y'], th, EPS, tol=NEWTON_TOL, lik=c['lik'])
        assert st['diffs'][-1] <= 1e-18 and st['diffs'][-2] > 1.1 * NEWTON_TOL, st['diffs'][-2:]
    return st


_CASES = {}


def case(ci):
    """Data and fits of one case, built once and left unchanged."""
    if ci not in _CASES:
        c = make_case(*CASES[ci], seed=3100 + ci)
        c['states'] = [fit_state(c, th) for th in c['thetas']]
        _CASES[ci] = c
    return _CASES[ci]


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def context(nat, c, eps=EPS, n_imp=S, max_batch=3):
    ctx = nat.Context(c['X'], c['y'], c['cov'].native_kind, eps, n_imp, max_batch=max_batch,
                      n_slots=1, n_ubufs=max_batch, likelihood=c['lik'],
                      ep_quadrature=c['fit'] == 'ep' and c['lik'] == 'logit')
    ctx.set_newton(NEWTON_TOL, 100)
    if c['fit'] == 'ep':
        ctx.set_ep(0.8, EP_TOL, 400)
    return ctx


def approx(nat, c):
    return nat.JOINT_EP if c['fit'] == 'ep' else nat.JOINT_LAPLACE


def device_stream(ctx, seeds, counters, m):
    """The device's own normals for the chains' (seed, counter): apm_u_normal fills a U buffer
    (n x n_imp, row-major) with the stream's elements in order, so with n_imp = the number of
    draws its first m rows are the m x n_draws matrix xi of the joint call."""
    idx = np.arange(len(seeds))
    ctx.u_normal(idx, seeds, counters)
    return [ctx.u_download(int(b))[:m].copy() for b in idx]


def marginal(ctx, c, thetas, Xs):
    fn = ctx.ep_predict if c['fit'] == 'ep' else ctx.predict
    return fn(thetas, Xs)


@pytest.mark.parametrize('ci', range(len(CASES)), ids=IDS)
def test_joint_vs_restatement(nat, ci):
    """Per block size m and theta:
      mean   bitwise the marginal call's;
      cov    exactly symmetric, its diagonal within 1e-9 k** of the marginal call's variance, all
             of it within 1e-9 max(1, max|ref|) of the restatement;
      draws, lpd  within max(16 gap, 1e-12 scale) of the fp64 restatement, gap its distance to the
             long-double one, scale = max|draw| resp. max(1, |lpd|).
    The restatement is fed the stream the device draws from, read back through apm_u_normal /
    apm_u_download (the same generator, philox.h), because the oracle's u_normal evaluates the
    Box-Muller transcendentals in fp64 and the device in fp32: the two agree to 2e-6 (asserted
    here as test_gpu_slot_state.py does), not to the rounding of fp64."""
    c = case(ci)
    ctx = context(nat, c)
    seeds, counters = np.array([41, 2 ** 40 + 7], dtype=np.uint64), np.array([0, 3], dtype=np.uint64)
    worst = dict(var=0.0, cov=0.0, draws=0.0, lpd=0.0, gap_draws=0.0, gap_lpd=0.0)
    try:
        for m in MS:
            Xs, ys = c['Xs'][:m], c['ys'][:m]
            xis = device_stream(ctx, seeds, counters, m)
            for b in range(2):
                ref = orc.u_normal(int(seeds[b]), int(counters[b]), m, S)
                np.testing.assert_allclose(xis[b], ref, rtol=2e-6, atol=2e-6)
            mean, cov, draws, lpd, st, nit = ctx.predict_joint(
                approx(nat, c), c['thetas'], Xs, n_draws=S, seeds=seeds, counters=counters,
                want_draws=True, y_test=ys)
            mmean, mvar, _, mst, mnit = marginal(ctx, c, c['thetas'], Xs)
            assert list(st) == [0, 0] and list(mst) == [0, 0]
            assert list(nit) == list(mnit) == [s['n_iter'] for s in c['states']]
            assert np.array_equal(mean, mmean)
            for t, th in enumerate(c['thetas']):
                args = (c['cov'], c['X'], Xs, th, c['states'][t], EPS)
                ref = jr.at_test_inputs(*args, xi=xis[t], ys=ys, lik=c['lik'])
                ref_ld = jr.at_test_inputs_ld(*args, xi=xis[t], ys=ys, lik=c['lik'])
                kss = c['cov'].prior_var(Xs, th) * np.ones(m)
                assert np.array_equal(cov[t], cov[t].T)
                e_var = float(np.max(np.abs(cov[t].diagonal() - mvar[t]) / kss))
                e_cov = float(np.abs(cov[t] - ref['cov']).max() / max(1.0, np.abs(ref['cov']).max()))
                gd, gl = jr.gap(ref, ref_ld, 'draws'), jr.gap(ref, ref_ld, 'lpd')
                sd, sl = float(np.abs(ref['draws']).max()), max(1.0, abs(ref['lpd']))
                e_d = float(np.abs(draws[t] - ref['draws']).max())
                e_l = abs(float(lpd[t]) - ref['lpd'])
                print('joint {0} m={1} theta {2}: var {3:.2e} cov {4:.2e} | draws err {5:.2e} gap '
                      '{6:.2e} scale {7:.2e} | lpd err {8:.2e} gap {9:.2e} scale {10:.2e}'
                      .format(IDS[ci], m, t, e_var, e_cov, e_d, gd, sd, e_l, gl, sl))
                for k, v in (('var', e_var), ('cov', e_cov), ('draws', e_d / sd), ('lpd', e_l / sl),
                             ('gap_draws', gd / sd), ('gap_lpd', gl / sl)):
                    worst[k] = max(worst[k], v)
                assert np.abs(mean[t] - ref['mean']).max() <= TOL * max(1.0, np.abs(ref['mean']).max())
                assert e_var <= TOL
                assert e_cov <= TOL
                assert e_d <= max(YARD * gd, FLOOR * sd), (m, t, e_d, gd, sd)
                assert e_l <= max(YARD * gl, FLOOR * sl), (m, t, e_l, gl, sl)
    finally:
        ctx.close()
    print('joint {0} worst: {1}'.format(IDS[ci], worst))


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize('ci', (0, 3), ids=[IDS[0], IDS[3]])
def test_batch_position_and_a_failing_chain(nat, ci):
    """A chain's outputs are bitwise the same alone (count = 1), first or last of three, and
    beside a chain that fails: with one Newton iteration (two EP sweeps) allowed, a theta with a
    tiny amplitude converges and an ordinary one ends APM_STATUS_MAXITER with NaN outputs."""
    c = case(ci)
    m = 65
    Xs, ys = c['Xs'][:m], c['ys'][:m]
    th3 = np.array([c['thetas'][0], c['thetas'][1], 0.5 * (c['thetas'][0] + c['thetas'][1])])
    sd3, ct3 = np.array([5, 6, 7], dtype=np.uint64), np.array([1, 0, 2], dtype=np.uint64)

    def call(ctx, order):
        out = ctx.predict_joint(approx(nat, c), th3[order], Xs, n_draws=S, seeds=sd3[order],
                                counters=ct3[order], want_draws=True, y_test=ys)
        return out[:4], out[4]

    ctx = context(nat, c)
    try:
        full, st = call(ctx, [0, 1, 2])
        assert list(st) == [0, 0, 0] and all(np.all(np.isfinite(o)) for o in full)
        rev, st = call(ctx, [2, 1, 0])
        assert list(st) == [0, 0, 0] and _same([o[::-1] for o in rev], full)
        for b in range(3):
            one, st = call(ctx, [b])
            assert list(st) == [0] and _same(one, [o[b:b + 1] for o in full]), b
    finally:
        ctx.close()

    easy = c['thetas'][0].copy()
    easy[0] = -16.0  # the first Newton step / second EP sweep moves the mode by less than the tol
    if c['cov'].flagged:
        easy[-2:] = -16.0  # (the constant and the linear term's amplitudes as well)
    thf = np.array([easy, c['thetas'][0], easy + 0.01])
    for th, few in zip(thf, (True, False, True)):  # the restatement's counts at these settings
        if c['fit'] == 'ep':
            n_it = jr.ep_state(c['cov'], c['X'], c['y'], th, EPS, lik=c['lik'],
                               quadrature=c['lik'] == 'logit', diff_tol=1e-8)['n_iter']
            assert (n_it == 2) == few, (th, n_it)
        else:
            n_it = jr.laplace_state(c['cov'], c['X'], c['y'], th, EPS, lik=c['lik'])['n_iter']
            assert (n_it == 1) == few, (th, n_it)
    ctx = context(nat, c)
    try:
        ctx.set_newton(1e-4, 1)
        if c['fit'] == 'ep':
            ctx.set_ep(0.8, 1e-8, 2)
        kw = dict(n_draws=S, seeds=sd3, counters=ct3, want_draws=True, y_test=ys)
        out = ctx.predict_joint(approx(nat, c), thf, Xs, **kw)
        assert list(out[4]) == [nat.STATUS_OK, nat.STATUS_MAXITER, nat.STATUS_OK]
        assert all(np.all(np.isnan(o[1])) for o in out[:4])
        assert all(np.all(np.isfinite(o[[0, 2]])) for o in out[:4])
        for b in (0, 2):
            one = ctx.predict_joint(approx(nat, c), thf[b:b + 1], Xs, n_draws=S,
                                    seeds=sd3[b:b + 1], counters=ct3[b:b + 1], want_draws=True,
                                    y_test=ys)
            assert list(one[4]) == [0] and _same(one[:4], [o[b:b + 1] for o in out[:4]]), b
    finally:
        ctx.close()


def _raw(ctx, approx, th, Xs, m, mean=None, cov=None, n_draws=0, seeds=None, counters=None,
         draws=None, ys=None, lpd=None, count=None, ldo=None, ldc=None):
    p = lambda a: None if a is None else a.ctypes.data
    count = th.shape[0] if count is None else count
    st = np.full(max(count, 1), -7, dtype=np.int32)
    rc = ctx.lib.apm_predict_joint(ctx._h, approx, count, p(th), th.shape[1], p(Xs), m, Xs.shape[1],
                                   p(mean), m if ldo is None else ldo, p(cov),
                                   m if ldc is None else ldc, n_draws, p(seeds), p(counters),
                                   p(draws), p(ys), p(lpd), p(st), None)
    return rc, st


def test_null_outputs_and_padded_strides(nat):
    """Every output may be NULL, alone and together, and what is asked for does not depend on
    what else is; row strides wider than m leave the caller's padding alone."""
    c = case(1)
    m, T = 65, 2
    Xs, ys, th = np.ascontiguousarray(c['Xs'][:m]), c['ys'][:m].copy(), c['thetas']
    sd, ct = np.array([9, 10], dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    ctx = context(nat, c)
    try:
        mean, cov, draws, lpd, st, _ = ctx.predict_joint(
            nat.JOINT_LAPLACE, th, Xs, n_draws=S, seeds=sd, want_draws=True, y_test=ys)
        assert list(st) == [0, 0]
        rc, st = _raw(ctx, nat.JOINT_LAPLACE, th, Xs, m)
        assert rc == 0 and list(st) == [0, 0]
        rc, st = _raw(ctx, nat.JOINT_LAPLACE, th, Xs, m, n_draws=S)  # (draws nobody asked for)
        assert rc == 0 and list(st) == [0, 0]
        for which in ('mean', 'cov', 'draws', 'lpd'):
            got = dict(mean=np.full((T, m), 5.0), cov=np.full((T, m, m), 5.0),
                       draws=np.full((T, S, m), 5.0), lpd=np.full(T, 5.0))[which]
            kw = {which: got}
            if which in ('draws', 'lpd'):
                kw.update(n_draws=S, seeds=sd, counters=ct)
            if which == 'lpd':
                kw.update(ys=ys)
            rc, st = _raw(ctx, nat.JOINT_LAPLACE, th, Xs, m, **kw)
            assert rc == 0 and list(st) == [0, 0], which
            assert np.array_equal(got, dict(mean=mean, cov=cov, draws=draws, lpd=lpd)[which]), which
        wm, wc = np.full((T, m + 3), 5.0), np.full((T, m, m + 2), 5.0)
        rc, st = _raw(ctx, nat.JOINT_LAPLACE, th, Xs, m, mean=wm, cov=wc, ldo=m + 3, ldc=m + 2)
        assert rc == 0 and np.array_equal(wm[:, :m], mean) and np.array_equal(wc[:, :, :m], cov)
        assert np.all(wm[:, m:] == 5.0) and np.all(wc[:, :, m:] == 5.0)
    finally:
        ctx.close()


def test_refusals(nat):
    """Every refusal of include/apm.h returns APM_E_INVALID and leaves the statuses alone."""
    c = case(1)
    th = c['thetas']
    ctx = context(nat, c, max_batch=2)
    np_ = ctx.padded_n
    assert np_ == 192
    Xbig = np.ascontiguousarray(np.tile(c['Xs'], (2, 1))[:np_ + 1])
    Xs, m = np.ascontiguousarray(c['Xs'][:5]), 5
    sd, ct = np.array([1, 2], dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    dr, lp, ys = np.empty((2, 4, m)), np.empty(2), c['ys'][:m].copy()
    L = nat.JOINT_LAPLACE
    try:
        bad = [
            _raw(ctx, 2, th, Xs, m),                                       # approx
            _raw(ctx, -1, th, Xs, m),
            _raw(ctx, L, np.tile(th, (2, 1))[:3], Xs, m),                  # count > max_batch
            _raw(ctx, L, th, Xs, m, count=0),
            _raw(ctx, L, th, Xs, 0),                                       # m
            _raw(ctx, L, th, Xbig, np_ + 1),
            _raw(ctx, L, th, Xs, m, n_draws=-1),                           # n_draws
            _raw(ctx, L, th, Xs, m, n_draws=nat.JOINT_MAX_DRAWS + 1, seeds=sd, counters=ct),
            _raw(ctx, L, th, Xs, m, n_draws=0, seeds=sd, counters=ct, draws=dr),
            _raw(ctx, L, th, Xs, m, n_draws=0, seeds=sd, counters=ct, ys=ys, lpd=lp),
            _raw(ctx, L, th, Xs, m, n_draws=4, draws=dr),                  # no seeds
            _raw(ctx, L, th, Xs, m, n_draws=4, seeds=sd, counters=ct, lpd=lp),  # no labels
            _raw(ctx, L, th, Xs, m, mean=np.empty((2, m)), ldo=m - 1),
            _raw(ctx, L, th, Xs, m, cov=np.empty((2, m, m)), ldc=m - 1),
            _raw(ctx, nat.JOINT_EP, th, Xs, m),                            # logit EP, no quadrature
        ]
        for i, (rc, st) in enumerate(bad):
            assert rc == nat.APM_E_INVALID and np.all(st == -7), i
        assert b'probit only' in ctx.lib.apm_last_error(ctx._h)
        rc, st = _raw(ctx, L, th, Xbig[:np_], np_)  # the largest block is accepted
        assert rc == 0 and list(st) == [0, 0]
        ctx.set_ep(0.8, 1e-8, 100, quadrature=True)
        rc, st = _raw(ctx, nat.JOINT_EP, th, Xs, m)
        assert rc == 0 and list(st) == [0, 0]
    finally:
        ctx.close()
    pre = nat.Context(None, c['y'], nat.KERNEL_PRECOMPUTED, EPS, 1)
    try:
        rc, st = _raw(pre, L, th, Xs, m)
        assert rc == nat.APM_E_INVALID and b'ISO or ARD' in pre.lib.apm_last_error(pre._h)
    finally:
        pre.close()


def _flat_theta(c):
    """Case 1's first theta with every length scale at e^10: the test points then differ by ~1e-8
    of a length scale, K** is s 1 1^T up to ~1e-8 and Sigma = K** - V V^T numerically has rank
    two or three."""
    flat = c['thetas'][0].copy()
    flat[1:] = 10.0
    return flat


def test_factor_failure_of_one_chain(nat):
    """At epsilon = 0 a theta with very long length scales makes its own chain's Sigma numerically
    rank-deficient (the restatement's Sigma has negative eigenvalues at rounding level, asserted
    here, so no factor of it exists), while its Laplace fit converges as any other: B = I +
    W^1/2 K W^1/2 is well conditioned whatever K's rank. That chain alone gets APM_STATUS_CHOL_C
    and NaN outputs; its neighbours of ordinary theta are bitwise what they are alone (count = 1),
    so the device's liveness gating behind the failed factor and the host's status merge leave
    them untouched. Without draws nothing is factored and all three chains are OK."""
    c = case(1)
    m = 65
    Xs, ys = np.ascontiguousarray(c['Xs'][:m]), c['ys'][:m]
    flat = _flat_theta(c)
    st = jr.laplace_state(c['cov'], c['X'], c['y'], flat, 0.0, tol=NEWTON_TOL, lik=c['lik'])
    ref = jr.at_test_inputs(c['cov'], c['X'], Xs, flat, st, 0.0)
    ev = np.linalg.eigvalsh(ref['cov'])
    assert (ev < 0).sum() >= 10 and ev[0] > -1e-12  # indefinite by rounding, nothing else
    with pytest.raises(np.linalg.LinAlgError):
        jr.cholesky_ld(ref['cov'])
    th3 = np.array([c['thetas'][0], flat, c['thetas'][1]])
    sd3, ct3 = np.array([5, 6, 7], dtype=np.uint64), np.array([1, 0, 2], dtype=np.uint64)
    ctx = context(nat, c, eps=0.0)
    try:
        kw = dict(n_draws=S, want_draws=True, y_test=ys)
        out = ctx.predict_joint(nat.JOINT_LAPLACE, th3, Xs, seeds=sd3, counters=ct3, **kw)
        assert list(out[4]) == [nat.STATUS_OK, nat.STATUS_CHOL_C, nat.STATUS_OK]
        assert out[5][1] == st['n_iter']  # (the fit itself converged)
        assert all(np.all(np.isnan(o[1])) for o in out[:4])
        assert all(np.all(np.isfinite(o[[0, 2]])) for o in out[:4])
        for b in (0, 2):
            one = ctx.predict_joint(nat.JOINT_LAPLACE, th3[b:b + 1], Xs, seeds=sd3[b:b + 1],
                                    counters=ct3[b:b + 1], **kw)
            assert list(one[4]) == [0] and _same(one[:4], [o[b:b + 1] for o in out[:4]]), b
        alone = ctx.predict_joint(nat.JOINT_LAPLACE, th3[1:2], Xs, seeds=sd3[1:2],
                                  counters=ct3[1:2], **kw)
        assert list(alone[4]) == [nat.STATUS_CHOL_C]
        mean, cov, _, _, st0, _ = ctx.predict_joint(nat.JOINT_LAPLACE, th3, Xs)
        assert list(st0) == [0, 0, 0] and np.all(np.isfinite(cov))
        assert _same([mean[[0, 2]], cov[[0, 2]]], [out[0][[0, 2]], out[1][[0, 2]]])
        assert np.abs(cov[1] - ref['cov']).max() <= TOL * max(1.0, np.abs(ref['cov']).max())
    finally:
        ctx.close()

    import gpdemo.kernels as krn
    import gpdemo.predict as prd
    from gpdemo.estimators import InvalidCovarianceMatrixError
    p = prd.LaplacePredictor(c['X'], c['y'], krn.make_kernel_func('ard', 0.0), Xs, max_batch=3,
                             likelihood='logit', diff_f_tol=NEWTON_TOL)
    try:
        d = p.sample_latent(th3, 16, seed=[5, 6, 7], on_error='nan')
        assert list(p.status) == [nat.STATUS_OK, nat.STATUS_CHOL_C, nat.STATUS_OK]
        assert np.all(np.isnan(d[1])) and np.all(np.isfinite(d[[0, 2]]))
        lp = p.joint_log_predictive_density(th3[[0, 2]], ys, 16, seed=[5, 7])
        assert math.isfinite(lp)
        with pytest.raises(InvalidCovarianceMatrixError):
            p.sample_latent(th3, 16, seed=[5, 6, 7])
    finally:
        p.close()


def test_more_draws_after_fewer(nat):
    """The draw buffers grow with the largest n_draws a context has seen: a call with more draws
    after one with fewer (the buffers are released and allocated again), and one that wants the
    draws back after one that did not, return bitwise what a fresh context returns."""
    c = case(0)
    m = 65
    Xs, ys, th = c['Xs'][:m], c['ys'][:m], c['thetas']
    sd = np.array([8, 9], dtype=np.uint64)

    def call(ctx, n_draws, want_draws):
        out = ctx.predict_joint(nat.JOINT_LAPLACE, th, Xs, n_draws=n_draws, seeds=sd,
                                want_draws=want_draws, y_test=ys)
        assert list(out[4]) == [0, 0]
        return out[:4]

    ctx = context(nat, c)
    try:
        small = call(ctx, 40, False)          # 64 rows of normals, no draw buffer yet
        big = call(ctx, 200, True)            # 256 rows: both buffers anew
        small_again = call(ctx, 40, True)     # fewer again, in the larger buffers
        assert _same([small[0], small[1], small[3]], [small_again[0], small_again[1],
                                                      small_again[3]])
    finally:
        ctx.close()
    fresh = context(nat, c)
    try:
        assert _same(call(fresh, 200, True), big)
        assert _same(call(fresh, 40, True), small_again)
    finally:
        fresh.close()


def test_duplicated_test_point_without_jitter(nat):
    """At epsilon = 0 a test point repeated twelve times makes Sigma singular: after the first
    copy's column the other copies' pivots are differences of equal numbers at rounding level, one
    of which is not positive, so the factor fails and the chain gets APM_STATUS_CHOL_C, its outputs
    NaN. The status belongs to the factor alone: the same call without draws is OK and returns the
    singular Sigma, and the same context is OK again at distinct points. The test inputs are one
    block shared by the chains of a call, so a duplicate is every chain's; one failing chain
    beside OK ones is test_factor_failure_of_one_chain."""
    c = case(1)
    m = 65
    Xs = np.ascontiguousarray(c['Xs'][:m])
    Xd = Xs.copy()
    Xd[40:52] = Xd[40]
    th, sd = c['thetas'], np.array([3, 4], dtype=np.uint64)
    ctx = context(nat, c, eps=0.0)
    try:
        mean, cov, draws, lpd, st, _ = ctx.predict_joint(nat.JOINT_LAPLACE, th, Xd, n_draws=8,
                                                         seeds=sd, want_draws=True,
                                                         y_test=c['ys'][:m])
        assert list(st) == [nat.STATUS_CHOL_C] * 2
        assert all(np.all(np.isnan(o)) for o in (mean, cov, draws, lpd))
        mean, cov, _, _, st, _ = ctx.predict_joint(nat.JOINT_LAPLACE, th, Xd)
        assert list(st) == [0, 0] and np.all(np.isfinite(cov))
        assert np.array_equal(cov[:, 40], cov[:, 51]) and np.array_equal(mean[:, 40], mean[:, 51])
        out = ctx.predict_joint(nat.JOINT_LAPLACE, th, Xs, n_draws=8, seeds=sd, want_draws=True)
        assert list(out[4]) == [0, 0] and np.all(np.isfinite(out[2]))
    finally:
        ctx.close()


def test_python_layer(nat):
    """LaplacePredictor / EPPredictor: shapes, the same seeds give the same draws and other
    seeds others, the draws' mean is near the latent mean, the density over thetas is the log
    mean of the per-theta densities, and a failing factor raises InvalidCovarianceMatrixError."""
    import gpdemo.kernels as krn
    import gpdemo.predict as prd
    from gpdemo.estimators import InvalidCovarianceMatrixError
    c = case(0)
    m, T = 64, 3
    Xs, ys = c['Xs'][:m], c['ys'][:m]
    th = np.array([c['thetas'][0], c['thetas'][1], c['thetas'][0] + 0.1])
    kf = krn.make_kernel_func('iso', EPS)
    for cls in (prd.LaplacePredictor, prd.EPPredictor):
        p = cls(c['X'], c['y'], kf, Xs, max_batch=2)  # (three thetas: two device calls)
        try:
            mean, cov = p.joint(th)
            assert mean.shape == (T, m) and cov.shape == (T, m, m)
            assert np.array_equal(mean, p(th)[0]) and np.array_equal(cov, cov.transpose(0, 2, 1))
            d1 = p.sample_latent(th, 256, seed=11)
            assert d1.shape == (T, 256, m) and np.all(np.isfinite(d1))
            assert np.array_equal(d1, p.sample_latent(th, 256, seed=[11, 12, 13]))
            assert not np.array_equal(d1, p.sample_latent(th, 256, seed=12))
            assert np.array_equal(d1[0], p.sample_latent(th[0], 256, seed=11)[0])
            se = np.sqrt(np.einsum('tjj->tj', cov) / 256)
            assert np.all(np.abs(d1.mean(1) - mean) <= 5.0 * se)
            one = [p.joint_log_predictive_density(th[t], ys, 256, seed=20 + t) for t in range(T)]
            both = p.joint_log_predictive_density(th, ys, 256, seed=20)
            top = max(one)
            assert abs(both - (top + math.log(np.mean(np.exp(np.array(one) - top))))) <= 1e-12
            assert abs(p.joint_log_predictive_density(th, ys, 256, seed=[21, 22], burn=1)
                       - (max(one[1:]) + math.log(np.mean(np.exp(np.array(one[1:]) - max(one[1:]))))
                          )) <= 1e-12
            assert p.status.shape == (2,)
        finally:
            p.close()
    Xd = Xs.copy()
    Xd[10:22] = Xd[10]
    p = prd.LaplacePredictor(c['X'], c['y'], krn.make_kernel_func('iso', 0.0), Xd)
    try:
        with pytest.raises(InvalidCovarianceMatrixError):
            p.sample_latent(th[0], 4, seed=1)
        assert np.all(np.isnan(p.sample_latent(th[0], 4, seed=1, on_error='nan')))
        assert list(p.status) == [nat.STATUS_CHOL_C]
    finally:
        p.close()
