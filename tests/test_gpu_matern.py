"""Matérn 3/2 and 5/2 covariance kinds (iso and ARD) on the device: Gram and
cross-Gram, the three estimators' theta-calls, the Laplace predictive distribution, the gradient
of the Laplace log marginal likelihood, batch neutrality and a batched sampler, against the numpy
restatement of tests/cov_restatement.py (the oracle's C Gram knows the SE family only) and
the oracle's estimators run with the restatement's kernel_func."""
import math

import numpy as np
import pytest
import scipy.linalg as la
from scipy.special import ndtr

import apm_oracle as orc
import cov_checks as cc
import cov_restatement as cr
import grad_restatement as gr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = 1e-8
TOL_NATS = 5e-4        # estimator values, no relative term: test_gpu_kernels.py
TOL = 1e-9             # fp64 against fp64 through the same factorisation: test_gpu_predict / _grad
NEWTON_TOL = 1e-14     # the gradient's Newton tolerance
FAR = 1000.0  # the far test row: k* underflows to exactly 0
FAMILY_KINDS = [(f, k) for f in cr.MATERN for k in ('iso', 'ard')]
# (family, n, d, kind) -> data seed, chosen so that for all three thetas (theta_0 = 0.3, 3.0,
# -1.0) the restatement's last Newton `diff` is at least 100x below the tolerance and the one
# before at least 100x above it at the gradient's 1e-14 (at n = 1, where the data cannot change the
# Newton path, 1.5x: test_gpu_grad.test_newton_margins), and a factor 3 on both sides of the
# estimators' and the predictor's 1e-4, where consecutive diffs are only ~1e3 apart: device and
# restatement then cannot disagree on an iteration count (diff's own relative error is ~1e-9).
# The gradient test asserts the 1e-14 margins on the CPU before it compares.
SEEDS = {
    '32': {(1, 1, 'ard'): 800, (64, 33, 'ard'): 908, (130, 5, 'ard'): 804, (200, 3, 'iso'): 991,
           (600, 4, 'ard'): 802},
    '52': {(1, 1, 'ard'): 800, (64, 33, 'ard'): 898, (130, 5, 'ard'): 804, (200, 3, 'iso'): 1130,
           (600, 4, 'ard'): 802},
}
GRAD_SHAPES = [(1, 1, 'ard'), (64, 33, 'ard'), (130, 5, 'ard'), (200, 3, 'iso'), (600, 4, 'ard')]
PREDICT_SHAPES = [(130, 5, 70, 'ard'), (64, 33, 64, 'ard'), (600, 4, 70, 'ard')]


def _name(family, kind):
    return 'matern{0}_{1}'.format(family, kind)


def _native_kind(nat, family, kind):
    return {('32', 'iso'): nat.KERNEL_M32_ISO, ('32', 'ard'): nat.KERNEL_M32_ARD,
            ('52', 'iso'): nat.KERNEL_M52_ISO, ('52', 'ard'): nat.KERNEL_M52_ARD}[family, kind]


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


_CASES = {}


def _case(family, n, d, kind):
    """Data of one (family, shape), drawn once (grad_restatement.make_case) and left unchanged."""
    key = (family, n, d, kind)
    if key not in _CASES:
        _CASES[key] = gr.make_case(n, d, kind, SEEDS[family][n, d, kind])
    return _CASES[key]


# ------------------------------------------------------------------ 1. Gram and cross-Gram


def _check_gram(K, Kref, bound, what):
    """|K - Kref| <= bound entry by entry; returns the largest error as a fraction of it."""
    err = np.abs(K - Kref)
    frac = float((err / bound).max())
    print('matern gram {0}: max error / bound = {1:.3f}'.format(what, frac))
    assert np.all(err <= bound), (what, frac)
    return frac


def _gram_inputs(n, d, kind, near_duplicates):
    if near_duplicates:  # the construction of test_gram_near_duplicate_rows_vs_c_oracle
        rng = np.random.RandomState(11)
        base = rng.normal(size=(n // 2, d))
        X = np.concatenate([base, base + 1e-4 * rng.normal(size=base.shape)])[rng.permutation(n)]
        X = np.concatenate([X, 3.0 + 0.01 * rng.normal(size=(n % 2, d))]) if n % 2 else X
        th = np.r_[0.2, rng.normal(scale=0.5, size=d if kind == 'ard' else 1)]
    else:
        rng = np.random.RandomState(5 + n)
        X = rng.normal(size=(n, d))
        th = np.r_[0.3, rng.normal(size=d if kind == 'ard' else 1)]
    return X, th


GRAM_SHAPES = ([(n, d, kind, False) for n, d in ((1, 1), (129, 64), (300, 7))
                for kind in ('iso', 'ard')] +
               [(130, 6, 'iso', True), (200, 3, 'ard', True), (150, 40, 'ard', True)])


@pytest.mark.parametrize('family', cr.MATERN)
@pytest.mark.parametrize('n,d,kind,dup', GRAM_SHAPES)
def test_gram_vs_restatement(nat, family, n, d, kind, dup):
    """Entry by entry within the bound derived from the arithmetic (Cov.gram_bound; u = 2^-53):
    delta(r^2) = 4u sum_k (|a_k| + |c_k|)|a_k - c_k| + (D + 2) u r^2, |K - Kref| <= |Kref| (8u +
    2 delta(r^2)). K is exactly symmetric and its diagonal is exp(theta_0) + eps within 2 ulp.
    Measured maximum over all cases: see DESIGN.md §14."""
    import gpdemo.kernels as krn
    X, th = _gram_inputs(n, d, kind, dup)
    K = np.full((n, n), np.nan)
    krn.make_kernel_func(_name(family, kind), EPS)(K, X, th)
    Kref = Cov(family, kind).gram(X, th, EPS)
    _check_gram(K, Kref, Cov(family, kind).gram_bound(X, X, th, Kref), (family, n, d, kind, dup))
    assert np.array_equal(K, K.T)
    dg = math.exp(th[0]) + EPS
    assert np.all(np.abs(K.diagonal() - dg) <= 2 * np.spacing(dg))
    # the same entry point by its reference-style name, and a too-short theta
    fn = getattr(krn, '{0}_matern{1}_kernel'.format('isotropic' if kind == 'iso' else 'diagonal',
                                                    family))
    K2 = np.empty((n, n))
    fn(K2, X, th, EPS)
    assert np.array_equal(K2, K)
    with pytest.raises(IndexError):
        fn(K2, X, th[:-1], EPS)


@pytest.mark.parametrize('family,kind', FAMILY_KINDS)
@pytest.mark.parametrize('m,n,d', [(70, 130, 5), (1, 129, 40)])
def test_gram_cross_vs_restatement(nat, family, kind, m, n, d):
    """The same bound for k(Xs_i, X_j); no epsilon where a test point coincides with a training
    point (sigma exactly: s comes from the host's exp in k*)."""
    rng = np.random.RandomState(m + n)
    X, Xs = rng.normal(size=(n, d)), rng.normal(size=(m, d))
    Xs[0] = X[7]
    th = np.r_[0.3, 0.5 * math.log(d) + rng.uniform(-0.3, 0.1, size=d if kind == 'ard' else 1)]
    Ks = nat.gram_cross(_native_kind(nat, family, kind), Xs, X, th)
    assert Ks.shape == (m, n)
    ref = Cov(family, kind).gram_cross(Xs, X, th)
    _check_gram(Ks, ref, Cov(family, kind).gram_bound(Xs, X, th, ref), (family, kind, m, n, d))
    assert Ks[0, 7] == math.exp(th[0])


# ------------------------------------------------------------------ 2. theta-calls


@pytest.mark.parametrize('family,kind', FAMILY_KINDS)
def test_estimators_vs_oracle(nat, family, kind):
    """IS (theta-call and one cached u-call), PriorMC and Laplace estimates of a context of each
    new kind - ARD at (130, 5), iso at (200, 3) - against the oracle's three estimators with the
    restatement's kernel_func: 5e-4 nats, status 0, the oracle's n_cubic_ops."""
    n, d = (130, 5) if kind == 'ard' else (200, 3)
    c = _case(family, n, d, kind)
    X, y = c['X'], c['y']
    kf = Cov(family, kind).kernel_func(EPS)
    rng = np.random.RandomState(17)
    ns1, ns2 = rng.normal(size=(n, 8)), rng.normal(size=(n, 8))
    ctx = nat.Context(X, y, _native_kind(nat, family, kind), EPS, 8, max_batch=1, n_slots=2,
                      n_ubufs=2)
    ctx.u_upload(0, ns1)
    ctx.u_upload(1, ns2)
    for th in c['thetas']:
        r1, rc, rops = orc.is_estimate(X, y, kf, ns1, th)
        r2, _, _ = orc.is_estimate(X, y, kf, ns2, None, rc)
        p1, _, pops = orc.priormc_estimate(X, y, kf, ns1, th)
        lml, lops = orc.laplace_estimate(X, y, kf, th)
        out, st, nops = ctx.theta_eval(nat.EST_IS, th[None], [0], [0])
        out2, st2 = ctx.u_eval([0], [1])
        pm, pst, pnops = ctx.theta_eval(nat.EST_PRIORMC, th[None], [0], [1])
        lp, lst, lnops = ctx.theta_eval(nat.EST_LAPLACE, th[None])
        print('matern {0} {1} theta_0 {2}: IS {3:.2e} u-call {4:.2e} PriorMC {5:.2e} Laplace '
              '{6:.2e} nats'.format(family, kind, th[0], abs(out[0] - r1), abs(out2[0] - r2),
                                    abs(pm[0] - p1), abs(lp[0] - lml)))
        assert st[0] == 0 and st2[0] == 0 and pst[0] == 0 and lst[0] == 0
        assert nops[0] == rops and pnops[0] == pops and lnops[0] == lops
        assert abs(out[0] - r1) <= TOL_NATS
        assert abs(out2[0] - r2) <= TOL_NATS
        assert abs(pm[0] - p1) <= TOL_NATS
        assert abs(lp[0] - lml) <= TOL_NATS
    ctx.close()


# ------------------------------------------------------------------ 3. prediction


def _predict_restatement(family, kind, c, Xs, th):
    """gr.newton at the predictor's default tolerance, then the predictive from the last
    iteration's W, L, a: mu = Ks a, var = s - |L^-1 (W^1/2 . ks)|^2, Phi(mu / sqrt(1 + var))."""
    nw = gr.newton(Cov(family, kind).gram(c['X'], th, EPS), c['y'], 1e-4)
    Ks = Cov(family, kind).gram_cross(Xs, c['X'], th)
    mu = Ks.dot(nw['a'])
    V = la.solve_triangular(nw['L'], (Ks * nw['Ws'][None, :]).T, lower=True)
    var = math.exp(th[0]) - (V * V).sum(0)
    return dict(mean=mu, var=var, prob=ndtr(mu / np.sqrt(1.0 + var)), n_iter=nw['n_iter'])


@pytest.mark.parametrize('family', cr.MATERN)
@pytest.mark.parametrize('n,d,m,kind', PREDICT_SHAPES)
def test_predict_vs_restatement(nat, family, n, d, m, kind):
    """mean and var relative to max(1, max|ref|), prob absolute, at 1e-9 (test_gpu_predict's
    tolerance); equal Newton iteration counts; the far test point returns bitwise the prior.
    (600, 4, 70) has two outer panels: its test rows take the trailing update."""
    import gpdemo.kernels as krn
    import gpdemo.predict as prd
    c = _case(family, n, d, kind)
    Xs = cc.far_test_inputs(c, m, FAR)
    p = prd.LaplacePredictor(c['X'], c['y'], krn.make_kernel_func(_name(family, kind), EPS), Xs)
    mean, var, prob = p(c['thetas'])
    nit = p.n_iter.copy()
    p.close()
    worst = 0.0
    for t, th in enumerate(c['thetas']):
        ref = _predict_restatement(family, kind, c, Xs, th)
        assert int(nit[t]) == ref['n_iter']
        for key, dev in (('mean', mean), ('var', var), ('prob', prob)):
            scale = 1.0 if key == 'prob' else max(1.0, np.abs(ref[key]).max())
            worst = max(worst, np.abs(dev[t] - ref[key]).max() / scale)
        assert mean[t, -1] == 0.0 and prob[t, -1] == 0.5
        assert var[t, -1] == math.exp(th[0])  # bitwise the caller's exp(theta_0)
        assert np.all(var[t] > 0.0) and np.all(var[t] <= math.exp(th[0]))
    print('matern predict parity {0}: worst {1:.3e} (tol {2:.0e})'
          .format((family, n, d, m, kind), worst, TOL))
    assert worst <= TOL


# ------------------------------------------------------------------ 4. gradient


@pytest.fixture(scope='module')
def grad_refs():
    """Restatement results per (family, shape), computed once on first use."""
    cache = {}

    def get(family, n, d, kind):
        key = (family, n, d, kind)
        if key not in cache:
            c = _case(family, n, d, kind)
            cache[key] = [cr.laplace_grad(Cov(family, kind), c['X'], c['y'], th, EPS, tol=NEWTON_TOL)
                          for th in c['thetas']]
        return cache[key]
    return get


@pytest.mark.parametrize('family', cr.MATERN)
@pytest.mark.parametrize('n,d,kind', GRAD_SHAPES)
def test_grad_vs_restatement_and_central_differences(nat, grad_refs, family, n, d, kind):
    """lml and grad against the restatement at 1e-9 of max(1, max|ref grad|) with equal Newton
    iteration counts (the seeds' margins are asserted first, on the CPU); grad against central
    differences (h = 1e-5) of the restatement's converged LML at 1e-6 of max(1, max|fd|); lml
    bitwise the Laplace theta-call's at the same Newton settings."""
    import gpdemo.gradients as gd
    import gpdemo.kernels as krn
    c = _case(family, n, d, kind)
    refs = grad_refs(family, n, d, kind)
    for ref in refs:
        last, prev = ref['diffs'][-1], ref['diffs'][-2]
        assert last <= NEWTON_TOL / 100.0
        assert prev >= (1.5 if n == 1 else 100.0) * NEWTON_TOL
    p = gd.LaplaceGradient(c['X'], c['y'], krn.make_kernel_func(_name(family, kind), EPS))
    lml, grad = p(c['thetas'])
    nit = p.n_iter.copy()
    p.close()
    ctx = nat.Context(c['X'], c['y'], _native_kind(nat, family, kind), EPS, 1, max_batch=4,
                      n_slots=1, n_ubufs=1)
    ctx.set_newton(NEWTON_TOL, 1000)
    val, st, nops = ctx.theta_eval(nat.EST_LAPLACE, c['thetas'])
    ctx.close()
    assert list(st) == [0, 0, 0]
    assert np.array_equal(val, lml) and np.array_equal(nops, nit)
    worst = worst_fd = 0.0
    for t, (th, ref) in enumerate(zip(c['thetas'], refs)):
        assert int(nit[t]) == ref['n_iter']
        scale = max(1.0, np.abs(ref['grad']).max())
        err = max(abs(lml[t] - ref['lml']), np.abs(grad[t] - ref['grad']).max()) / scale
        fd = gr.central_differences(
            lambda x: cr.lml(Cov(family, kind), c['X'], c['y'], x, EPS, tol=1e-24), th)
        err_fd = np.abs(grad[t] - fd).max() / max(1.0, np.abs(fd).max())
        worst, worst_fd = max(worst, err), max(worst_fd, err_fd)
        print('matern grad parity {0} theta {1}: {2:.3e}, vs fd {3:.3e} (max|grad| {4:.3e})'
              .format((family, n, d, kind), t, err, err_fd, np.abs(ref['grad']).max()))
    print('matern grad parity {0}: worst {1:.3e} (tol {2:.0e}), vs fd {3:.3e} (tol 1e-06)'
          .format((family, n, d, kind), worst, TOL, worst_fd))
    if n == 1:  # one point: every length-scale derivative has a zero diagonal
        assert np.all(grad[:, 1:] == 0.0) and np.all(grad[:, 0] != 0.0)
    assert worst <= TOL
    assert worst_fd <= 1e-6


# ------------------------------------------------------------------ 5. batch neutrality


def test_batches_are_bitwise_neutral(nat):
    """One Matérn 5/2 ARD context (130, 5), max_batch = 8: a chain's gradient and predictive
    outputs are bitwise the same alone, first of 3 and last of 8."""
    c = _case('52', 130, 5, 'ard')
    Xs = cc.far_test_inputs(c, 70, FAR)
    rng = np.random.RandomState(5)
    other = c['thetas'][rng.randint(0, 3, size=7)] + rng.uniform(-0.2, 0.2, size=(7, 6))
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_M52_ARD, EPS, 1, max_batch=8, n_slots=1,
                      n_ubufs=1)
    for tol in (NEWTON_TOL, 1e-4):
        ctx.set_newton(tol, 1000)
        for th in c['thetas']:
            first_th, last_th = np.vstack([th[None], other[:2]]), np.vstack([other, th[None]])
            alone, first, last = (ctx.laplace_grad(x) for x in (th, first_th, last_th))
            assert alone[2][0] == 0 and np.all(np.isfinite(alone[1]))
            for got, i in ((first, 0), (last, 7)):
                assert got[0][i] == alone[0][0] and np.array_equal(got[1][i], alone[1][0])
                assert got[3][i] == alone[3][0]
            alone, first, last = (ctx.predict(x, Xs) for x in (th, first_th, last_th))
            assert alone[3][0] == 0 and all(np.all(np.isfinite(a)) for a in alone[:3])
            for got, i in ((first, 0), (last, 7)):
                for k in range(3):
                    assert np.array_equal(got[k][i], alone[k][0])
                assert got[4][i] == alone[4][0]
    ctx.close()


# ------------------------------------------------------------------ 6. batched sampler


def test_batched_ess_mh_matern52_ard(nat):
    """kernel='matern52_ard' at n = 130, 3 chains, 3 iterations of E-SS(u) + MH(theta): chain 0's
    trajectory is bitwise the same alone and in the batch, and every chain's current state (cache
    slot, u, log f) is consistent with the oracle's IS estimate on the same (theta, fp32 u) at
    5e-4 nats (the pattern of test_batched_ess_mh_consistent_and_batch_invariant)."""
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler
    from gpdemo.utils import synthetic_gp_data
    n, d = 130, 4
    X, y = synthetic_gp_data(n, d, 5)
    prior = dict(a_tau=1., b_tau=1. / d ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(d, np.log(2.))], (3, 1))
    smp = BatchedAPMEllSSPlusMHSampler(X, y, 3, 16, prior, prop_scales=0.1, seed=31,
                                       kernel='matern52_ard')
    assert smp.ctx.kind == nat.KERNEL_M52_ARD
    th, nrej = smp.get_samples(4, th0)  # the start state and 3 iterations
    assert np.isfinite(th).all() and not smp.failed.any()
    kf = Cov('52', 'ard').kernel_func(EPS)
    for ch in range(3):
        lp = smp.log_prior(smp.theta[ch][None])[0]
        out, st = smp.ctx.u_eval([smp.slot_cur[ch]], [smp.ub_u[ch]])
        assert st[0] == 0 and abs(out[0] + lp - smp.log_f[ch]) < 1e-9 * max(1, abs(out[0]))
        v, _, _ = orc.is_estimate(X, y, kf, smp.ctx.u_download(smp.ub_u[ch]), smp.theta[ch])
        assert abs(smp.log_f[ch] - (v + lp)) <= TOL_NATS, (ch, smp.log_f[ch], v + lp)
    one = BatchedAPMEllSSPlusMHSampler(X, y, 1, 16, prior, prop_scales=0.1, seed=31,
                                       kernel='matern52_ard', first_chain=0)
    th1, nrej1 = one.get_samples(4, th0[:1])
    np.testing.assert_array_equal(th1[0], th[0])
    assert nrej1[0] == nrej[0]
    # the SE sampler on the same data and streams takes another path: the kernel name is read
    se = BatchedAPMEllSSPlusMHSampler(X, y, 1, 16, prior, prop_scales=0.1, seed=31)
    assert se.ctx.kind == nat.KERNEL_ARD
    se.initialise(th0[:1])
    assert se.log_f[0] != one.log_f[0] or not np.array_equal(se.theta, one.theta)
