"""Predictive, gradient and apm_laplace's covariance at the panel boundaries of the fp64 schedule's
solve-only form (host_chol64.cpp chol_solve_rows, row_start = nb), which predict_block, grad_block
and augmented() run the work matrix through: N = 65, 128, 512, 513, 1024, 1025, 1089 (nb = 2, 2,
8, 9, 16, 17, 18; tests/edge_cases.py says what each size reaches), test-row counts mb = 1, 2, 3,
nb and a second block of one row, against the numpy/scipy restatements (grad_restatement,
cov_restatement, predict_restatement) and the oracle's laplace_approximation. Then the order
of calls on one context (predict and gradient write the bottom rows of the work matrix the IS
theta-call also uses) and the reuse of apm_laplace's cached context.

Tolerances are the suite's own: 1e-9 for fp64 against fp64 through the same factorisation
 and the golden Laplace test's for f, C and lml. The seeds of the inputs
keep device and restatement from disagreeing on a Newton iteration count
(test_grad_host.test_edge_case_seeds_keep_their_newton_margins asserts it without a device)."""
import math

import numpy as np
import pytest

import apm_oracle as orc
import edge_cases as ec
import cov_restatement as cr
import grad_restatement as gr
import predict_restatement as pr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = ec.EPS
TOL = 1e-9
CASES = [(None, 'ard', n) for n in ec.SIZES] + sorted(ec.MATERN)
PREDICT_CASES = ([(None, 'ard', n, m) for n in ec.SIZES for m in ec.PREDICT_M[n]] +
                 [('52', 'ard', 513, 70)])


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _native_kind(nat, family, kind):
    return {(None, 'ard'): nat.KERNEL_ARD, ('32', 'iso'): nat.KERNEL_M32_ISO,
            ('52', 'ard'): nat.KERNEL_M52_ARD}[family, kind]


def _context(nat, c, **kw):
    return nat.Context(c['X'], c['y'], _native_kind(nat, c['family'], c['kind']), EPS, 1,
                       max_batch=len(c['thetas']), n_slots=1, n_ubufs=1, **kw)


# ----------------------------------------------------------------------------- restatements

_GRAD_REF, _FIT_REF, _PRED_DEV = {}, {}, {}


def _grad_ref(family, kind, n):
    """The gradient restatement per theta of a case, computed once and left unchanged."""
    key = (family, kind, n)
    if key not in _GRAD_REF:
        c = ec.case(n, family, kind)
        _GRAD_REF[key] = [cr.laplace_grad(ec.cov(c), c['X'], c['y'], th, EPS, tol=ec.GRAD_TOL)
                          for th in c['thetas']]
    return _GRAD_REF[key]


def _fit_ref(family, kind, n):
    """The Newton state (L, W^1/2, a, n_iter) at the predictor's tolerance per theta, once."""
    key = (family, kind, n)
    if key not in _FIT_REF:
        c = ec.case(n, family, kind)
        _FIT_REF[key] = [gr.newton(ec.gram(c, th), c['y'], ec.FIT_TOL) for th in c['thetas']]
    return _FIT_REF[key]


# ----------------------------------------------------------------------------- B. gradient

@pytest.mark.parametrize('family,kind,n', CASES)
def test_grad_at_panel_edges(nat, family, kind, n):
    """lml and grad against the restatement at 1e-9 of max(1, max|ref grad|) with equal Newton
    iteration counts; lml bitwise the Laplace theta-call's at the same Newton settings. Measured
    maxima per size: DESIGN.md §13."""
    c = ec.case(n, family, kind)
    refs = _grad_ref(family, kind, n)
    for ref in refs:  # (of the inputs, not of the device)
        assert ec.margins_hold(ref['diffs'])
    ctx = _context(nat, c)
    ctx.set_newton(ec.GRAD_TOL, 1000)
    lml, grad, st, nit = ctx.laplace_grad(c['thetas'])
    val, lst, nops = ctx.theta_eval(nat.EST_LAPLACE, c['thetas'])
    ctx.close()
    assert not st.any() and not lst.any()
    worst = 0.0
    for t, ref in enumerate(refs):
        assert int(nit[t]) == ref['n_iter']
        scale = max(1.0, np.abs(ref['grad']).max())
        err = max(abs(lml[t] - ref['lml']), np.abs(grad[t] - ref['grad']).max()) / scale
        worst = max(worst, err)
        print('edge grad parity {0} theta {1}: {2:.3e} (max|grad| {3:.3e}, {4} iterations)'
              .format((family, kind, n), t, err, np.abs(ref['grad']).max(), ref['n_iter']))
    print('edge grad parity {0}: worst {1:.3e} (tol {2:.0e})'.format((family, kind, n), worst, TOL))
    assert worst <= TOL
    assert np.array_equal(val, lml) and np.array_equal(nops, nit)


# ----------------------------------------------------------------------------- C. predictive

def _shift(family):
    return 50.0 if family is None else 1000.0


def _device_predict(nat, family, kind, n, m):
    """(mean, var, prob, status, n_iter) of one predict call on a fresh context, once per case."""
    key = (family, kind, n, m)
    if key not in _PRED_DEV:
        c = ec.case(n, family, kind)
        ctx = _context(nat, c)
        ctx.set_newton(ec.FIT_TOL, 1000)
        _PRED_DEV[key] = ctx.predict(c['thetas'], ec.predict_inputs(c, m, _shift(family)))
        ctx.close()
    return _PRED_DEV[key]


@pytest.mark.parametrize('family,kind,n,m', PREDICT_CASES)
def test_predict_at_panel_edges(nat, family, kind, n, m):
    """mean and var relative to max(1, max|ref|), prob absolute, at 1e-9; equal Newton iteration
    counts; the far rows bitwise the prior (0, exp(theta_0), 0.5); 0 < var <= exp(theta_0).
    Measured maxima per size: DESIGN.md §12."""
    c = ec.case(n, family, kind)
    Xs = ec.predict_inputs(c, m, _shift(family))
    assert Xs.shape == (m, ec.D)
    far = [] if m < 3 else ([m - 2, m - 1] if m == 577 else [m - 1])
    mean, var, prob, st, nit = _device_predict(nat, family, kind, n, m)
    assert not st.any()
    worst = 0.0
    for t, (th, nw) in enumerate(zip(c['thetas'], _fit_ref(family, kind, n))):
        sigma = math.exp(th[0])
        Ks = ec.gram_cross(c, Xs, th)
        if m >= 3:  # (of the inputs: the coinciding row carries no epsilon, the far rows are 0)
            assert Ks[0, ec.I_EQ] == sigma and not Ks[far].any()
        ref = pr.at_test_inputs(Ks, sigma, nw['L'], nw['Ws'], nw['a'])
        assert int(nit[t]) == nw['n_iter']
        for key, dev in (('mean', mean), ('var', var), ('prob', prob)):
            scale = 1.0 if key == 'prob' else max(1.0, np.abs(ref[key]).max())
            err = np.abs(dev[t] - ref[key]).max() / scale
            worst = max(worst, err)
            print('edge predict parity {0} theta {1} {2}: {3:.3e}'
                  .format((family, kind, n, m), t, key, err))
        for r in far:
            assert mean[t, r] == 0.0 and var[t, r] == sigma and prob[t, r] == 0.5
        assert np.all(var[t] > 0.0) and np.all(var[t] <= sigma)
    print('edge predict parity {0}: worst {1:.3e} (tol {2:.0e})'
          .format((family, kind, n, m), worst, TOL))
    assert worst <= TOL


def test_second_block_of_one_row_is_a_one_row_call(nat):
    """N = 513 (np = 576): the m = 577 result is bitwise the m = 576 result and a call with the
    last row alone."""
    c = ec.case(513)
    full = _device_predict(nat, None, 'ard', 513, 577)
    head = _device_predict(nat, None, 'ard', 513, 576)
    ctx = _context(nat, c)
    ctx.set_newton(ec.FIT_TOL, 1000)
    tail = ctx.predict(c['thetas'], ec.predict_inputs(c, 577)[576:])
    ctx.close()
    assert not full[3].any() and not head[3].any() and not tail[3].any()
    for k in range(3):
        assert np.array_equal(full[k], np.concatenate([head[k], tail[k]], axis=1))
    assert np.array_equal(full[4], head[4]) and np.array_equal(full[4], tail[4])


# ----------------------------------------------------------------------------- D. apm_laplace

@pytest.mark.parametrize('n', ec.COV_SIZES)
def test_laplace_covariance_beyond_one_panel(nat, n):
    """apm_laplace(calc_cov=1) against the oracle's laplace_approximation with K from the C
    oracle's Gram: test_laplace_vs_golden's checks and bounds, and C exactly symmetric. The
    entrywise bound on C = K - V^T V is usable at these inputs: the oracle's C and C_chol C_chol^T
    of theta_state_pushthrough, two fp64 routes, differ by at most 5.2e-4 of it (9.8e-15 of
    max|C|)."""
    c = ec.case(n)
    for t, th in enumerate(c['thetas'][:2]):
        K = ec.gram(c, th)
        rf, rC, rlml, rops = orc.laplace_approximation(K, c['y'], calc_cov=True, calc_lml=True)
        f, C, lml, nit, st = nat.laplace(K, c['y'], True, True, ec.FIT_TOL, 1000)
        assert st == 0
        assert nit + 1 == rops
        dC = np.abs(C - rC)
        print('edge laplace n = {0} theta {1}: max|df|/max|f| {2:.3e}, |dlml| {3:.3e}, max|dC|/'
              'max|C| {4:.3e}, max |dC| / (1e-10 + 1e-8 |C|) {5:.3e}'
              .format(n, t, np.abs(f - rf).max() / np.abs(rf).max(), abs(lml - rlml),
                      dC.max() / np.abs(rC).max(), (dC / (1e-10 + 1e-8 * np.abs(rC))).max()))
        np.testing.assert_allclose(f, rf, rtol=1e-9, atol=1e-11)
        assert abs(lml - rlml) <= 1e-8 * max(1.0, abs(rlml))
        assert np.array_equal(C, C.T)
        np.testing.assert_allclose(C, rC, rtol=1e-8, atol=1e-10)


def _same(a, b):
    """Two nat.laplace results, bit for bit (C may be None in both)."""
    return (np.array_equal(a[0], b[0]) and (a[1] is b[1] or np.array_equal(a[1], b[1])) and
            a[2:] == b[2:])


def test_laplace_cached_context_reuse(nat):
    """The stand-alone call keeps one context per (device, n); n = 131 is used by no other test.
    Problem 1, another problem, problem 1 again: the third call returns bitwise what the first
    did, whether the call between them asked for the covariance, for f and lml only, or stopped
    at max_iters = 1 with STATUS_MAXITER."""
    n = 131
    p1, p2 = (gr.make_case(n, ec.D, 'ard', seed) for seed in (1311, 1312))
    K1 = Cov('se', 'ard').gram(p1['X'], p1['thetas'][0], EPS)
    K2 = Cov('se', 'ard').gram(p2['X'], p2['thetas'][1], EPS)
    y1, y2 = p1['y'], p2['y']
    assert not np.array_equal(y1, y2)
    first = nat.laplace(K1, y1, True, True, ec.FIT_TOL, 1000)
    other = nat.laplace(K2, y2, True, True, ec.FIT_TOL, 1000)
    assert first[4] == 0 and other[4] == 0 and first[3] > 1 and other[3] > 1
    assert first[2] != other[2] and not np.array_equal(first[0], other[0])
    assert _same(nat.laplace(K1, y1, True, True, ec.FIT_TOL, 1000), first)
    # f and lml only, right behind a call that left K W^1/2 -> V^T and C in the bottom rows
    lean = nat.laplace(K2, y2, False, True, ec.FIT_TOL, 1000)
    assert lean[1] is None and np.array_equal(lean[0], other[0]) and lean[2:] == other[2:]
    assert _same(nat.laplace(K1, y1, True, True, ec.FIT_TOL, 1000), first)
    lean1 = nat.laplace(K1, y1, False, True, ec.FIT_TOL, 1000)
    assert np.array_equal(lean1[0], first[0]) and lean1[2:] == first[2:]
    # a call that fails with STATUS_MAXITER leaves nothing behind either
    assert nat.laplace(K2, y2, True, True, ec.FIT_TOL, 1)[4] == nat.STATUS_MAXITER
    assert _same(nat.laplace(K1, y1, True, True, ec.FIT_TOL, 1000), first)
    assert _same(nat.laplace(K2, y2, True, True, ec.FIT_TOL, 1000), other)


# ----------------------------------------------------------------------------- E. call order

def test_call_order_on_one_context(nat):
    """N = 577, d = 5 (nb = 10: the Gram's partial copy into chol(K)'s working buffer is active),
    n_imp = 8, max_batch = 2. An IS theta-call for two thetas into two slots, a u-call on a second
    U buffer and both slots read back give the same bits on a fresh context and on one that ran
    predict and laplace_grad first; predict, laplace_grad and the Laplace theta-call give the
    same bits on a fresh context, before and after the IS sequence. The Newton settings are part
    of the state and are set before every call."""
    n, d, m = 577, 5, 70
    c = gr.make_case(n, d, 'ard', 5770)
    thetas = c['thetas'][:2]
    rng = np.random.RandomState(5771)
    Xs = rng.normal(size=(m, d))
    Xs[0], Xs[-1] = c['X'][ec.I_EQ], c['X'][ec.I_FAR] + 50.0

    def context():
        ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=2, n_slots=2,
                          n_ubufs=2)
        ctx.u_normal([0, 1], [57, 58], [0, 1])
        return ctx

    def is_sequence(ctx):
        ctx.set_newton(ec.FIT_TOL, 1000)
        out, st, nops = ctx.theta_eval(nat.EST_IS, thetas, [0, 0], [0, 1])
        out2, st2 = ctx.u_eval([0, 1], [1, 1])
        assert not st.any() and not st2.any()
        rec = [out, st, nops, out2, st2]
        for slot in (0, 1):
            rec.extend(np.asarray(a) for a in ctx.slot_read(slot))
        return rec

    def laplace_calls(ctx):
        ctx.set_newton(ec.FIT_TOL, 1000)
        rec = list(ctx.predict(thetas, Xs))
        assert not rec[3].any()
        ctx.set_newton(ec.GRAD_TOL, 1000)
        rec.extend(ctx.laplace_grad(thetas))
        assert not rec[7].any()
        ctx.set_newton(ec.GRAD_TOL, 1000)
        rec.extend(ctx.theta_eval(nat.EST_LAPLACE, thetas))
        assert not rec[10].any()
        return rec

    def same(a, b):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), i

    ctx1 = context()
    alone = is_sequence(ctx1)
    ctx1.close()
    ctx2 = context()
    before = laplace_calls(ctx2)
    same(is_sequence(ctx2), alone)
    after = laplace_calls(ctx2)
    ctx2.close()
    ctx3 = context()
    fresh = laplace_calls(ctx3)
    ctx3.close()
    same(after, fresh)
    same(before, fresh)
    assert all(np.all(np.isfinite(x)) for x in alone + fresh)
