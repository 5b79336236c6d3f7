"""Replicate spread and weight diagnostics of the IS estimate on the device (apm_u_eval_diag,
apm_is_spread; is_diag.hip k_lme_blocks, host_is_diag.cpp): the full-block value
against apm_u_eval bitwise, sub-blocks against the numpy restatement
(tests/is_spread_restatement.py), batch independence, that nothing else on the context moves,
refusals and failed chains, and the Python layers."""
import math

import numpy as np
import pytest

import epis_restatement as eis
import grad_restatement as gr
import is_spread_restatement as sr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = 1e-8
LOGF_TOL = 5e-4  # |delta log f| of an IS estimate, nats, absolute
# ess and wmax against the restatement, relative: ten times the worst value measured over the
# sub-block cases below, 1.20e-6 (wmax at S = 50, B = 16, Laplace; DESIGN.md §20 has them all)
DIAG_TOL = 1.2e-5
# (n, d, S): the smallest multi-tile n with one sample block; ragged n and ragged S (padded
# columns); three sample blocks; a second outer panel; past k_lme's 1024-sample LDS copy
SHAPES = [(65, 4, 64), (130, 5, 50), (130, 5, 192), (513, 4, 64), (65, 4, 1088)]
SIGMAS = (0.3, 3.0)
SEEDS = np.array([0x5eed0001, 0x5eed0002], dtype=np.uint64)
CTRS = np.array([7, 1 << 33], dtype=np.uint64)


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _case(n, d):
    return gr.make_case(n, d, 'ard', 9000 + n, rows=SIGMAS)


def _context(nat, c, S, likelihood='probit', max_batch=2, n_slots=2, n_ubufs=4):
    return nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, S, max_batch=max_batch,
                       n_slots=n_slots, n_ubufs=n_ubufs, likelihood=likelihood)


def _theta_call(nat, ctx, est, thetas, slots, ubufs):
    """The theta-call that fills `slots` (draws of its own in `ubufs`); every chain must be OK."""
    T = len(thetas)
    ctx.u_normal(ubufs, [11] * T, list(range(T)))
    out, st, _ = ctx.theta_eval(est, thetas, ubufs, slots)
    assert not st.any(), st
    return out


@pytest.mark.parametrize('likelihood', ['probit', 'logit'])
@pytest.mark.parametrize('n,d,S', SHAPES)
def test_full_block_is_u_eval_bitwise(nat, n, d, S, likelihood):
    """B = S: every replicate's logf is bitwise apm_u_normal(seed, counter + r) on a second buffer
    followed by apm_u_eval, with equal statuses, and apm_u_eval_diag's logf is apm_u_eval's - for
    slots written by every estimator the likelihood has, both thetas as one batch of two."""
    c = _case(n, d)
    ests = [nat.EST_IS, nat.EST_PRIORMC] + ([nat.EST_IS_EP] if likelihood == 'probit' else [])
    ctx = _context(nat, c, S, likelihood)
    try:
        for est in ests:
            _theta_call(nat, ctx, est, c['thetas'], [0, 1], [0, 1])
            logf, ess, wmax, st = ctx.is_spread([0, 1], [0, 1], SEEDS, CTRS, 3)
            assert logf.shape == (2, 3, 1) and not st.any()
            for r in range(3):
                ctx.u_normal([2, 3], SEEDS, CTRS + np.uint64(r))
                ref, rst = ctx.u_eval([0, 1], [2, 3])
                assert np.array_equal(rst, st)
                assert np.array_equal(logf[:, r, 0], ref), (est, r, logf[:, r, 0], ref)
                dlogf, dess, dwmax, dst = ctx.u_eval_diag([0, 1], [2, 3])
                assert np.array_equal(dlogf[:, 0], ref) and np.array_equal(dst, rst)
                assert np.array_equal(dess[:, 0], ess[:, r, 0])
                assert np.array_equal(dwmax[:, 0], wmax[:, r, 0])
            assert np.isfinite(logf).all()
            assert (ess >= 1.0).all() and (ess <= S * (1 + 1e-12)).all()
            assert (wmax >= 1.0 / S * (1 - 1e-12)).all() and (wmax <= 1.0).all()
    finally:
        ctx.close()


def _state(name, K, y):
    return eis.laplace_state(K, y) if name == 'laplace' else eis.state(K, y)


@pytest.mark.parametrize('proposal', ['laplace', 'ep'])
@pytest.mark.parametrize('S,B', [(192, 64), (50, 16), (50, 1), (192, 1)])
def test_sub_blocks_vs_restatement(nat, S, B, proposal):
    """(130, 5), both thetas, two replicates: logf, ess and wmax of every block against the
    restatement on the downloaded draws; B = 1 gives ess = wmax = 1 exactly; and on the device
    the log-mean-exp of the block values is the B = S value to 1e-12 relative (where B divides
    S: at S = 50, B = 16 two samples belong to no block)."""
    c = _case(130, 5)
    est = nat.EST_IS if proposal == 'laplace' else nat.EST_IS_EP
    ctx = _context(nat, c, S)
    try:
        _theta_call(nat, ctx, est, c['thetas'], [0, 1], [0, 1])
        logf, ess, wmax, st = ctx.is_spread([0, 1], [0, 1], SEEDS, CTRS, 2, B)
        full = ctx.is_spread([0, 1], [0, 1], SEEDS, CTRS, 2)[0]
        U = []
        for r in range(2):
            ctx.u_normal([2, 3], SEEDS, CTRS + np.uint64(r))
            U.append([ctx.u_download(2), ctx.u_download(3)])
    finally:
        ctx.close()
    nblk = S // B
    assert logf.shape == (2, 2, nblk) and not st.any()
    worst = [0.0, 0.0, 0.0]
    for t in range(2):
        ref_st = _state(proposal, Cov('se', 'ard').gram(c['X'], c['thetas'][t], EPS), c['y'])
        for r in range(2):
            lw = sr.log_weights(c['y'], ref_st, U[r][t])
            rl, re, rw = sr.blocks(lw, B)
            worst[0] = max(worst[0], np.abs(logf[t, r] - rl).max())
            worst[1] = max(worst[1], np.abs(ess[t, r] / re - 1).max())
            worst[2] = max(worst[2], np.abs(wmax[t, r] / rw - 1).max())
            if S % B == 0:
                lme = sr.log_mean_exp(logf[t, r])
                assert abs(lme - full[t, r, 0]) <= 1e-12 * max(1.0, abs(full[t, r, 0]))
    print('sub-blocks S {0} B {1} {2}: d logf {3:.2e} nats, ess {4:.2e}, wmax {5:.2e} relative'
          .format(S, B, proposal, *worst))
    assert worst[0] <= LOGF_TOL
    assert worst[1] <= DIAG_TOL and worst[2] <= DIAG_TOL
    if B == 1:
        assert np.array_equal(ess, np.ones_like(ess)) and np.array_equal(wmax, np.ones_like(wmax))


def test_batch_independence(nat):
    """A chain's outputs are bitwise the same alone and as the last of 4."""
    c = _case(130, 5)
    th = c['thetas'][[0, 1, 0, 1]]
    seeds = np.r_[SEEDS, SEEDS + np.uint64(9)]
    ctrs = np.r_[CTRS, CTRS]
    ctx = _context(nat, c, 192, max_batch=4, n_slots=4, n_ubufs=5)
    try:
        _theta_call(nat, ctx, nat.EST_IS, th, [0, 1, 2, 3], [0, 1, 2, 3])
        four = ctx.is_spread([0, 1, 2, 3], [0, 1, 2, 3], seeds, ctrs, 2, 64)
        one = ctx.is_spread([3], [4], seeds[3:], ctrs[3:], 2, 64)
        ctx.u_normal([0, 1, 2, 3], seeds, ctrs)
        four_d = ctx.u_eval_diag([0, 1, 2, 3], [0, 1, 2, 3], 64)
        one_d = ctx.u_eval_diag([3], [3], 64)
    finally:
        ctx.close()
    for a, b in zip(four + four_d, one + one_d):
        assert np.array_equal(a[3:], b)
    assert np.array_equal(four[0][3, 0], four_d[0][3])  # (replicate 0 is the counter itself)


def _sequence(nat, ctx, c, Xs):
    """An IS theta-call with its u-call, a slot read-back and apm_is_predict, as a flat list."""
    ctx.u_normal([0, 1], [3, 4], [0, 0])
    rec = list(ctx.theta_eval(nat.EST_IS, c['thetas'][:1], [0], [0]))
    rec.extend(ctx.u_eval([0], [1]))
    rec.extend(np.asarray(a) for a in ctx.slot_read(0))
    rec.extend(ctx.is_predict(nat.EST_IS, c['thetas'][:1], [0], [1], Xs))
    return rec


def test_nothing_else_moves(nat):
    """The same calls give the same bits before and after apm_is_spread on one context, and on a
    fresh one; the scratch buffer ends as apm_u_normal(seed, counter + n_rep - 1) fills it."""
    c = _case(130, 5)
    Xs = np.random.RandomState(5).normal(size=(5, 5))
    ctx = _context(nat, c, 50, max_batch=2, n_slots=2, n_ubufs=4)
    try:
        before = _sequence(nat, ctx, c, Xs)
        logf = ctx.is_spread([0], [2], SEEDS[:1], CTRS[:1], 4, 16)[0]
        scratch = ctx.u_download(2)
        ctx.u_normal([3], SEEDS[:1], CTRS[:1] + np.uint64(3))
        assert np.array_equal(scratch, ctx.u_download(3))
        after = _sequence(nat, ctx, c, Xs)
    finally:
        ctx.close()
    fresh_ctx = _context(nat, c, 50, max_batch=2, n_slots=2, n_ubufs=4)
    try:
        fresh = _sequence(nat, fresh_ctx, c, Xs)
    finally:
        fresh_ctx.close()
    assert np.isfinite(logf).all() and len(before) == len(after) == len(fresh)
    for a, b, f in zip(before, after, fresh):
        assert np.array_equal(a, b) and np.array_equal(a, f)


def test_invalid_arguments_and_failed_chains(nat):
    c = _case(65, 4)
    S = 64
    ctx = _context(nat, c, S, max_batch=2, n_slots=2, n_ubufs=2)
    lib, h = ctx.lib, ctx._h
    idx = np.array([0, 1], dtype=np.int64)
    far = np.array([0, 2], dtype=np.int64)
    out = np.full((3, 2, 64), 7.0)
    st = np.full(2, 9, dtype=np.int32)

    def spread(count=2, slots=idx, ubufs=idx, seeds=SEEDS, ctrs=CTRS, n_rep=2, block=S, ldo=64):
        p = [None if a is None else a.ctypes.data for a in (slots, ubufs, seeds, ctrs)]
        return lib.apm_is_spread(h, count, p[0], p[1], p[2], p[3], n_rep, block,
                                 out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, ldo,
                                 st.ctypes.data)

    def diag(count=2, slots=idx, ubufs=idx, block=S, ldo=64):
        p = [None if a is None else a.ctypes.data for a in (slots, ubufs)]
        return lib.apm_u_eval_diag(h, count, p[0], p[1], block, out[0].ctypes.data,
                                   out[1].ctypes.data, out[2].ctypes.data, ldo, st.ctypes.data)
    try:
        bad = [spread(block=0), spread(block=S + 1), spread(n_rep=0), spread(n_rep=4097),
               spread(n_rep=65, block=1, ldo=1 << 20), spread(n_rep=2, block=16, ldo=7),
               spread(count=3), spread(count=0), spread(slots=None), spread(ubufs=None),
               spread(seeds=None), spread(ctrs=None), spread(slots=far), spread(ubufs=far),
               diag(block=0), diag(block=S + 1), diag(block=1, ldo=63), diag(count=3),
               diag(slots=None), diag(ubufs=None), diag(ubufs=far)]
        assert bad == [nat.APM_E_INVALID] * len(bad)
        assert (out == 7.0).all() and (st == 9).all()  # nothing was written
        # chain 1 is good; chain 0's theta-call then fails (one Newton iteration allowed)
        _theta_call(nat, ctx, nat.EST_IS, c['thetas'][1:], [1], [1])
        alone = ctx.is_spread([1], [1], SEEDS[1:], CTRS[1:], 2, 16)
        alone_d = ctx.u_eval_diag([1], [1], 16)
        ctx.set_newton(1e-4, 1)
        _, fst, _ = ctx.theta_eval(nat.EST_IS, c['thetas'][1:], [0], [0])
        assert fst[0] == nat.STATUS_MAXITER
        both = ctx.is_spread([0, 1], [0, 1], SEEDS, CTRS, 2, 16)
        ref_st = ctx.u_eval([0, 1], [0, 1])[1]
        both_d = ctx.u_eval_diag([0, 1], [0, 1], 16)
        # every output may be NULL
        assert lib.apm_is_spread(h, 2, idx.ctypes.data, idx.ctypes.data, SEEDS.ctypes.data,
                                 CTRS.ctypes.data, 2, 16, None, None, None, 8,
                                 st.ctypes.data) == 0
        # a later good theta-call into the slot clears the mark
        ctx.set_newton(1e-4, 1000)
        _theta_call(nat, ctx, nat.EST_IS, c['thetas'][:1], [0], [0])
        again = ctx.is_spread([0, 1], [0, 1], SEEDS, CTRS, 2, 16)
    finally:
        ctx.close()
    for got, ref in ((both, alone), (both_d, alone_d)):
        assert np.array_equal(got[3], ref_st)           # what apm_u_eval gives it
        for k in range(3):
            assert np.isnan(got[k][0]).all()            # NaN diagnostics for the failed chain
            assert np.array_equal(got[k][1], ref[k][0])  # the other keeps the bits it has alone
    assert np.isfinite(again[0]).all() and np.array_equal(again[0][1], alone[0][0])


@pytest.mark.parametrize('which', ['laplace', 'ep', 'priormc'])
def test_estimator_spread_and_n_imp_curve(nat, which):
    """estimator.spread returns Context.is_spread's bits; n_imp_curve at block n_imp is spread."""
    import gpdemo.estimators as est
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    c = _case(65, 4)
    kf = krn.make_kernel_func('ard', EPS)
    if which == 'priormc':
        e, code = est.LogMarginalLikelihoodPriorMCEstimator(c['X'], c['y'], kf), nat.EST_PRIORMC
    elif which == 'ep':
        e = est.LogMarginalLikelihoodApproxPosteriorISEstimator(c['X'], c['y'], kf,
                                                                lpa.ep_approximation)
        code = nat.EST_IS_EP
    else:
        e = est.LogMarginalLikelihoodApproxPosteriorISEstimator(c['X'], c['y'], kf,
                                                                lpa.laplace_approximation)
        code = nat.EST_IS
    th = c['thetas'][0]
    with pytest.raises(ValueError):
        e.spread(th)  # n_imp is not known before the first call
    ops0 = e.n_cubic_ops
    res = e.spread(th, n_rep=3, block=16, seed=5, n_imp=128)
    assert res['block'] == 16 and res['log_estimates'].shape == (3, 8)
    assert e.n_cubic_ops - ops0 == res['n_cubic_ops'] > 0
    assert res['sd'] == np.std(res['log_estimates'], ddof=1)
    ctx = e._prob.ctx(128)
    ctx.u_normal([0], [5], [0])
    slot = ctx.slots.acquire()
    try:
        _, st, _ = ctx.theta_eval(code, th[None], [0], [slot])
        assert st[0] == 0
        logf, ess, wmax, _ = ctx.is_spread([slot], [0], [5], [0], 3, 16)
    finally:
        ctx.slots.release(slot)
    assert np.array_equal(res['log_estimates'], logf[0])
    assert np.array_equal(res['ess'], ess[0]) and np.array_equal(res['wmax'], wmax[0])
    e(np.zeros((65, 128)), th)  # the last call's n_imp becomes the default
    curve = est.n_imp_curve(e, th, n_rep=3, seed=5)
    full = e.spread(th, n_rep=3, seed=5)
    assert list(curve) == [64, 128] and full['block'] == 128
    for k in ('log_estimates', 'ess', 'wmax'):
        assert np.array_equal(curve[128][k], full[k])
    assert curve[128]['sd'] == full['sd']
    # the same draws at every block length: the blocks of 64 average to the full estimate
    for r in range(3):
        lme = sr.log_mean_exp(curve[64]['log_estimates'][r])
        assert abs(lme - full['log_estimates'][r, 0]) <= 1e-12 * abs(full['log_estimates'][r, 0])
    curves, block = est.tune_n_imp(e, c['thetas'], target_sd=1e9, n_rep=2)
    assert len(curves) == 2 and block == 64
    assert est.tune_n_imp(e, c['thetas'][:1], target_sd=0.0, n_rep=2)[1] is None


def test_sampler_estimate_spread_leaves_the_trajectories_alone(nat):
    """E-SS + MH, 4 chains at n = 130: 3 steps, estimate_spread, 3 steps is bitwise 6 steps."""
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler
    c = _case(130, 5)
    prior = dict(a_tau=1., b_tau=1. / 5 ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(5, math.log(2.))], (4, 1))

    def run(with_spread):
        smp = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 4, 64, prior, prop_scales=0.1, seed=31)
        try:
            smp.initialise(th0)
            trace, got = [], []
            for k in range(6):
                if with_spread and k == 3:
                    got.append(smp.estimate_spread(n_rep=4, block=32))
                    got.append(smp.estimate_spread(n_rep=4, block=32))
                smp.step()
                trace.append((smp.theta.copy(), smp.log_f.copy()))
            u = [smp.ctx.u_download(b) for b in smp.ub_u]
        finally:
            smp.ctx.close()
        return trace, u, got
    plain, u0, _ = run(False)
    mixed, u1, got = run(True)
    for (ta, fa), (tb, fb) in zip(plain, mixed):
        assert np.array_equal(ta, tb) and np.array_equal(fa, fb)
    for a, b in zip(u0, u1):
        assert np.array_equal(a, b)
    first, second = got
    assert first['log_estimates'].shape == (4, 4, 2) and first['block'] == 32
    assert np.isfinite(first['log_estimates']).all() and (first['sd'] > 0).all()
    assert (first['ess'] >= 1).all() and (first['ess'] <= 32 * (1 + 1e-12)).all()
    # the stream moves on: a second call draws fresh replicates
    assert not np.array_equal(first['log_estimates'], second['log_estimates'])
