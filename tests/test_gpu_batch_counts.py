"""Every batched call at 7 to 17 chains, per chain against the fp64 oracle and bitwise against
the chain alone.

The rest of the suite pins the kernels along N and S at 1 to 5 chains (8 in two files) and runs 64
chains only in full-size estimate parities, which cannot see one wrong tile. The work-item orders
take another path from 8 chains up: xcd_remap (update_item.h), which every update kernel of
chol.hip and chol32_update.hip and the bulk rows of k_chol_panel_df32 (chol32_panel.hip) call and
whose text ugemm_item (ugemm_tile.h: k_ugemm, k_is_row_gemm) carries itself, deals the
items over the 8 XCDs with a branch on rem = total & 7, total = tiles x chains. At (N, S) =
(130, 64) the u-path has total = 3 B, so B = 9 .. 15 reach every nonzero remainder, which neither
8 nor 64 chains can; (65, 130) has total = 6 B with a padded sample block; N = 577 adds a far
update and an outer panel boundary. test_batch_counts_host.py holds the preconditions (the
arithmetic, that the chains' references are far apart, that their Newton counts differ).

A. against the oracle / the restatements at the tolerances the suite already states for each
   quantity; B. bitwise against the same chain evaluated with count = 1 in the same context (the
   check that sees one misplaced tile); C. mixed batches: a failed chain in the middle, every
   slot wide (APM_WIDE_Q=0), wide and narrow slots in one batch, the compact and the flagged
   panel form at N = 2048; D. the asynchronous E-SS + RD-SS sampler at 11 chains.

Chains are passed with non-identity slot and U-buffer index arrays (fixed permutations), and every
chain's buffers differ in scale (batch_counts_cases.chain_draws), so a kernel that reads chain b's
data through the wrong index is wrong under A as well as B.

Measured values are in the docstrings below; DESIGN.md §29 has the table."""
import math
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp

import apm_oracle as orc
import batch_counts_cases as bc
import cov_restatement as cr
import ep_restatement as ep
import epis_restatement as eis
import is_loo_restatement as ilr
import is_predict_restatement as ipr
import is_spread_restatement as sr
import test_gpu_ep as tge
import test_gpu_ep_grad as tgeg
import test_gpu_grad as tgg
from cov_restatement import Cov
from predict_restatement import predictive
from test_gpu_epis import IS_TOL
from test_gpu_is_loo import W_TOL, _r32
from test_gpu_is_predict import PROB_TOL, _fit, _grams
from test_gpu_is_spread import LOGF_TOL
from test_gpu_kernels import _mixed_case, _run_is_stats
from test_gpu_predict import TOL as FP64_TOL
from test_gpu_predict import _make_case
from test_gpu_psis import B_TOL, _check_B, _ratios

pytestmark = pytest.mark.gpu

TOL = bc.TOL  # 5e-4 nats
EPS = bc.EPS
SWEEP = [(shape, b) for shape in bc.SHAPES for b in bc.BATCHES[shape]]


def _id(case):
    return 'N{0}-S{1}-B{2}'.format(case[0][0], case[0][1], case[1])


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


@pytest.fixture(scope='module')
def refs():
    """The oracle's values per shape and chain (batch_counts_cases.refs), once per module."""
    return {shape: bc.refs(shape) for shape in bc.SHAPES}


@pytest.fixture(scope='module')
def loo_refs(refs):
    """Per shape and chain of the LOO batches: the restatement's log ratios, normalised log
    weights and their fp32 yardstick Y, as test_gpu_psis.refs forms them."""
    out = {}
    for shape, bs in bc.LOO_BATCHES.items():
        r = refs[shape]
        y = r['c']['y']
        for b in range(max(bs)):
            slot = ilr.slot_of(_fit(r['st'][b]['K'], y, 'laplace', 'probit'))
            t, lwbar = _ratios(ilr.loo_quantities(y, *slot, r['U1'][b], 'probit'))
            t32, _ = _ratios(ilr.loo_quantities(y, slot[0], slot[1], slot[2], _r32(slot[3]),
                                                slot[4], _r32(r['U1'][b]), 'probit'))
            assert np.isfinite(t).all() and np.isfinite(t32).all()
            out[shape, b] = dict(t=t, lwbar=lwbar, Y=float(np.abs(t32 - t).max()))
    return out


# ----------------------------------------------------------------------------- the device side

class _Layout(object):
    """Where chain b's data lives in a context of B chains: IS slot sl[b] and PriorMC slot
    psl[b] of 2 B slots, buffers ub1[b] (U1) and ub2[b] (U2) of 2 B buffers - four different
    fixed permutations, none the identity."""

    def __init__(self, B):
        self.B = B
        self.sl, self.psl = bc.perm(B, 3), B + bc.perm(B, 1)
        self.ub1, self.ub2 = bc.perm(B, 1), B + bc.perm(B, 2)


def _open(nat, monkeypatch, r, B, env=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    ctx = nat.Context(r['c']['X'], r['c']['y'], nat.KERNEL_ARD, EPS, r['s'], max_batch=B,
                      n_slots=2 * B, n_ubufs=2 * B)
    for k in env or {}:
        monkeypatch.delenv(k)
    lay = _Layout(B)
    for b in range(B):
        ctx.u_upload(lay.ub1[b], r['U1'][b])
        ctx.u_upload(lay.ub2[b], r['U2'][b])
    return ctx, lay


def _calls(nat, ctx, lay, thetas, idx, loo=False):
    """The theta- and u-calls of chains idx (in that order in every call): dict of arrays whose
    leading axis runs over idx."""
    idx = np.asarray(idx, dtype=np.int64)
    th = thetas[idx]
    o = {}
    o['is'], o['is_st'], o['is_ops'] = ctx.theta_eval(nat.EST_IS, th, lay.ub1[idx], lay.sl[idx])
    state = [ctx.slot_read(s) for s in lay.sl[idx]]
    o['L'], o['f'], o['g'] = (np.stack([s[k] for s in state]) for k in range(3))
    o['cst'] = np.array([s[3] for s in state])
    o['u'], o['u_st'] = ctx.u_eval(lay.sl[idx], lay.ub2[idx])
    o['pm'], o['pm_st'], o['pm_ops'] = ctx.theta_eval(nat.EST_PRIORMC, th, lay.ub1[idx],
                                                      lay.psl[idx])
    o['pmu'], o['pmu_st'] = ctx.u_eval(lay.psl[idx], lay.ub2[idx])
    o['LK'] = np.stack([ctx.slot_read(s)[0] for s in lay.psl[idx]])
    o['lml'], o['lml_st'], o['lml_ops'] = ctx.theta_eval(nat.EST_LAPLACE, th)
    if loo:
        for k, a in zip(('logf', 'loo', 'lpd', 'ess_loo', 'gauss', 'ess', 'st'),
                        ctx.is_loo(lay.sl[idx], lay.ub1[idx])):
            o['loo_' + k] = a
        for k, a in zip(('logf', 'loo', 'khat', 'khat_w', 'lr', 'st'),
                        ctx.is_loo_psis(lay.sl[idx], lay.ub1[idx], want_logratio=True)):
            o['psis_' + k] = a
        o['lw'] = ctx.u_eval_diag(lay.sl[idx], lay.ub1[idx], block=1)[0]
    return o


def _assert_bitwise(batch, alone, q, b, label):
    """Every output of position q of the batch is that of chain b's own call, bit for bit."""
    for k in batch:
        np.testing.assert_array_equal(batch[k][q], alone[k][0],
                                      err_msg='{0}: chain {1} output {2}'.format(label, b, k))


def _rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def _check_A(r, o, chains, label):
    """A for the theta- and u-calls of `chains` (o's leading axis): the slot state under
    test_slot_state_vs_oracle's bounds, the estimates to 5e-4 nats, the LML to 1e-7 relative, op
    counts equal. Prints the case's maxima, then asserts."""
    w = dict(L=0.0, f=0.0, g=0.0, cst=0.0, est=0.0, lml=0.0)
    for q, b in enumerate(chains):
        st = r['st'][b]
        assert o['is_st'][q] == 0 and o['u_st'][q] == 0 and o['pm_st'][q] == 0, (label, b)
        assert o['pmu_st'][q] == 0 and o['lml_st'][q] == 0, (label, b)
        assert o['is_ops'][q] == r['ops'][b] == st['n_ops'] + 2, (label, b, o['is_ops'][q])
        assert o['pm_ops'][q] == 1 and o['lml_ops'][q] == r['lops'][b], (label, b)
        w['L'] = max(w['L'], _rel(o['L'][q], np.tril(st['C_chol'])))
        w['f'] = max(w['f'], _rel(o['f'][q], st['f_post']))
        w['g'] = max(w['g'], _rel(o['g'][q], st['g']))
        w['cst'] = max(w['cst'], abs(o['cst'][q] - st['cst']) / r['cst_bound'][b])
        for key, ref in (('is', 'is1'), ('u', 'is2'), ('pm', 'pm1'), ('pmu', 'pm2')):
            w['est'] = max(w['est'], abs(o[key][q] - r[ref][b]))
        w['lml'] = max(w['lml'], abs(o['lml'][q] - r['lml'][b]) / max(1., abs(r['lml'][b])))
    print('{0}: A max|dL|/max|L| {L:.2e} (1e-5) max|df|/max|f| {f:.2e} (1e-8) max|dg|/max|g| '
          '{g:.2e} (2e-6) |d cst| / bound {cst:.1e} (1) estimates {est:.2e} nats (5e-4) '
          'LML {lml:.2e} (1e-7)'.format(label, **w))
    assert w['f'] <= 1e-8 and w['L'] <= 1e-5 and w['g'] <= 2e-6 and w['cst'] <= 1.0, (label, w)
    assert w['est'] <= TOL and w['lml'] < 1e-7, (label, w)
    return w


def _check_loo(lr_, o, chains, shape, label):
    """A and B of test_gpu_psis on every chain: the stored log ratios and normalised log weights
    under W_TOL + 10 Y, loo_psis / khat / khat_w against psis_restatement on the device's own
    ratios within B_TOL, and the raw sum of the ratios against apm_is_loo's loo."""
    w = dict(t=0.0, b=0.0, raw=0.0, frac=0.0)
    for q, b in enumerate(chains):
        ref = lr_[shape, b]
        assert o['loo_st'][q] == 0 and o['psis_st'][q] == 0
        bound = W_TOL + 10.0 * ref['Y']
        lr = o['psis_lr'][q]
        assert np.array_equal(np.isneginf(lr), np.isneginf(ref['t']))
        lwbar = o['lw'][q] - logsumexp(o['lw'][q])
        d_t = max(float(np.abs(lr - ref['t']).max()), float(np.abs(lwbar - ref['lwbar']).max()))
        dev = dict(ps=tuple(o['psis_' + k][q:q + 1] for k in
                            ('logf', 'loo', 'khat', 'khat_w', 'lr', 'st')), lwbar=lwbar)
        d_b = max(_check_B(dev, '{0} chain {1}'.format(label, b)))
        d_raw = float(np.abs(-logsumexp(lr, axis=1) - o['loo_loo'][q]).max())
        w['t'], w['b'], w['raw'] = max(w['t'], d_t), max(w['b'], d_b), max(w['raw'], d_raw)
        w['frac'] = max(w['frac'], d_t / bound)
        assert d_t <= bound, (label, b, d_t, bound)
        assert d_b <= B_TOL and d_raw <= 1e-12, (label, b, d_b, d_raw)
        assert o['psis_logf'][q] == o['loo_logf'][q]
    print('{0}: LOO / PSIS A log ratios {t:.2e} ({frac:.3f} of W_TOL + 10 Y) B loo_psis, khat, '
          'khat_w {b:.2e} (1e-8) raw sum {raw:.2e} (1e-12)'.format(label, **w))


def _sweep(nat, monkeypatch, refs, shape, B, loo_refs=None, env=None, label=''):
    """A on the batch of the first B chains and B against each chain alone, in one context."""
    r = refs[shape]
    label = _id((shape, B)) + label
    ctx, lay = _open(nat, monkeypatch, r, B, env=env)
    loo = loo_refs is not None
    try:
        chains = np.arange(B)
        batch = _calls(nat, ctx, lay, r['thetas'], chains, loo)
        for b in chains:
            _assert_bitwise(batch, _calls(nat, ctx, lay, r['thetas'], [b], loo), b, b, label)
    finally:
        ctx.close()
    w = _check_A(r, batch, chains, label)
    if loo:
        _check_loo(loo_refs, batch, chains, shape, label)
    return w


# ----------------------------------------------------------------------------- A and B

@pytest.mark.parametrize('case', SWEEP, ids=_id)
def test_theta_and_u_calls_vs_oracle_and_alone(nat, monkeypatch, refs, loo_refs, case):
    """IS theta-call with apm_slot_read (every lower entry of the factor, f_post, g, cst), cached
    u-call on a second buffer, PriorMC theta- and u-call and the Laplace theta-call of B chains in
    one call each, against the oracle per chain and bitwise against the chain alone; apm_is_loo and
    apm_is_loo_psis with the log ratios at the batches of LOO_BATCHES.
    Measured on an MI355X (maxima over the batches at N = 130 / 65 / 577; DESIGN.md §29 has them
    per B): factor 1.24e-7 / 1.12e-7 / 3.88e-7 (1e-5), f_post 3.9e-11 / 5.9e-12 / 3.2e-9 (1e-8), g
    4.0e-8 / 5.2e-8 / 4.8e-8 (2e-6), cst at most 1e-2 of its bound, estimates 4.44e-5 / 4.37e-5 /
    1.22e-4 nats (5e-4), LML 5.5e-15 relative (1e-7), op counts equal; log ratios 9.44e-5 (0.09 of
    W_TOL + 10 Y), PSIS against its restatement 1.8e-14 (1e-8); every bitwise comparison exact."""
    shape, B = case
    with_loo = B in bc.LOO_BATCHES.get(shape, ())
    _sweep(nat, monkeypatch, refs, shape, B, loo_refs if with_loo else None)


@pytest.mark.parametrize('B', bc.DIAG_BATCHES)
def test_diag_and_spread_vs_oracle_and_alone(nat, monkeypatch, refs, B):
    """apm_u_eval_diag with blocks of one sample and apm_is_spread with two replicates of
    one-sample blocks at (130, 64): a block's estimate is its sample's log weight, compared with
    the restatement's on the uploaded (the downloaded, for the replicates) draws under
    test_gpu_is_spread's 5e-4 nats; ess = wmax = 1 exactly; bitwise the chain alone.
    Measured on an MI355X: apm_u_eval_diag 4.03e-5 (B = 9) and 6.59e-5 (B = 12), apm_is_spread
    1.21e-5 nats; the bitwise comparisons exact."""
    shape = (130, 64)
    r = refs[shape]
    y = r['c']['y']
    ctx, lay = _open(nat, monkeypatch, r, B)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(0x5eed0100)
    ctrs = np.array([7 + (b << 20) for b in range(B)], dtype=np.uint64)
    try:
        chains = np.arange(B)
        _, st0, _ = ctx.theta_eval(nat.EST_IS, r['thetas'][:B], lay.ub1, lay.sl)
        assert not st0.any()
        diag = ctx.u_eval_diag(lay.sl, lay.ub1, block=1)
        spread = ctx.is_spread(lay.sl, lay.ub2, seeds, ctrs, 2, 1)  # (the U2 buffers are scratch)
        drawn = [[ctx.u_download(u) for u in lay.ub2]]
        ctx.u_normal(lay.ub2, seeds, ctrs)
        drawn.insert(0, [ctx.u_download(u) for u in lay.ub2])
        for b in chains:
            one = ctx.u_eval_diag(lay.sl[b:b + 1], lay.ub1[b:b + 1], block=1)
            for a, c in zip(diag, one):
                np.testing.assert_array_equal(a[b], c[0])
            one = ctx.is_spread(lay.sl[b:b + 1], lay.ub2[b:b + 1], seeds[b:b + 1], ctrs[b:b + 1],
                                2, 1)
            for a, c in zip(spread, one):
                np.testing.assert_array_equal(a[b], c[0])
    finally:
        ctx.close()
    assert not diag[3].any() and not spread[3].any()
    assert diag[0].shape == (B, 64) and spread[0].shape == (B, 2, 64)
    worst = [0.0, 0.0]
    for b in chains:
        fit = eis.laplace_state(r['st'][b]['K'], y)
        worst[0] = max(worst[0], np.abs(diag[0][b] - sr.log_weights(y, fit, r['U1'][b])).max())
        for rep in range(2):
            lw = sr.log_weights(y, fit, drawn[rep][b])
            worst[1] = max(worst[1], np.abs(spread[0][b, rep] - lw).max())
    print('N130-S64-B{0}: u_eval_diag {1:.2e} is_spread {2:.2e} nats (5e-4)'.format(B, *worst))
    assert worst[0] <= LOGF_TOL and worst[1] <= LOGF_TOL
    for a in (diag[1], diag[2], spread[1], spread[2]):
        assert np.array_equal(a, np.ones_like(a))


@pytest.fixture(scope='module')
def family_refs(refs):
    """The restatements of the gradient, the predictives, EP and EP-IS for the first 13 chains of
    (130, 64), computed once."""
    r = refs[130, 64]
    c, y = r['c'], r['c']['y']
    out = []
    for b in range(max(bc.FAMILY_BATCHES)):
        th = r['thetas'][b]
        K, Ks = _grams(c, None, th)
        s = math.exp(th[0])
        fit = ep.ep_fit(K, y)
        tge.assert_stop_margin(fit)
        epis = eis.state(K, y)
        out.append(dict(
            predict=predictive(K, Ks, y, s),
            grad=cr.laplace_grad(Cov('se', 'ard'), c['X'], y, th, EPS, tol=tgg.NEWTON_TOL),
            is_predict=ipr.predictive(K, Ks, s, y, r['U1'][b], _fit(K, y, 'laplace', 'probit'),
                                      'probit'),
            ep=fit, ep_predict=ep.at_test_inputs(Ks, s, fit),
            ep_grad=cr.ep_grad(Cov('se', 'ard'), c['X'], y, th, EPS),
            epis=eis.is_consistent(y, epis, r['U1'][b]), epis_sweeps=epis['n_sweeps']))
    return out


@pytest.mark.parametrize('B', bc.FAMILY_BATCHES)
def test_gradient_predictive_and_ep_calls_vs_restatements_and_alone(nat, monkeypatch, refs,
                                                                    family_refs, B):
    """apm_predict, apm_is_predict, apm_ep_eval, apm_ep_predict, apm_ep_grad, the APM_EST_IS_EP
    theta-call and apm_laplace_grad at (130, 64), B chains in one call (in a permuted order where
    the call takes thetas alone), each against its restatement at the tolerance of its own test
    file and bitwise against the chain alone. Measured on an MI355X (B = 9 / 13): predict 2.8e-14,
    laplace_grad 1.9e-13, ep_eval 2.1e-14, ep_predict 2.6e-14, ep_grad 1.3e-14 / 1.8e-14 (1e-9);
    is_predict 9.0e-7 (1e-3); IS_EP 1.21e-6 / 5.62e-6 nats (5e-4); the bitwise comparisons exact."""
    r = refs[130, 64]
    c = r['c']
    ctx, lay = _open(nat, monkeypatch, r, B)
    order = bc.perm(B, 2)
    th = r['thetas'][order]
    one = lambda b: r['thetas'][b:b + 1]
    try:
        dev = dict(predict=ctx.predict(th, c['Xs']), ep=ctx.ep(th),
                   ep_predict=ctx.ep_predict(th, c['Xs']), ep_grad=ctx.ep_grad(th),
                   is_predict=ctx.is_predict(nat.EST_IS, th, lay.ub1[order], lay.sl[order],
                                             c['Xs']),
                   epis=ctx.theta_eval(nat.EST_IS_EP, th, lay.ub1[order], lay.psl[order]))
        for q, b in enumerate(order):
            alone = dict(predict=ctx.predict(one(b), c['Xs']), ep=ctx.ep(one(b)),
                         ep_predict=ctx.ep_predict(one(b), c['Xs']), ep_grad=ctx.ep_grad(one(b)),
                         is_predict=ctx.is_predict(nat.EST_IS, one(b), lay.ub1[b:b + 1],
                                                   lay.sl[b:b + 1], c['Xs']),
                         epis=ctx.theta_eval(nat.EST_IS_EP, one(b), lay.ub1[b:b + 1],
                                             lay.psl[b:b + 1]))
            for k in dev:
                for a, a1 in zip(dev[k], alone[k]):
                    np.testing.assert_array_equal(a[q], a1[0], err_msg='{0} chain {1}'.format(k, b))
        ctx.set_newton(tgg.NEWTON_TOL, 1000)  # (test_gpu_grad's setting; the last calls here)
        dev['grad'] = ctx.laplace_grad(th)
        for q, b in enumerate(order):
            for a, a1 in zip(dev['grad'], ctx.laplace_grad(one(b))):
                np.testing.assert_array_equal(a[q], a1[0], err_msg='grad chain {0}'.format(b))
    finally:
        ctx.close()
    w = dict(predict=0.0, grad=0.0, is_predict=0.0, ep=0.0, ep_predict=0.0, ep_grad=0.0, epis=0.0)
    for q, b in enumerate(order):
        ref = family_refs[b]
        for k in ('predict', 'ep_predict'):
            mean, var, prob, st, cnt = dev[k]
            assert st[q] == 0
            for key, got in (('mean', mean), ('var', var), ('prob', prob)):
                scale = 1.0 if key == 'prob' else max(1.0, float(np.abs(ref[k][key]).max()))
                w[k] = max(w[k], float(np.abs(got[q] - ref[k][key]).max()) / scale)
        assert int(dev['predict'][4][q]) == ref['predict']['n_iter']
        assert int(dev['ep_predict'][4][q]) == ref['ep']['n_sweeps']
        assert dev['ep'][5][q] == 0 and int(dev['ep'][6][q]) == ref['ep']['n_sweeps']
        w['ep'] = max(w['ep'], tge.parity(dev['ep'], q, ref['ep']))
        w['ep_grad'] = max(w['ep_grad'], tgeg._parity(dev['ep_grad'], q, ref['ep_grad']))
        assert dev['grad'][2][q] == 0
        w['grad'] = max(w['grad'], tgg._parity(dev['grad'][0][q], dev['grad'][1][q], ref['grad']))
        logf, prob, mean, var, ess, st, nops = dev['is_predict']
        rp = ref['is_predict']
        assert st[q] == 0 and int(nops[q]) == r['ops'][b] + 2
        ms = max(1.0, float(np.abs(rp['m']).max()))
        w['is_predict'] = max(w['is_predict'], float(np.abs(prob[q] - rp['prob']).max()),
                              float(np.abs(mean[q] - rp['mean']).max()) / ms,
                              float(np.abs(var[q] - rp['var']).max()) / max(1.0, ms ** 2),
                              abs(ess[q] - rp['ess']) / rp['ess'])
        assert abs(logf[q] - r['is1'][b]) <= TOL
        out, st, nops = dev['epis']
        assert st[q] == 0 and int(nops[q]) == 2 * ref['epis_sweeps'] + 3
        w['epis'] = max(w['epis'], abs(out[q] - ref['epis']))
    print('N130-S64-B{0}: predict {predict:.2e} laplace_grad {grad:.2e} ep_eval {ep:.2e} '
          'ep_predict {ep_predict:.2e} ep_grad {ep_grad:.2e} (1e-9) is_predict {is_predict:.2e} '
          '(1e-3) IS_EP {epis:.2e} nats (5e-4)'.format(B, **w))
    assert FP64_TOL == tge.TOL == tgg.TOL == tgeg.TOL == 1e-9
    for k in ('predict', 'grad', 'ep', 'ep_predict', 'ep_grad'):
        assert w[k] <= FP64_TOL, (k, w[k])
    assert w['is_predict'] <= PROB_TOL and w['epis'] <= IS_TOL


# ----------------------------------------------------------------------------- C. mixed batches

def _failing_theta():
    """theta_0 = 3 of the (130, 5) case of test_gpu_is_loo / test_gpu_psis's failed-slot tests."""
    return _make_case(130, 5, 70, 'ard', 100)['thetas'][1]


@pytest.mark.parametrize('B', (9, 12))
def test_failed_chain_in_the_middle(nat, monkeypatch, refs, loo_refs, B):
    """(130, 64). First the good batch; then, under set_newton(1e-4, 2), a theta-call of its own
    fails the middle chain's slot (theta_0 = 3 needs six iterations) and the batch's u-call, LOO
    and PSIS run over the failed slot: the failed chain has its alone status and NaN outputs, the
    others the bits of their own calls. Second, a theta-call whose middle chain fails inside the
    batch: the others (theta_0 in -14 .. -11, which the two iterations allowed suffice for) keep
    their alone bits, the failed one its alone status and NaN. This case showed that
    apm_theta_eval left a failed chain's out_logf as the context's output buffer held it from an
    earlier call (apm_u_eval likewise over a failed slot): both now return NaN there."""
    r = refs[130, 64]
    ctx, lay = _open(nat, monkeypatch, r, B)
    mid = B // 2
    chains = np.arange(B)
    bad = _failing_theta()
    low = r['thetas'][:B].copy()
    low[:, 0] = np.linspace(-14.0, -11.0, B)
    low[mid] = bad
    calls = lambda i: (ctx.u_eval(lay.sl[i], lay.ub2[i]) + ctx.is_loo(lay.sl[i], lay.ub1[i]) +
                       ctx.is_loo_psis(lay.sl[i], lay.ub1[i], want_logratio=True))
    try:
        _, st0, _ = ctx.theta_eval(nat.EST_IS, r['thetas'][:B], lay.ub1, lay.sl)
        assert not st0.any()
        alone = [calls(chains[b:b + 1]) for b in chains]
        ctx.set_newton(1e-4, 2)
        _, fst, _ = ctx.theta_eval(nat.EST_IS, bad[None], lay.ub1[mid:mid + 1],
                                   lay.sl[mid:mid + 1])
        assert fst[0] == nat.STATUS_MAXITER
        alone[mid] = calls(chains[mid:mid + 1])
        both = calls(chains)
        tb = ctx.theta_eval(nat.EST_IS, low, lay.ub1, lay.sl)
        tb_u = ctx.u_eval(lay.sl, lay.ub2)
        ta = [ctx.theta_eval(nat.EST_IS, low[b:b + 1], lay.ub1[b:b + 1], lay.sl[b:b + 1]) +
              ctx.u_eval(lay.sl[b:b + 1], lay.ub2[b:b + 1]) for b in chains]
    finally:
        ctx.close()
    for b in chains:
        for a, a1 in zip(both, alone[b]):
            np.testing.assert_array_equal(a[b], a1[0])
        for a, a1 in zip(tb + tb_u, ta[b]):
            np.testing.assert_array_equal(a[b], a1[0])
    # (u_eval: value, status; is_loo: 6 outputs, status; is_loo_psis: 5 outputs, status). The
    # status of a call over a failed slot is the u-call's own, which may be 0: the slot's mark
    # is the host's (apm.h), so the failed chain's status is pinned to its alone one above
    st_idx = (1, 8, 14)
    for k, a in enumerate(both):
        if k in st_idx:
            assert not np.delete(a, mid).any()
        else:
            assert np.isnan(a[mid]).all() and np.isfinite(np.delete(a, mid, axis=0)).any()
    assert tb[1][mid] == nat.STATUS_MAXITER and not np.delete(tb[1], mid).any()
    assert np.isnan(tb[0][mid]) and np.isfinite(np.delete(tb[0], mid)).all()
    assert np.isnan(tb_u[0][mid]) and not np.delete(tb_u[1], mid).any()
    assert np.isfinite(np.delete(tb_u[0], mid)).all()
    assert (np.delete(tb[2], mid) <= 2 + 3).all()  # (at most two Newton iterations each)


@pytest.mark.parametrize('B', (9, 12))
def test_every_slot_wide(nat, monkeypatch, refs, loo_refs, B):
    """The same batches under APM_WIDE_Q=0: every slot is wide, so the u-path runs k_ugemm64 /
    k_is_row_gemm64 on the plain (nb nsb, nchains) grid from the fp64 factor and the fp64 U. A and
    B again, LOO and PSIS included. Measured on an MI355X (B = 9 and 12): factor 5.24e-8,
    estimates 3.86e-6 nats, log ratios 1.68e-6 / 3.91e-6; the bitwise comparisons exact."""
    assert B in bc.LOO_BATCHES[130, 64]
    _sweep(nat, monkeypatch, refs, (130, 64), B, loo_refs, env={'APM_WIDE_Q': 0},
           label=' APM_WIDE_Q=0')


# the estimate of a chain at theta_0 = 11 .. 17, relative (test_fp16x3_walk_range_against_fp64)
WIDE_REL = 1e-6


def _default_wide_q():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       'auxiliary-pm-mcmc_amd', 'csrc', 'apm_internal.h')
    with open(src) as fh:
        return float(re.search(r'#define\s+APM_WIDE_Q\s+([0-9.eE+-]+)', fh.read()).group(1))


def test_wide_and_narrow_slots_in_one_batch(nat, monkeypatch, refs):
    """(130, 64), B = 9 under the default APM_WIDE_Q (read from apm_internal.h): chains 2 and 6
    get the smallest theta_0 of 11.5, 12, .. whose oracle trace(C_chol C_chol^T) is at least
    twice the threshold (converging ones exist at N = 130: theta_0 = 12 and 12.5, traces 2.2e6 and
    2.8e6 against 1e6, 15 Newton iterations each), the other seven keep theirs (traces below half
    the threshold), so one u-call holds wide and narrow slots. B bitwise on every chain (IS
    theta-call, u-call, PSIS with the log ratios), equal op counts, and the narrow chains keep
    the bits they have in the all-narrow batch. A: the narrow chains to 5e-4 nats. For the wide
    chains the suite's statement for this range of theta_0 is test_fp16x3_walk_range_against_fp64's
    (theta_0 = 11 .. 17: the default path's estimate within 1e-6 relative of the all-fp64 Newton
    iteration's); it is applied here against the oracle, which that path (APM_MIXED=0) meets to
    6e-6 nats at these thetas.
    Measured on an MI355X: narrow 4.4e-6 nats; wide 1.5e-3 nats at log f = -1.35e5 (theta_0 = 12,
    bound 0.135) and 1.8e-2 at -4.27e5 (theta_0 = 12.5, bound 0.427). That is not the batch's
    doing - each wide chain has the same bits alone - and not the wide u-path's: it is the
    mixed-precision Newton mode (f_post within 7e-9 .. 2e-8 of its maximum there), since with
    APM_MIXED=0 the same chains are within 6e-6 nats (DESIGN.md §29 has the figures per
    theta_0)."""
    r = refs[130, 64]
    B, wide = 9, (2, 6)
    X, y = r['c']['X'], r['c']['y']
    q = _default_wide_q()
    th = r['thetas'][:B].copy()
    ref = {}
    for b in wide:
        for t0 in np.arange(11.5, 16.0, 0.5):
            th[b, 0] = t0
            K = np.empty((130, 130))
            bc.KF(K, X, th[b])
            st = orc.theta_state_pushthrough(K, y)
            if (st['C_chol'] ** 2).sum() >= 2.0 * q:
                break
        else:
            raise AssertionError('no wide theta found')
        v1, rc, ops = orc.is_estimate(X, y, bc.KF, r['U1'][b], th[b])
        ref[b] = (v1, orc.is_estimate(X, y, bc.KF, r['U2'][b], None, rc)[0], ops)
    for b in range(B):
        if b not in wide:
            assert (r['st'][b]['C_chol'] ** 2).sum() < 0.5 * q
            ref[b] = (r['is1'][b], r['is2'][b], r['ops'][b])
    ctx, lay = _open(nat, monkeypatch, r, B)
    call = lambda t, i: (ctx.theta_eval(nat.EST_IS, t[i], lay.ub1[i], lay.sl[i]) +
                         ctx.u_eval(lay.sl[i], lay.ub2[i]) +
                         ctx.is_loo_psis(lay.sl[i], lay.ub1[i], want_logratio=True))
    try:
        chains = np.arange(B)
        narrow = call(r['thetas'], chains)
        mixed = call(th, chains)
        alone = [call(th, chains[b:b + 1]) for b in chains]
    finally:
        ctx.close()
    worst = {True: 0.0, False: 0.0}
    for b in chains:
        for a, a1 in zip(mixed, alone[b]):
            np.testing.assert_array_equal(a[b], a1[0])
        if b not in wide:
            for a, a0 in zip(mixed, narrow):
                np.testing.assert_array_equal(a[b], a0[b])
        assert mixed[1][b] == 0 and mixed[4][b] == 0 and mixed[10][b] == 0
        assert int(mixed[2][b]) == ref[b][2], (b, mixed[2][b], ref[b][2])
        d = max(abs(mixed[0][b] - ref[b][0]), abs(mixed[3][b] - ref[b][1]))
        worst[b in wide] = max(worst[b in wide], d)
        if b in wide:
            print('N130-S64-B9 wide chain {0} (theta_0 = {1}): {2:.2e} nats at log f = {3:.1f} '
                  '(bound {4:.2e})'.format(b, th[b, 0], d, ref[b][0], WIDE_REL * abs(ref[b][0])))
            assert abs(mixed[0][b] - ref[b][0]) <= WIDE_REL * max(1.0, abs(ref[b][0]))
            assert abs(mixed[3][b] - ref[b][1]) <= WIDE_REL * max(1.0, abs(ref[b][1]))
    print('N130-S64-B9 wide and narrow: wide chains {0:.2e} narrow {1:.2e} nats (5e-4)'
          .format(worst[True], worst[False]))
    assert worst[False] <= TOL


def test_panel_forms_at_nine_chains(nat, monkeypatch):
    """N = 2048, B = 9, after test_panel_forms_are_batch_independent: eight chains on the
    explicit-inverse panel with a ninth like them (the compact form), and the same eight with a
    walking chain (theta_0 = 12: the flagged form). The eight chains' statuses, op counts, modes
    and estimates are bitwise the same in both."""
    X, y, thetas, ns = _mixed_case(n=2048)
    rng = np.random.RandomState(11)
    eight = thetas[np.arange(8) % 3] + rng.uniform(-0.2, 0.2, size=(8, thetas.shape[1]))
    ninth = thetas[1] + rng.uniform(-0.2, 0.2, size=thetas.shape[1])
    walker = np.r_[12.0, thetas[1, 1:]]
    oc, sc, nc, fc, _ = _run_is_stats(nat, X, y, np.vstack([eight, ninth]), ns, monkeypatch)
    of, sf, nf, ff, _ = _run_is_stats(nat, X, y, np.vstack([eight[:4], walker, eight[4:]]), ns,
                                      monkeypatch)
    assert not sc.any()
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    np.testing.assert_array_equal(sf[keep], sc[:8])
    np.testing.assert_array_equal(nf[keep], nc[:8])
    np.testing.assert_array_equal(of[keep], oc[:8])
    for q, k in enumerate(keep):
        np.testing.assert_array_equal(ff[k], fc[q])
    assert len(set(oc)) == 9


# ----------------------------------------------------------------------------- D. the sampler

def test_async_sampler_at_eleven_chains(nat):
    """BatchedAPMEllSSPlusRandDirSliceSampler (the class bench.py runs), 11 chains, N = 130,
    S = 64, six transitions per chain on the asynchronous schedule: chains 0, 5 and 10 have
    bitwise the trajectory of the same chain run alone with first_chain=; loo(psis=True) rows of
    those chains are ISLeaveOneOut(psis=True)'s on the downloaded (theta, u); and the u-calls
    issued had the batch counts printed below, among them counts >= 8 that are no multiple of 8.
    Measured on an MI355X with seed 31, the first tried: u-calls of 1 (19 of them), 2 (3), 3 (2),
    4, 5, 7 (4), 8 and 11 chains, theta-calls of 1, 2, 3, 5, 6, 7 and 11 (7); all comparisons
    exact."""
    import gpdemo.kernels as krn
    from auxpm.batched import BatchedAPMEllSSPlusRandDirSliceSampler as Sampler
    from gpdemo.loo import ISLeaveOneOut
    c = _make_case(130, 5, 70, 'ard', 100)
    prior = dict(a_tau=1., b_tau=1. / 5 ** 0.5, a_sigma=1.1, b_sigma=0.1)
    C, pick = 11, (0, 5, 10)
    th0 = np.tile(np.r_[0.0, np.full(5, np.log(2.))], (C, 1))
    th0[:, 0] = np.linspace(-0.5, 1.0, C)

    def run(n_chains, first):
        smp = Sampler(c['X'], c['y'], n_chains, 64, prior, seed=31, first_chain=first)
        smp.initialise(th0[first:first + n_chains])
        traces, done = smp.run_async(6)
        assert (done == 6).all() and not smp.failed.any()
        return smp, np.array(traces)
    smp, tr = run(C, 0)
    try:
        rows = smp.loo(psis=True)
        us = np.stack([smp.ctx.u_download(smp.ub_u[q]) for q in pick])
        theta, log_f = smp.theta.copy(), smp.log_f.copy()
        u_counts = dict(smp.ctx.batch_hist['u'])
        t_counts = dict(smp.ctx.batch_hist['theta'])
    finally:
        smp.ctx.close()
    print('u-call batch counts {0}; theta-call batch counts {1}'.format(
        sorted(u_counts.items()), sorted(t_counts.items())))
    assert any(k >= 8 and k % 8 for k in u_counts), u_counts
    assert len(u_counts) >= 3
    for q, ch in enumerate(pick):
        one, tr1 = run(1, ch)
        try:
            np.testing.assert_array_equal(tr[ch], tr1[0])
            np.testing.assert_array_equal(theta[ch], one.theta[0])
            assert log_f[ch] == one.log_f[0]
            np.testing.assert_array_equal(us[q], one.ctx.u_download(one.ub_u[0]))
        finally:
            one.ctx.close()
    p = ISLeaveOneOut(c['X'], c['y'], krn.make_kernel_func('ard', EPS), 64, max_batch=4)
    try:
        out = p(theta[list(pick)], us=us, psis=True)
    finally:
        p.close()
    assert not out['status'].any()
    for k in ('loo', 'lpd', 'ess_loo', 'gauss', 'ess', 'loo_psis', 'khat', 'khat_w'):
        np.testing.assert_array_equal(rows[k][list(pick)], out[k])
