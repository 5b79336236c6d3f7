"""Leave-one-out predictive densities from the importance samples on the device (apm_is_loo;
is_loo.hip, host_is_loo.cpp) against the numpy restatement
(is_loo_restatement.py) on the C oracle's Gram, plus what needs no restatement: one-sample
contexts, log f bitwise apm_u_eval's, batch independence, that the call leaves every other path's
bits alone, padding, refusals and failures, and the batched sampler's loo()."""
import math

import numpy as np
import pytest

import is_loo_restatement as ilr
from test_gpu_ep import kind_code
from test_gpu_is_predict import _draws, _est, _fit, _grams
from test_gpu_predict import _make_case

pytestmark = pytest.mark.gpu

EPS = 1e-8
# loo, lpd and log ess_loo: 2 delta with delta = 5e-4 nats, the project's tolerance on the log
# weights that ride on the fp32 C_chol.U - a relative weight change delta moves a
# ratio of positive weighted sums by at most 2 delta (§19's argument) - plus ten times the case's
# fp32 yardstick Y: the restatement with C_chol and U rounded through float32 against itself
W_TOL = 1e-3
# gauss: ten times what a relative change of 2.4e-7 in C_ii (two fp32 roundings of a squared
# factor entry, as rowq is formed from the fp32 bottom block) moves it, floored
G_FLOOR, G_REL = 1e-9, 2.4e-7

# (name, n, d, m, kind, theta index, S, seed): test_gpu_is_predict's inputs (m enters the data's
# random stream only) with theta_0 = 0.3, 3, -1. One tile of samples, a padded second one, three
CASES = [('130x5', 130, 5, 70, 'ard', t, S, 100) for S in (64, 100, 130) for t in range(3)] + \
        [('200x3', 200, 3, 70, 'iso', 0, 64, 102), ('N65', 65, 4, 70, 'ard', 0, 64, 365),
         ('N513', 513, 4, 1, 'ard', 1, 64, 813), ('N577', 577, 4, 70, 'ard', 2, 64, 877)]
# (case index, proposal, likelihood) of every parity run
RUNS = [(i, 'laplace', 'probit') for i in range(len(CASES))] + \
       [(i, 'ep', 'probit') for i in (0, 1, 2, 6, 10)] + \
       [(i, 'laplace', 'logit') for i in (0, 1, 2, 3)]
WIDE_RUNS = [i for i, r in enumerate(RUNS) if r[0] < 9]  # the (130, 5) cases


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _r32(a):
    return a.astype(np.float32).astype(np.float64)


def _gauss_bound(y, slot, lik):
    f, W, z, C_chol, _ = slot
    cd = (C_chol * C_chol).sum(1)
    g0 = ilr.cavity(y, f, W, z, cd, lik)['gauss']
    g1 = ilr.cavity(y, f, W, z, cd * (1.0 + G_REL), lik)['gauss']
    return G_FLOOR + 10.0 * np.abs(g1 - g0)


@pytest.fixture(scope='module')
def refs():
    """Per run: the case, the restatement on the oracle's fit (tau > 0 asserted at every point),
    its fp32 yardstick Y and the gauss bound, computed once and left unchanged."""
    data, out = {}, []
    for i, prop, lik in RUNS:
        name, n, d, m, kind, t, S, seed = CASES[i]
        if (n, d, m, kind, seed) not in data:
            data[n, d, m, kind, seed] = _make_case(n, d, m, kind, seed)
        c = data[n, d, m, kind, seed]
        th = c['thetas'][t]
        K, _ = _grams(c, None, th)
        U = _draws(n, S, seed + 7)
        slot = ilr.slot_of(_fit(K, c['y'], prop, lik))
        ref = ilr.loo_quantities(c['y'], *slot, U, lik)
        r32 = ilr.loo_quantities(c['y'], slot[0], slot[1], slot[2], _r32(slot[3]), slot[4],
                                 _r32(U), lik)
        Y = max(float(np.abs(r32[k] - ref[k]).max()) for k in ('loo', 'lpd'))
        Y = max(Y, float(np.abs(np.log(r32['ess_loo'] / ref['ess_loo'])).max()))
        out.append(dict(c=c, th=th, U=U, ref=ref, Y=Y, S=S, kind=kind,
                        gbound=_gauss_bound(c['y'], slot, lik),
                        label='{0} theta_0 {1} S {2} {3}/{4}'.format(name, th[0], S, prop, lik)))
    return out


def _compare(nat, r, run):
    _, prop, lik = run
    c, ref = r['c'], r['ref']
    ctx = nat.Context(c['X'], c['y'], kind_code(nat, r['kind']), EPS, r['S'], max_batch=1,
                      n_slots=1, n_ubufs=1, likelihood=lik)
    try:
        ctx.u_upload(0, r['U'])
        logf0, st0, _ = ctx.theta_eval(_est(nat, prop), r['th'][None], [0], [0])
        logf, loo, lpd, ess_loo, gauss, ess, st = ctx.is_loo([0], [0])
    finally:
        ctx.close()
    assert st0[0] == 0 and st[0] == 0
    bound = W_TOL + 10.0 * r['Y']
    d_loo = float(np.abs(loo[0] - ref['loo']).max())
    d_lpd = float(np.abs(lpd[0] - ref['lpd']).max())
    d_ess = float(np.abs(np.log(ess_loo[0] / ref['ess_loo'])).max())
    d_g = np.abs(gauss[0] - ref['gauss'])
    print('{0}: d loo {1:.2e} d lpd {2:.2e} d log ess_loo {3:.2e} (Y {4:.1e}, bound {5:.2e}) '
          'd gauss {6:.2e} (worst ratio to its bound {7:.2f}) min tau {8:.3g} sum loo {9:.2f} '
          'sum gauss {10:.2f} sum lpd {11:.2f}'.format(
              r['label'], d_loo, d_lpd, d_ess, r['Y'], bound, d_g.max(),
              (d_g / r['gbound']).max(), ref['tau'].min(), loo[0].sum(), gauss[0].sum(),
              lpd[0].sum()))
    assert d_loo <= bound and d_lpd <= bound and d_ess <= bound
    assert np.all(d_g <= r['gbound']), (d_g / r['gbound']).max()
    assert np.all(lpd[0] >= loo[0] - 1e-12)
    assert np.all((ess_loo[0] >= 1.0) & (ess_loo[0] <= r['S'] * (1 + 1e-12)))
    assert abs(ess[0] / ref['ess'] - 1.0) <= W_TOL
    assert abs(logf[0] - ref['logf']) <= W_TOL


@pytest.mark.parametrize('ri', range(len(RUNS)))
def test_loo_vs_restatement(nat, refs, ri):
    """loo, lpd, log ess_loo and gauss against the restatement on the oracle's fit; lpd >= loo at
    every point. Measured on an MI355X (DESIGN.md §23 has every case): worst d loo 2.13e-06
    (N = 513), d lpd 8.74e-07, d log ess_loo 2.81e-06, with Y between 8e-09 and 2.9e-07; gauss at
    most 0.51 of its bound (N = 513; 0.05 to 0.26 elsewhere)."""
    _compare(nat, refs[ri], RUNS[ri])


@pytest.mark.parametrize('ri', WIDE_RUNS)
def test_wide_twin_vs_restatement(nat, refs, ri, monkeypatch):
    """The (130, 5) cases with APM_WIDE_Q=0: every slot wide, k_is_loo_gemm64 on the fp64 factor and
    the fp64 U buffer. The same bounds. Measured on an MI355X: d loo at most 4.23e-07, d lpd
    2.17e-07, d log ess_loo 5.12e-07, d gauss 5.66e-11 (rowq comes from the fp64 factor there)."""
    monkeypatch.setenv('APM_WIDE_Q', '0')
    _compare(nat, refs[ri], RUNS[ri])


@pytest.mark.parametrize('likelihood', ['probit', 'logit'])
@pytest.mark.parametrize('n,d', [(1, 1), (64, 4), (65, 4), (130, 5), (577, 4)])
def test_one_sample_contexts(nat, n, d, likelihood):
    """S = 1, so wbar = 1: ess_loo = 1 exactly, loo_i = lpd_i bitwise, and both are
    log p(y_i | f_1i) of the restatement fed the slot's read-back factor (already fp32) and the
    fp32-rounded u, within 1e-3 + 10 Y with Y the product's fp32 yardstick: the same rows with
    the product accumulated in float32 against float64. Measured on an MI355X: d loo between
    1.3e-08 (N = 1) and 4.98e-07 (N = 577, where Y is 2.4e-07)."""
    c = _make_case(n, d, 1, 'ard', 400 + n)
    u = _draws(n, 1, 17 + n)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 1, max_batch=1, n_slots=1, n_ubufs=1,
                      likelihood=likelihood)
    try:
        ctx.u_upload(0, u)
        _, st0, _ = ctx.theta_eval(nat.EST_IS, c['thetas'][:1], [0], [0])
        logf, loo, lpd, ess_loo, gauss, ess, st = ctx.is_loo([0], [0])
        L, f_post, _, _ = ctx.slot_read(0)
    finally:
        ctx.close()
    assert st0[0] == 0 and st[0] == 0
    assert np.all(ess_loo[0] == 1.0) and ess[0] == 1.0
    np.testing.assert_array_equal(loo[0], lpd[0])
    ref = ilr.log_lik(c['y'] * (f_post + L.dot(u[:, 0])), likelihood)
    f32 = f_post + (L.astype(np.float32).dot(u[:, 0].astype(np.float32))).astype(np.float64)
    Y = float(np.abs(ilr.log_lik(c['y'] * f32, likelihood) - ref).max())
    err = float(np.abs(loo[0] - ref).max())
    print('n {0} {1}: d loo {2:.2e} Y {3:.1e}'.format(n, likelihood, err, Y))
    assert err <= W_TOL + 10.0 * Y
    assert np.isfinite(gauss[0]).all()


def _three(nat, S=100, seeds=(21, 22, 23)):
    """(case, context, theta-call results): three thetas of (130, 5) in slots 0..2 with device
    draws in buffers 0..2."""
    c = _make_case(130, 5, 70, 'ard', 100)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, S, max_batch=4, n_slots=4, n_ubufs=4)
    ctx.u_normal([0, 1, 2], list(seeds), [0, 0, 0])
    idx = np.arange(3)
    first = ctx.theta_eval(nat.EST_IS, c['thetas'], idx, idx)
    assert not first[1].any()
    return c, ctx, first


def test_bitwise_properties(nat):
    """log f is apm_u_eval's; U buffers, slot read-backs, a following u-call and a following IS
    theta-call are unchanged; a chain has the same bits alone, first of 3 and last of 4; and with
    S = 100 every output equals that of a second context whose U buffers were filled by upload
    instead of by apm_u_normal (the padded columns add nothing)."""
    c, ctx, first = _three(nat)
    idx = np.arange(3)
    try:
        U0 = [ctx.u_download(q) for q in range(3)]
        slots0 = [ctx.slot_read(q) for q in range(3)]
        ue0 = ctx.u_eval(idx, idx)
        allthree = ctx.is_loo(idx, idx)
        alone = [ctx.is_loo([q], [q]) for q in range(3)]
        first3 = [ctx.is_loo([q, (q + 1) % 3, (q + 2) % 3], [q, (q + 1) % 3, (q + 2) % 3])
                  for q in range(3)]
        last4 = [ctx.is_loo([(q + 1) % 3, (q + 2) % 3, (q + 1) % 3, q],
                            [(q + 1) % 3, (q + 2) % 3, (q + 1) % 3, q]) for q in range(3)]
        U1 = [ctx.u_download(q) for q in range(3)]
        slots1 = [ctx.slot_read(q) for q in range(3)]
        ue1 = ctx.u_eval(idx, idx)
        again = ctx.theta_eval(nat.EST_IS, c['thetas'], idx, idx)
    finally:
        ctx.close()
    assert not allthree[6].any()
    np.testing.assert_array_equal(allthree[0], ue0[0])
    for a, b in zip(ue0 + first, ue1 + again):
        np.testing.assert_array_equal(a, b)
    for q in range(3):
        np.testing.assert_array_equal(U0[q], U1[q])
        for a, b in zip(slots0[q], slots1[q]):
            np.testing.assert_array_equal(a, b)
        for k in range(7):
            np.testing.assert_array_equal(allthree[k][q], alone[q][k][0])
            np.testing.assert_array_equal(allthree[k][q], first3[q][k][0])
            np.testing.assert_array_equal(allthree[k][q], last4[q][k][3])
    assert np.isfinite(allthree[1]).all() and len(set(allthree[1][:, 0])) == 3
    ctx2 = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 100, max_batch=4, n_slots=4,
                       n_ubufs=4)
    try:
        for q in range(3):
            ctx2.u_upload(q, U0[q])
        st2 = ctx2.theta_eval(nat.EST_IS, c['thetas'], idx, idx)[1]
        uploaded = ctx2.is_loo(idx, idx)
    finally:
        ctx2.close()
    assert not st2.any()
    for a, b in zip(allthree, uploaded):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('likelihood', ['probit', 'logit'])
def test_ess_and_logf_are_is_predicts_bitwise(nat, likelihood):
    """apm_is_predict forms the weights and apm_is_loo their logarithms from one text
    (csrc/is_weights.h): ess = 1 / sum wbar_s^2 is one value bitwise, and so is log f. N = 65 (two
    row blocks: the ascending per-sample sum has two terms) and n_imp = 100 (a padded sample tile,
    threads that own no sample), three chains."""
    c = _make_case(65, 4, 5, 'ard', 365)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 100, max_batch=3, n_slots=3, n_ubufs=3,
                      likelihood=likelihood)
    idx = np.arange(3)
    try:
        ctx.u_normal(idx, [41, 42, 43], [0, 0, 0])
        logf_p, _, _, _, ess_p, st_p, _ = ctx.is_predict(nat.EST_IS, c['thetas'], idx, idx, c['Xs'])
        logf_l, _, _, _, _, ess_l, st_l = ctx.is_loo(idx, idx)
    finally:
        ctx.close()
    assert not st_p.any() and not st_l.any()
    assert np.isfinite(ess_p).all() and np.all((ess_p >= 1.0) & (ess_p <= 100.0))
    np.testing.assert_array_equal(ess_l, ess_p)
    np.testing.assert_array_equal(logf_l, logf_p)


def test_priormc_slots_are_accepted(nat):
    """A PriorMC slot (W = z = 0, factor chol(K)): loo is the prior-proposal estimate and gauss
    the prior predictive, log Phi(0) = log 1/2 at every point of a zero-mean prior."""
    c = _make_case(130, 5, 70, 'ard', 100)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 64, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        ctx.u_normal([0], [5], [0])
        lf, st0, _ = ctx.theta_eval(nat.EST_PRIORMC, c['thetas'][:1], [0], [0])
        logf, loo, lpd, ess_loo, gauss, ess, st = ctx.is_loo([0], [0])
    finally:
        ctx.close()
    assert st0[0] == 0 and st[0] == 0 and logf[0] == lf[0]
    np.testing.assert_allclose(gauss[0], math.log(0.5), rtol=0, atol=1e-12)
    assert np.all(lpd[0] >= loo[0] - 1e-12) and np.isfinite(loo).all()
    assert np.all((ess_loo[0] >= 1.0) & (ess_loo[0] <= 64.0 * (1 + 1e-12)))


def test_refusals_and_failed_slots(nat):
    """Every APM_E_INVALID case leaves its outputs untouched; a slot failed by max_iters = 2 gives
    apm_u_eval's status and NaN everywhere, while the chain beside it keeps the bits it has
    alone."""
    c, ctx, _ = _three(nat, S=64)
    lib, h, n = ctx.lib, ctx._h, 130
    idx = np.array([0, 1], dtype=np.int64)
    bad_idx = np.array([0, 4], dtype=np.int64)
    rows = [np.full((2, n), 7.0) for _ in range(4)]
    logf, ess = np.full(2, 7.0), np.full(2, 7.0)
    st = np.full(2, 9, dtype=np.int32)

    def call(count=2, sl=idx, ub=idx, ldo=n, status=st, rowp=None, handle=h):
        rp = [r.ctypes.data for r in rows] if rowp is None else rowp
        return lib.apm_is_loo(handle, count, None if sl is None else sl.ctypes.data,
                              None if ub is None else ub.ctypes.data, logf.ctypes.data, rp[0],
                              rp[1], rp[2], rp[3], ldo,
                              ess.ctypes.data, None if status is None else status.ctypes.data)
    try:
        bad = [call(count=0), call(count=5), call(sl=None), call(ub=None), call(status=None),
               call(sl=bad_idx), call(ub=bad_idx), call(sl=-idx - 1), call(ldo=n - 1),
               call(ldo=n - 1, rowp=[None, None, None, rows[3].ctypes.data]), call(handle=None)]
        assert bad == [nat.APM_E_INVALID] * len(bad)
        assert all((r == 7.0).all() for r in rows + [logf, ess]) and (st == 9).all()
        # ldo is not read when no row output is asked for; every output but status may be NULL
        assert call(ldo=0, rowp=[None] * 4) == 0 and not st.any()
        assert lib.apm_is_loo(h, 2, idx.ctypes.data, idx.ctypes.data, None, None, None, None,
                              None, 0, None, st.ctypes.data) == 0
        alone = ctx.is_loo([1], [1])
        ctx.set_newton(1e-4, 2)
        _, fst, _ = ctx.theta_eval(nat.EST_IS, c['thetas'][1:2], [0], [0])  # theta_0 = 3
        assert fst[0] == nat.STATUS_MAXITER
        ref_st = ctx.u_eval([0, 1], [0, 1])[1]
        both = ctx.is_loo([0, 1], [0, 1])
    finally:
        ctx.close()
    np.testing.assert_array_equal(both[6], ref_st)
    for k in range(6):
        assert np.isnan(both[k][0]).all()
        np.testing.assert_array_equal(both[k][1], alone[k][0])
    assert np.isfinite(alone[1]).all()


def test_batched_sampler_loo(nat):
    """BatchedAPMEllSSPlusMHSampler, 4 chains, N = 130, S = 64: six steps with loo() after every
    step give bitwise the theta and log f trajectories of six steps without it, and the returned
    rows are ISLeaveOneOut's on the downloaded (theta, u), bitwise."""
    import gpdemo.kernels as krn
    from auxpm.batched import BatchedAPMEllSSPlusMHSampler
    from gpdemo.loo import ISLeaveOneOut, combine_loo
    c = _make_case(130, 5, 70, 'ard', 100)
    prior = dict(a_tau=1., b_tau=1. / 5 ** 0.5, a_sigma=1.1, b_sigma=0.1)
    th0 = np.tile(np.r_[0.0, np.full(5, np.log(2.))], (4, 1))

    def run(with_loo):
        smp = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 4, 64, prior, prop_scales=0.1, seed=31)
        smp.initialise(th0)
        trace, rows = [], []
        for _ in range(6):
            smp.step()
            if with_loo:
                rows.append(smp.loo())
            trace.append((smp.theta.copy(), smp.log_f.copy()))
        return smp, trace, rows
    plain, t0, _ = run(False)
    plain.ctx.close()
    smp, t1, rows = run(True)
    try:
        for (tha, lfa), (thb, lfb) in zip(t0, t1):
            np.testing.assert_array_equal(tha, thb)
            np.testing.assert_array_equal(lfa, lfb)
        assert not smp.failed.any() and rows[-1]['loo'].shape == (4, 130)
        us = np.stack([smp.ctx.u_download(smp.ub_u[q]) for q in range(4)])
        theta = smp.theta.copy()
    finally:
        smp.ctx.close()
    p = ISLeaveOneOut(c['X'], c['y'], krn.make_kernel_func('ard', EPS), 64, max_batch=4)
    try:
        out = p(theta, us=us)
        a, b = p(theta[:2], seeds=[7, 8]), p(theta[:2], seeds=[7, 8])
    finally:
        p.close()
    assert not out['status'].any()
    for k in ('loo', 'lpd', 'ess_loo', 'gauss', 'ess'):
        np.testing.assert_array_equal(rows[-1][k], out[k])
        np.testing.assert_array_equal(a[k], b[k])
    # chain 0's rows over the run, combined as the docstring of loo() says
    crit = combine_loo(np.stack([r['loo'][0] for r in rows]),
                       np.stack([r['lpd'][0] for r in rows]), burn=1)
    assert np.isfinite(crit['elpd_loo']) and crit['p_loo'] >= 0.0 and crit['se'] > 0.0
    other = BatchedAPMEllSSPlusMHSampler(c['X'], c['y'], 2, 8, prior, prop_scales=0.1, seed=1,
                                         estimator='laplace')
    try:
        with pytest.raises(ValueError):
            other.loo()
    finally:
        other.ctx.close()
