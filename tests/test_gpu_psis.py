"""Pareto-smoothed leave-one-out densities and the Pareto k-hat on the device (apm_is_loo_psis;
is_psis.hip, host_is_psis.cpp).

A. the stored log ratios against the restatement's log wbar - log p (is_loo_restatement.py on the C
   oracle's Gram), under §23's bound; B. loo_psis, khat and khat_w against the numpy statement of
   the steps (psis_restatement.py) applied to the device's own log ratios and log weights, fp64
   against fp64; C. agreement with apm_is_loo; D. batch independence, NULL outputs and that the
   call disturbs no other path; E. refusals and failed slots; F. the batched sampler's
   loo(psis=True). Two mutations of the restatement show that B sees what it should."""
import numpy as np
import pytest
from scipy.special import logsumexp

import is_loo_restatement as ilr
import psis_restatement as pr
from test_gpu_ep import kind_code
from test_gpu_is_loo import CASES, EPS, W_TOL, _r32, _three
from test_gpu_is_predict import _draws, _est, _fit, _grams
from test_gpu_predict import _make_case

pytestmark = pytest.mark.gpu

# B's bound: both sides are fp64 on identical inputs
B_TOL = 1e-8
# (case index of test_gpu_is_loo.CASES, proposal, likelihood): (130, 5) with S = 64, 100, 130 at
# the three thetas and (65, 4) with S = 64 under Laplace / probit; S = 64 at the three thetas
# under EP / probit and Laplace / logit
RUNS = [(i, 'laplace', 'probit') for i in list(range(9)) + [10]] + \
       [(i, 'ep', 'probit') for i in (0, 1, 2)] + [(i, 'laplace', 'logit') for i in (0, 1, 2)]
WIDE_RUNS = [0, 1, 2, 3, 6, 10, 13]  # one per (S, theta at S = 64) and per proposal / likelihood
SMALL_S = [4, 24, 25]  # (8, 2): M = 0, 4 (no fit) and 5 (the smallest fit)


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _ratios(q):
    with np.errstate(invalid='ignore'):
        lwbar = q['lw'] - logsumexp(q['lw'])
        return lwbar[None] - q['lp'], lwbar


@pytest.fixture(scope='module')
def refs():
    """Per run: the case and the restatement's log ratios t = log wbar - log p (n, S) with their
    fp32 yardstick Y (the same with C_chol and U rounded through float32, against itself),
    computed once and left unchanged."""
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
        tref, lwbar = _ratios(ilr.loo_quantities(c['y'], *slot, U, lik))
        t32, _ = _ratios(ilr.loo_quantities(c['y'], slot[0], slot[1], slot[2], _r32(slot[3]),
                                            slot[4], _r32(U), lik))
        assert np.isfinite(tref).all() and np.isfinite(t32).all()
        out.append(dict(c=c, th=th, U=U, t=tref, lwbar=lwbar, Y=float(np.abs(t32 - tref).max()),
                        S=S, kind=kind,
                        label='{0} theta_0 {1} S {2} {3}/{4}'.format(name, th[0], S, prop, lik)))
    return out


def _device(nat, c, kind, th, U, S, prop, lik):
    """One chain: theta-call, apm_is_loo, apm_is_loo_psis with the log ratios, and the device's
    own log weights (apm_u_eval_diag with blocks of one sample: a block's estimate is its
    sample's log w_s), normalised."""
    ctx = nat.Context(c['X'], c['y'], kind_code(nat, kind), EPS, S, max_batch=1, n_slots=1,
                      n_ubufs=1, likelihood=lik)
    try:
        ctx.u_upload(0, U)
        _, st0, _ = ctx.theta_eval(_est(nat, prop), th[None], [0], [0])
        loo = ctx.is_loo([0], [0])
        ps = ctx.is_loo_psis([0], [0], want_logratio=True)
        lw = ctx.u_eval_diag([0], [0], block=1)[0][0]
    finally:
        ctx.close()
    assert st0[0] == 0 and loo[6][0] == 0 and ps[5][0] == 0
    return dict(loo=loo, ps=ps, lwbar=lw - logsumexp(lw))


def _check_B(dev, label, **mut):
    """loo_psis, khat and khat_w against the restatement on the device's own log ratios and log
    weights: the three largest differences (NaN must meet NaN)."""
    logf, loo_psis, khat, khat_w, lr, st = dev['ps']
    r_loo, r_khat = pr.psis_rows(lr[0], **mut)
    _, r_kw, _ = pr.psis_row(dev['lwbar'], **mut)
    assert np.array_equal(np.isnan(khat[0]), np.isnan(r_khat)), label
    fit = ~np.isnan(r_khat)
    d_loo = float(np.abs(loo_psis[0] - r_loo).max())
    d_k = float(np.abs(khat[0][fit] - r_khat[fit]).max()) if fit.any() else 0.0
    d_kw = 0.0 if np.isnan(r_kw) and np.isnan(khat_w[0]) else abs(khat_w[0] - r_kw)
    return d_loo, d_k, float(d_kw)


def _compare(nat, r, run):
    _, prop, lik = run
    dev = _device(nat, r['c'], r['kind'], r['th'], r['U'], r['S'], prop, lik)
    logf, loo_psis, khat, khat_w, lr, st = dev['ps']
    # A
    bound = W_TOL + 10.0 * r['Y']
    assert np.array_equal(np.isneginf(lr[0]), np.isneginf(r['t']))
    d_t = float(np.abs(lr[0] - r['t']).max())
    d_w = float(np.abs(dev['lwbar'] - r['lwbar']).max())
    # B
    d_loo, d_k, d_kw = _check_B(dev, r['label'])
    # C
    d_raw = float(np.abs(-logsumexp(lr[0], axis=1) - dev['loo'][1][0]).max())
    print('{0}: A d t {1:.2e} d lwbar {2:.2e} (Y {3:.1e}, bound {4:.2e}) B d loo_psis {5:.2e} '
          'd khat {6:.2e} d khat_w {7:.2e} C d raw {8:.2e} | khat median {9:.2f} max {10:.2f} '
          'above 0.7: {11} of {12}, khat_w {13:.2f}, largest loo - loo_psis {14:.2f}'.format(
              r['label'], d_t, d_w, r['Y'], bound, d_loo, d_k, d_kw, d_raw, np.median(khat[0]),
              khat[0].max(), int((khat[0] > 0.7).sum()), khat.shape[1], khat_w[0],
              float(np.abs(dev['loo'][1][0] - loo_psis[0]).max())))
    assert d_t <= bound and d_w <= bound
    assert np.isfinite(khat).all() and np.isfinite(khat_w).all() and np.isfinite(loo_psis).all()
    assert d_loo <= B_TOL and d_k <= B_TOL and d_kw <= B_TOL
    assert d_raw <= 1e-12
    np.testing.assert_array_equal(logf, dev['loo'][0])
    np.testing.assert_array_equal(st, dev['loo'][6])
    # the cap: no smoothed ratio exceeds the row's largest raw one
    assert np.all(loo_psis[0] >= -(lr[0].max(axis=1) + np.log(r['S'])) - 1e-12)
    return dev


@pytest.mark.parametrize('ri', range(len(RUNS)))
def test_psis_vs_restatement(nat, refs, ri):
    """A, B and C on every run. Measured on an MI355X (DESIGN.md §24 has every case): A at most
    1.19e-5 (theta_0 = 3, S = 130; Y 2.0e-6, bound 1.02e-3); B at most 9.99e-15 (loo_psis), 1.69e-14
    (khat), 6.7e-16 (khat_w) against the bound 1e-8; C at most 8.9e-16 against 1e-12."""
    _compare(nat, refs[ri], RUNS[ri])


@pytest.mark.parametrize('ri', WIDE_RUNS)
def test_wide_twin_vs_restatement(nat, refs, ri, monkeypatch):
    """The same with APM_WIDE_Q=0: every slot wide, k_psis_gemm64 on the fp64 factor and the fp64
    U buffer. The same bounds."""
    monkeypatch.setenv('APM_WIDE_Q', '0')
    _compare(nat, refs[ri], RUNS[ri])


def test_mutations_are_caught(nat, refs):
    """B with the restatement mutated - the tail one longer, the prior term of khat dropped - on
    (130, 5) theta_0 = 0.3 at S = 64 and S = 130: every mutation moves khat and loo_psis past
    the bound, so B checks the tail size and the prior, not only the plumbing."""
    for ri in (0, 6):
        r = refs[ri]
        dev = _device(nat, r['c'], r['kind'], r['th'], r['U'], r['S'], 'laplace', 'probit')
        assert max(_check_B(dev, r['label'])) <= B_TOL
        for mut in (dict(tail_shift=1), dict(tail_shift=-1), dict(drop_prior=True)):
            d_loo, d_k, d_kw = _check_B(dev, r['label'], **mut)
            print('{0} {1}: d loo_psis {2:.2e} d khat {3:.2e} d khat_w {4:.2e}'.format(
                r['label'], mut, d_loo, d_k, d_kw))
            assert d_loo > B_TOL and d_k > B_TOL and d_kw > B_TOL


@pytest.mark.parametrize('likelihood', ['probit', 'logit'])
@pytest.mark.parametrize('S', SMALL_S)
def test_short_tails(nat, S, likelihood):
    """(8, 2): at S = 4 and S = 24 (M = 0 and 4) khat and khat_w are NaN and loo_psis equals
    apm_is_loo's loo within 1e-12; at S = 25 (M = 5) the fit runs, khat is finite and B holds."""
    c = _make_case(8, 2, 70, 'ard', 108)
    dev = _device(nat, c, 'ard', c['thetas'][0], _draws(8, S, 115 + S), S, 'laplace', likelihood)
    logf, loo_psis, khat, khat_w, lr, st = dev['ps']
    assert pr.tail_size(S) == {4: 0, 24: 4, 25: 5}[S]
    assert float(np.abs(-logsumexp(lr[0], axis=1) - dev['loo'][1][0]).max()) <= 1e-12
    np.testing.assert_array_equal(logf, dev['loo'][0])
    if S < 25:
        assert np.isnan(khat).all() and np.isnan(khat_w).all()
        assert float(np.abs(loo_psis[0] - dev['loo'][1][0]).max()) <= 1e-12
    else:
        assert np.isfinite(khat).all() and np.isfinite(khat_w).all()
    d = _check_B(dev, 'S {0}'.format(S))
    print('S {0} {1}: B {2}'.format(S, likelihood, d))
    assert max(d) <= B_TOL


@pytest.mark.parametrize('S', [1024, 4096])
def test_long_rows(nat, S):
    """(8, 2) at S = 1024 and at the cap S = 4096 (M = 96 and 192, the largest tail): the row is
    longer than the workgroup, so the strided loads and the sort's comparators take 2 and 8
    iterations per thread, and the grid's lanes 2 and 3 elements. B and C hold and every khat is
    finite."""
    c = _make_case(8, 2, 70, 'ard', 108)
    dev = _device(nat, c, 'ard', c['thetas'][0], _draws(8, S, 115 + S), S, 'laplace', 'probit')
    logf, loo_psis, khat, khat_w, lr, st = dev['ps']
    assert pr.tail_size(S) == {1024: 96, 4096: 192}[S]
    d_raw = float(np.abs(-logsumexp(lr[0], axis=1) - dev['loo'][1][0]).max())
    d = _check_B(dev, 'S {0}'.format(S))
    print('S {0}: B {1} C {2:.2e} khat {3} khat_w {4:.3f}'.format(S, d, d_raw, khat[0], khat_w[0]))
    assert np.isfinite(khat).all() and np.isfinite(khat_w).all() and np.isfinite(loo_psis).all()
    assert max(d) <= B_TOL and d_raw <= 1e-12
    np.testing.assert_array_equal(logf, dev['loo'][0])


def test_bitwise_properties(nat):
    """A chain has the same bits alone, first of 3 and last of 4, and twice in one batch; log f
    and status are apm_is_loo's; a call between two apm_is_loo / apm_u_eval / theta-calls leaves
    their outputs, the U buffers and the slots bitwise unchanged (S = 100: a padded tile)."""
    c, ctx, first = _three(nat)
    idx = np.arange(3)
    try:
        U0 = [ctx.u_download(q) for q in range(3)]
        slots0 = [ctx.slot_read(q) for q in range(3)]
        ue0 = ctx.u_eval(idx, idx)
        loo0 = ctx.is_loo(idx, idx)
        allthree = ctx.is_loo_psis(idx, idx, want_logratio=True)
        alone = [ctx.is_loo_psis([q], [q], want_logratio=True) for q in range(3)]
        first3 = [ctx.is_loo_psis([q, (q + 1) % 3, (q + 2) % 3], [q, (q + 1) % 3, (q + 2) % 3],
                                  want_logratio=True) for q in range(3)]
        last4 = [ctx.is_loo_psis([(q + 1) % 3, (q + 2) % 3, (q + 1) % 3, q],
                                 [(q + 1) % 3, (q + 2) % 3, (q + 1) % 3, q], want_logratio=True)
                 for q in range(3)]
        twice = ctx.is_loo_psis([1, 1], [1, 1], want_logratio=True)
        loo1 = ctx.is_loo(idx, idx)
        ue1 = ctx.u_eval(idx, idx)
        U1 = [ctx.u_download(q) for q in range(3)]
        slots1 = [ctx.slot_read(q) for q in range(3)]
        again = ctx.theta_eval(nat.EST_IS, c['thetas'], idx, idx)
    finally:
        ctx.close()
    assert not allthree[5].any()
    np.testing.assert_array_equal(allthree[0], ue0[0])
    np.testing.assert_array_equal(allthree[0], loo0[0])
    np.testing.assert_array_equal(allthree[5], loo0[6])
    for a, b in zip(ue0 + first + loo0, ue1 + again + loo1):
        np.testing.assert_array_equal(a, b)
    for q in range(3):
        np.testing.assert_array_equal(U0[q], U1[q])
        for a, b in zip(slots0[q], slots1[q]):
            np.testing.assert_array_equal(a, b)
        for k in range(6):
            np.testing.assert_array_equal(allthree[k][q], alone[q][k][0])
            np.testing.assert_array_equal(allthree[k][q], first3[q][k][0])
            np.testing.assert_array_equal(allthree[k][q], last4[q][k][3])
    for k in range(6):
        np.testing.assert_array_equal(twice[k][0], allthree[k][1])
        np.testing.assert_array_equal(twice[k][1], allthree[k][1])
    assert np.isfinite(allthree[1]).all() and np.isfinite(allthree[2]).all()
    assert len(set(allthree[3])) == 3


def test_priormc_slots_are_accepted(nat):
    """A PriorMC slot (W = z = 0, factor chol(K)): the prior as the proposal. log f is the
    theta-call's, the raw sum of the log ratios is apm_is_loo's loo and B holds."""
    c = _make_case(130, 5, 70, 'ard', 100)
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 64, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        ctx.u_normal([0], [5], [0])
        lf, st0, _ = ctx.theta_eval(nat.EST_PRIORMC, c['thetas'][:1], [0], [0])
        loo = ctx.is_loo([0], [0])
        ps = ctx.is_loo_psis([0], [0], want_logratio=True)
        lw = ctx.u_eval_diag([0], [0], block=1)[0][0]
    finally:
        ctx.close()
    assert st0[0] == 0 and ps[5][0] == 0 and ps[0][0] == lf[0]
    assert float(np.abs(-logsumexp(ps[4][0], axis=1) - loo[1][0]).max()) <= 1e-12
    d = _check_B(dict(ps=ps, lwbar=lw - logsumexp(lw)), 'priormc')
    print('priormc: B {0}, khat median {1:.2f}, khat_w {2:.2f}'.format(
        d, np.nanmedian(ps[2][0]), ps[3][0]))
    assert max(d) <= B_TOL


def _last_error(lib, h):
    return lib.apm_last_error(h)


def test_refusals_and_failed_slots(nat):
    """Every APM_E_INVALID case leaves its outputs untouched and sets the message, byte for byte;
    the context is usable afterwards; every output pointer but status can be NULL in turn; a slot
    failed by max_iters = 2 gives apm_u_eval's status and NaN everywhere, while the chain beside
    it keeps the bits it has alone."""
    c, ctx, _ = _three(nat, S=64)
    lib, h, n, S = ctx.lib, ctx._h, 130, 64
    idx = np.array([0, 1], dtype=np.int64)
    bad_idx = np.array([0, 4], dtype=np.int64)
    rows = [np.full((2, n), 7.0) for _ in range(2)]
    logf, kw, lr = np.full(2, 7.0), np.full(2, 7.0), np.full((2, n * S), 7.0)
    st = np.full(2, 9, dtype=np.int32)

    def call(count=2, sl=idx, ub=idx, ldo=n, ldr=n * S, status=st, outs=None, handle=h):
        o = [logf, rows[0], rows[1], kw, lr] if outs is None else outs
        p = [None if a is None else a.ctypes.data for a in o]
        return lib.apm_is_loo_psis(handle, count, None if sl is None else sl.ctypes.data,
                                   None if ub is None else ub.ctypes.data, p[0], p[1], p[2], ldo,
                                   p[3], p[4], ldr, None if status is None else status.ctypes.data)
    w = b'apm_is_loo_psis: '
    try:
        for kwargs, msg in [
                (dict(count=0), w + b'count outside [1, max_batch]'),
                (dict(count=5), w + b'count outside [1, max_batch]'),
                (dict(sl=None), w + b'bad arguments'), (dict(ub=None), w + b'bad arguments'),
                (dict(status=None), w + b'bad arguments'),
                (dict(sl=bad_idx), b'slot index out of range'),
                (dict(ub=bad_idx), b'ubuf index out of range'),
                (dict(sl=-idx - 1), b'slot index out of range'),
                (dict(ldo=n - 1), w + b'ldo < n'),
                (dict(ldo=n - 1, outs=[None, None, rows[1], None, None]), w + b'ldo < n'),
                (dict(ldr=n * S - 1), w + b'ldr < n*n_imp')]:
            assert call(**kwargs) == nat.APM_E_INVALID
            assert _last_error(lib, h) == msg
        assert call(handle=None) == nat.APM_E_INVALID
        assert lib.apm_global_error() == w + b'null context'
        assert all((r == 7.0).all() for r in rows + [logf, kw, lr]) and (st == 9).all()
        # ldo and ldr are not read when their outputs are not asked for
        assert call(ldo=0, ldr=0, outs=[logf, None, None, kw, None]) == 0 and not st.any()
        full = ctx.is_loo_psis(idx, idx, want_logratio=True)
        for drop in range(5):  # every output but status NULL in turn: the others keep their bits
            bufs = [np.full(2, 7.0), np.full((2, n), 7.0), np.full((2, n), 7.0), np.full(2, 7.0),
                    np.full((2, n * S), 7.0)]
            outs = [None if k == drop else b for k, b in enumerate(bufs)]
            assert call(outs=outs) == 0
            for k in range(5):
                if k != drop:
                    np.testing.assert_array_equal(bufs[k].ravel(), full[k].ravel())
        assert lib.apm_is_loo_psis(h, 2, idx.ctypes.data, idx.ctypes.data, None, None, None, 0,
                                   None, None, 0, st.ctypes.data) == 0
        alone = ctx.is_loo_psis([1], [1], want_logratio=True)
        ctx.set_newton(1e-4, 2)
        _, fst, _ = ctx.theta_eval(nat.EST_IS, c['thetas'][1:2], [0], [0])  # theta_0 = 3
        assert fst[0] == nat.STATUS_MAXITER
        ref_st = ctx.u_eval([0, 1], [0, 1])[1]
        both = ctx.is_loo_psis([0, 1], [0, 1], want_logratio=True)
    finally:
        ctx.close()
    np.testing.assert_array_equal(both[5], ref_st)
    for k in range(5):
        assert np.isnan(both[k][0]).all()
        np.testing.assert_array_equal(both[k][1], alone[k][0])
    assert np.isfinite(alone[1]).all() and np.isfinite(alone[2]).all()


def test_too_many_samples_are_refused(nat):
    """n_imp = 4097 > APM_PSIS_MAX_SAMPLES (n = 2): APM_E_INVALID with the message, nothing
    written, and the context goes on serving apm_is_loo."""
    rng = np.random.RandomState(5)
    X, y = rng.normal(size=(2, 1)), np.array([1.0, -1.0])
    ctx = nat.Context(X, y, nat.KERNEL_ARD, EPS, 4097, max_batch=1, n_slots=1, n_ubufs=1)
    try:
        ctx.u_normal([0], [3], [0])
        _, st0, _ = ctx.theta_eval(nat.EST_IS, np.zeros((1, 2)), [0], [0])
        z = np.zeros(1, dtype=np.int64)
        st, logf = np.full(1, 9, dtype=np.int32), np.full(1, 7.0)
        rc = ctx.lib.apm_is_loo_psis(ctx._h, 1, z.ctypes.data, z.ctypes.data, logf.ctypes.data,
                                     None, None, 0, None, None, 0, st.ctypes.data)
        msg = ctx.lib.apm_last_error(ctx._h)
        with pytest.raises(ValueError):
            ctx.is_loo_psis([0], [0])
        loo = ctx.is_loo([0], [0])
    finally:
        ctx.close()
    assert st0[0] == 0 and rc == nat.APM_E_INVALID and st[0] == 9 and logf[0] == 7.0
    assert msg == b'apm_is_loo_psis: n_imp above APM_PSIS_MAX_SAMPLES'
    assert loo[6][0] == 0 and np.isfinite(loo[1]).all()


def test_batched_sampler_loo_psis(nat):
    """BatchedAPMEllSSPlusMHSampler, 4 chains, N = 130, S = 64: six steps with loo(psis=True)
    after every step give bitwise the theta and log f trajectories of six steps without it; the
    other rows are loo()'s, the extra ones ISLeaveOneOut(psis=True)'s on the downloaded
    (theta, u), bitwise, whose default path is unchanged; combine_loo takes the stacked khat."""
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
                rows.append(smp.loo(psis=True))
            trace.append((smp.theta.copy(), smp.log_f.copy()))
        return smp, trace, rows
    plain, t0, _ = run(False)
    plain.ctx.close()
    smp, t1, rows = run(True)
    try:
        for (tha, lfa), (thb, lfb) in zip(t0, t1):
            np.testing.assert_array_equal(tha, thb)
            np.testing.assert_array_equal(lfa, lfb)
        assert not smp.failed.any()
        without = smp.loo()
        us = np.stack([smp.ctx.u_download(smp.ub_u[q]) for q in range(4)])
        theta = smp.theta.copy()
    finally:
        smp.ctx.close()
    assert sorted(set(rows[-1]) - set(without)) == ['khat', 'khat_w', 'loo_psis']
    for k in without:
        np.testing.assert_array_equal(rows[-1][k], without[k])
    assert rows[-1]['loo_psis'].shape == (4, 130) and rows[-1]['khat_w'].shape == (4,)
    p = ISLeaveOneOut(c['X'], c['y'], krn.make_kernel_func('ard', EPS), 64, max_batch=4)
    try:
        out = p(theta, us=us, psis=True)
        default = p(theta, us=us)
    finally:
        p.close()
    assert not out['status'].any()
    for k in ('loo', 'lpd', 'ess_loo', 'gauss', 'ess', 'loo_psis', 'khat', 'khat_w'):
        np.testing.assert_array_equal(rows[-1][k], out[k])
    assert sorted(set(out) - set(default)) == ['khat', 'khat_w', 'loo_psis']
    for k in default:
        np.testing.assert_array_equal(out[k], default[k])
    crit = combine_loo(np.stack([r['loo_psis'][0] for r in rows]),
                       np.stack([r['lpd'][0] for r in rows]), burn=1,
                       khat=np.stack([r['khat'][0] for r in rows]))
    assert np.isfinite(crit['elpd_loo']) and crit['khat'].shape == (130,)
    assert 0 <= crit['n_bad'] <= 130 and np.isfinite(crit['khat']).all()
