"""The refusals of the batched theta-calls of the C-ABI (apm_predict, apm_laplace_grad, apm_ep_eval,
apm_ep_predict, apm_ep_grad, apm_is_predict) and of apm_u_eval_diag / apm_is_spread: for every
branch of their argument checks the return code and the exact bytes of apm_last_error /
apm_global_error, with pairs of bad arguments that pin the order of the checks; that a refused
call leaves the context usable; and the edges of row finishing and batching (a ragged last batch,
two blocks of test inputs, no surviving chain, null optional outputs). The strings are written out
here, not taken from the library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, S, B = 8, 2, 4, 2
P = D + 1
M = 3  # test inputs of the refused and the good calls
EPS = 1e-8
THETAS = np.array([[0.1, 0.0, -0.1], [-0.2, 0.1, 0.05], [0.05, -0.1, 0.2]])
SEEDS = np.array([0x5eed0001, 0x5eed0002], dtype=np.uint64)
CTRS = np.array([7, 9], dtype=np.uint64)

PROBIT_ONLY = b" probit only (the logit's tilted moments need quadrature)"
ON_DEVICE_XCOV = b' needs an ISO or ARD context (the cross-covariance is built on the device)'
ON_DEVICE_DK = b' needs an ISO or ARD context (dK/dtheta is built on the device)'
COUNT = b' count outside [1, max_batch]'
BAD = b' bad arguments'


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _data():
    rng = np.random.RandomState(808)
    X = rng.normal(size=(N, D))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=N) > 0, 1.0, -1.0)
    return X, y, rng.normal(size=(M, D))


def _context(nat, which):
    X, y, _ = _data()
    if which == 'pre':
        return nat.Context(None, y, nat.KERNEL_PRECOMPUTED, EPS, S, max_batch=B, n_slots=2,
                           n_ubufs=2)
    return nat.Context(X, y, nat.KERNEL_ARD, EPS, S, max_batch=B, n_slots=2, n_ubufs=2,
                       likelihood=which)


class _Args(object):
    """The good arguments of every entry point (count = 2, m = 3), each replaceable by keyword;
    `call(name, h, **bad)` passes them in the entry point's order."""

    ORDER = {
        'apm_predict': 'count thetas ldt Xs m ldxs mean var prob ldo status n_iter',
        'apm_ep_predict': 'count thetas ldt Xs m ldxs mean var prob ldo status n_iter',
        'apm_laplace_grad': 'count thetas ldt val grad ldg status n_iter',
        'apm_ep_grad': 'count thetas ldt val grad ldg status n_iter',
        'apm_ep_eval': 'count thetas ldt val mu svar tau nu ldn status n_iter',
        'apm_is_predict': 'est count thetas ldt ubufs slots Xs m ldxs val prob mean var ldo ess '
                          'status nops',
        'apm_u_eval_diag': 'count slots ubufs block dlogf dess dwmax ldb status',
        'apm_is_spread': 'count slots ubufs seeds counters n_rep block dlogf dess dwmax ldb status',
    }

    def __init__(self, nat):
        self.lib = nat.load_library()
        f = lambda *shape: np.full(shape, -7.0)  # noqa: E731
        self.good = dict(
            est=nat.EST_IS, count=B, thetas=THETAS[:B].copy(), ldt=P, Xs=_data()[2], m=M, ldxs=D,
            mean=f(B, M), var=f(B, M), prob=f(B, M), ldo=M, status=np.zeros(B, dtype=np.int32),
            n_iter=np.zeros(B, dtype=np.int64), nops=np.zeros(B, dtype=np.int64), val=f(B),
            grad=f(B, P), ldg=P, mu=f(B, N), svar=f(B, N), tau=f(B, N), nu=f(B, N), ldn=N,
            ess=f(B), ubufs=np.arange(B, dtype=np.int64), slots=np.arange(B, dtype=np.int64),
            seeds=SEEDS, counters=CTRS, n_rep=2, block=2, dlogf=f(B, 4), dess=f(B, 4),
            dwmax=f(B, 4), ldb=4)

    def call(self, name, h, **bad):
        a = dict(self.good, **bad)
        vals = [a[k] for k in self.ORDER[name].split()]
        return getattr(self.lib, name)(
            h, *[v.ctypes.data if isinstance(v, np.ndarray) else v for v in vals])


def _i64(*v):
    return np.array(v, dtype=np.int64)


def _ladder(name, probit, why_device, shape):
    """The cases of one of the five calls that check their own theta arguments: (context, bad
    arguments, message after the entry point's name and the colon)."""
    cases = [('null', {}, b' null context'), ('pre', {}, why_device)]
    if probit:
        cases += [('logit', {}, PROBIT_ONLY), ('logit', dict(count=0, thetas=None), PROBIT_ONLY)]
    cases += [('probit', dict(count=0), COUNT), ('probit', dict(count=B + 1), COUNT)]
    if shape == 'predict':
        cases += [
            ('pre', dict(m=0, count=0), why_device),
            ('probit', dict(m=0), b' m <= 0'), ('probit', dict(m=-1, count=B + 1), b' m <= 0'),
            ('probit', dict(count=B + 1, ldo=M - 1), COUNT),
            ('probit', dict(ldo=M - 1), b' ldo < m'),
            ('probit', dict(ldo=M - 1, thetas=None), b' ldo < m'),
            ('probit', dict(Xs=None), BAD), ('probit', dict(ldxs=D - 1), BAD),
            ('probit', dict(ldt=P - 1), BAD)]
    elif shape == 'grad':
        cases += [
            ('pre', dict(count=0, ldt=0), why_device),
            ('probit', dict(count=B + 1, ldt=P - 1), COUNT),
            ('probit', dict(ldt=P - 1), b' ldt < theta length'),
            ('probit', dict(ldt=P - 1, ldg=P - 1), b' ldt < theta length'),
            ('probit', dict(ldg=P - 1), b' ldg < theta length'),
            ('probit', dict(ldg=P - 1, grad=None), b' ldg < theta length'),
            ('probit', dict(grad=None), BAD)]
    else:  # apm_ep_eval
        cases += [
            ('pre', dict(count=0, thetas=None), why_device),
            ('probit', dict(count=B + 1, ldt=P - 1), COUNT),
            ('probit', dict(ldt=P - 1), BAD), ('probit', dict(ldn=N - 1), BAD),
            ('probit', dict(ldn=N - 1, mu=None, svar=None, tau=None), BAD)]
    cases += [('probit', dict(thetas=None), BAD), ('probit', dict(status=None), BAD)]
    return [(name, ctx, bad, name.encode() + b':' + msg) for ctx, bad, msg in cases]


def _diag_ladder(name):
    spread = name == 'apm_is_spread'
    cases = [
        ('null', {}, b' null context'),
        ('probit', dict(count=0), COUNT), ('probit', dict(count=B + 1), COUNT),
        ('probit', dict(count=B + 1, slots=None), COUNT),
        ('probit', dict(slots=None), BAD), ('probit', dict(ubufs=None), BAD),
        ('probit', dict(status=None), BAD), ('probit', dict(status=None, block=0), BAD),
        ('probit', dict(block=0), b' block outside [1, n_imp]'),
        ('probit', dict(block=S + 1), b' block outside [1, n_imp]'),
        ('probit', dict(ldb=1), b' ldo < n_rep * nblk'),
        ('probit', dict(ldb=1, slots=_i64(0, 2)), b' ldo < n_rep * nblk'),
        ('pre', dict(slots=_i64(0, 2)), None), ('probit', dict(slots=_i64(-1, 0)), None),
        ('probit', dict(slots=_i64(2, 0), ubufs=_i64(2, 0)), None),
        ('logit', dict(ubufs=_i64(0, 2)), None)]
    if spread:
        cases += [
            ('probit', dict(seeds=None), BAD), ('probit', dict(counters=None), BAD),
            ('probit', dict(block=0, n_rep=0), b' block outside [1, n_imp]'),
            ('probit', dict(n_rep=0), b' n_rep < 1'),
            ('probit', dict(n_rep=0, ldb=0), b' n_rep < 1'),
            ('probit', dict(n_rep=4097, block=S), b' n_rep * nblk above APM_SPREAD_MAX_BLOCKS'),
            ('probit', dict(n_rep=2049), b' n_rep * nblk above APM_SPREAD_MAX_BLOCKS'),
            ('probit', dict(n_rep=2049, ldb=1), b' n_rep * nblk above APM_SPREAD_MAX_BLOCKS')]
    out = []
    for ctx, bad, msg in cases:
        if msg is None:  # (the index checks name no entry point; slots are checked first)
            msg = b'slot index out of range' if 'slots' in bad else b'ubuf index out of range'
        else:
            msg = name.encode() + b':' + msg
        out.append((name, ctx, bad, msg))
    return out


def _is_predict_ladder(nat):
    name = 'apm_is_predict'
    own = [
        ('null', {}, b' null context'),
        ('probit', dict(est=nat.EST_LAPLACE), b' APM_EST_IS or APM_EST_IS_EP only'),
        ('probit', dict(est=nat.EST_PRIORMC), b' APM_EST_IS or APM_EST_IS_EP only'),
        ('pre', dict(est=nat.EST_LAPLACE), b' APM_EST_IS or APM_EST_IS_EP only'),
        ('pre', {}, b' needs a context whose covariance is built on the device (the cross-'
                    b'covariance is)'),
        ('pre', dict(m=0), b' needs a context whose covariance is built on the device (the cross-'
                           b'covariance is)'),
        ('probit', dict(m=0), b' bad test inputs or ldo < m'),
        ('probit', dict(ldo=M - 1), b' bad test inputs or ldo < m'),
        ('probit', dict(Xs=None), b' bad test inputs or ldo < m'),
        ('probit', dict(ldxs=D - 1), b' bad test inputs or ldo < m'),
        ('probit', dict(m=0, count=0), b' bad test inputs or ldo < m')]
    # what it leaves to apm_theta_eval, under that call's name
    th = b'apm_theta_eval:'
    theirs = [
        ('probit', dict(count=0), th + BAD), ('probit', dict(count=B + 1), th + BAD),
        ('probit', dict(thetas=None), th + BAD), ('probit', dict(val=None), th + BAD),
        ('probit', dict(status=None), th + BAD), ('probit', dict(ldt=P - 1), th + BAD),
        ('logit', dict(est=nat.EST_IS_EP, count=0), th + BAD),
        ('logit', dict(est=nat.EST_IS_EP), th + b" APM_EST_IS_EP is probit only (the logit's "
                                                b'tilted moments need quadrature)'),
        ('logit', dict(est=nat.EST_IS_EP, slots=None), th + b" APM_EST_IS_EP is probit only (the "
                                                            b"logit's tilted moments need "
                                                            b'quadrature)'),
        ('probit', dict(ubufs=None), th + b' ubufs/slots required'),
        ('probit', dict(slots=None), th + b' ubufs/slots required'),
        ('probit', dict(slots=_i64(0, 2)), b'slot index out of range'),
        ('probit', dict(slots=_i64(0, 2), ubufs=_i64(0, 2)), b'slot index out of range'),
        ('probit', dict(ubufs=_i64(0, -1)), b'ubuf index out of range')]
    return ([(name, ctx, bad, name.encode() + b':' + msg) for ctx, bad, msg in own] +
            [(name, ctx, bad, msg) for ctx, bad, msg in theirs])


def _table(nat):
    return (_ladder('apm_predict', False, ON_DEVICE_XCOV, 'predict') +
            _ladder('apm_ep_predict', True, ON_DEVICE_XCOV, 'predict') +
            _ladder('apm_laplace_grad', False, ON_DEVICE_DK, 'grad') +
            _ladder('apm_ep_grad', True, ON_DEVICE_DK, 'grad') +
            _ladder('apm_ep_eval', True,
                    b" needs an ISO or ARD context (apm_ep takes a K of the caller's)", 'eval') +
            _is_predict_ladder(nat) + _diag_ladder('apm_u_eval_diag') +
            _diag_ladder('apm_is_spread'))


def _good_calls(nat, ctx, which):
    """One good call of every entry point the context supports; all outputs, in order."""
    out = []
    idx = [0, 1]
    ctx.u_normal(idx, [11, 11], [0, 1])  # (apm_is_spread leaves its own draws in the buffers)
    if which == 'pre':
        K = np.empty((N, N))
        nat.gram(nat.KERNEL_ARD, K, _data()[0], THETAS[0], EPS)
        out += list(ctx.theta_eval_K(nat.EST_IS, K, 0, 0))
        out += list(ctx.theta_eval_K(nat.EST_IS, K, 1, 1))
    else:
        th, Xs = THETAS[:B], _data()[2]
        out += list(ctx.predict(th, Xs)) + list(ctx.laplace_grad(th))
        ests = [nat.EST_IS]
        if which == 'probit':
            out += list(ctx.ep(th)) + list(ctx.ep_predict(th, Xs)) + list(ctx.ep_grad(th))
            ests.append(nat.EST_IS_EP)
        for est in ests:
            out += list(ctx.is_predict(est, th, idx, idx, Xs))
    out += list(ctx.u_eval_diag(idx, idx, 2))
    out += list(ctx.is_spread(idx, idx, SEEDS, CTRS, 2, 2))
    return out


def _same(a, b):
    return len(a) == len(b) and all(
        x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        for x, y in zip(a, b))


@pytest.mark.parametrize('which', ['null', 'probit', 'logit', 'pre'])
def test_refusals_and_context_stays_usable(nat, which):
    a = _Args(nat)
    cases = [t for t in _table(nat) if t[1] == which]
    assert len(cases) >= (8 if which == 'null' else 10)
    ctx = None if which == 'null' else _context(nat, which)
    h = ctx._h if ctx else None
    try:
        before = _good_calls(nat, ctx, which) if ctx else None
        wrong = []
        for name, _, bad, msg in cases:
            rc = a.call(name, h, **bad)
            got = a.lib.apm_last_error(h) if ctx else a.lib.apm_global_error()
            if rc != nat.APM_E_INVALID or got != msg:
                wrong.append((name, sorted(bad), rc, got, msg))
        assert not wrong, wrong
        if ctx:
            after = _good_calls(nat, ctx, which)
            assert all(np.isfinite(x).all() for x in before if x.dtype == np.float64)
            assert all(not x.any() for x in before if x.dtype == np.int32)
            assert _same(before, after)
    finally:
        if ctx:
            ctx.close()


def test_every_entry_point_has_two_double_faults(nat):
    """The table itself: at least two cases with two bad arguments at once per entry point."""
    for name in _Args.ORDER:
        assert sum(1 for t in _table(nat) if t[0] == name and len(t[2]) >= 2) >= 2, name


# ---- row finishing and batching at the edges ---------------------------------------------------

def _batched(ctx, Xs):
    return {'predict': lambda th: ctx.predict(th, Xs), 'laplace_grad': ctx.laplace_grad,
            'ep': ctx.ep, 'ep_predict': lambda th: ctx.ep_predict(th, Xs), 'ep_grad': ctx.ep_grad}


def test_ragged_last_batch(nat):
    """T = 3 rows with max_batch = 2: bitwise the calls on rows [0:2] and [2:3]."""
    ctx = _context(nat, 'probit')
    try:
        for name, fn in _batched(ctx, _data()[2]).items():
            whole, head, tail = fn(THETAS), fn(THETAS[:2]), fn(THETAS[2:])
            assert not whole[-2].any(), (name, whole[-2])
            assert _same(list(whole), [np.concatenate([h, t]) for h, t in zip(head, tail)]), name
    finally:
        ctx.close()


def test_two_test_blocks(nat):
    """m = padded_n + 1 test inputs are two blocks: the first padded_n rows are bitwise a call with
    those rows, the last row bitwise a call with it alone (m = 1)."""
    ctx = _context(nat, 'probit')
    np_ = ctx.padded_n
    Xs = np.random.RandomState(809).normal(size=(np_ + 1, D))
    th, idx = THETAS[:B], [0, 1]
    ctx.u_normal(idx, [11, 11], [0, 1])
    calls = {'predict': (lambda x: ctx.predict(th, x), (0, 1, 2)),
             'ep_predict': (lambda x: ctx.ep_predict(th, x), (0, 1, 2)),
             'is': (lambda x: ctx.is_predict(nat.EST_IS, th, idx, idx, x), (1, 2, 3)),
             'is_ep': (lambda x: ctx.is_predict(nat.EST_IS_EP, th, idx, idx, x), (1, 2, 3))}
    try:
        for name, (fn, per_row) in calls.items():
            both, first, last = fn(Xs), fn(Xs[:np_]), fn(Xs[np_:])
            assert last[per_row[0]].shape == (B, 1)
            for k in range(len(both)):
                if k in per_row:
                    assert np.isfinite(both[k]).all(), (name, k)
                    assert _same([both[k][:, :np_], both[k][:, np_:]], [first[k], last[k]]), \
                        (name, k)
                else:
                    assert _same([both[k], both[k]], [first[k], last[k]]), (name, k)
    finally:
        ctx.close()


def test_no_chain_survives(nat):
    """One Newton iteration and one EP sweep allowed: every chain ends STATUS_MAXITER, every float
    output the call finishes is NaN, statuses and counts are reported and the calls succeed."""
    ctx = _context(nat, 'probit')
    ctx.set_newton(1e-10, 1)
    ctx.set_ep(0.8, 1e-8, 1)
    Xs, th, idx = _data()[2], THETAS[:B], [0, 1]
    ctx.u_normal(idx, [11, 11], [0, 1])
    try:
        for name, fn in _batched(ctx, Xs).items():
            res = fn(THETAS)
            assert list(res[-2]) == [nat.STATUS_MAXITER] * 3, (name, res[-2])
            assert list(res[-1]) == [1] * 3, (name, res[-1])
            assert all(np.isnan(r).all() for r in res[:-2]), name
        for est in (nat.EST_IS, nat.EST_IS_EP):
            ref = ctx.theta_eval(est, th, idx, idx)
            res = ctx.is_predict(est, th, idx, idx, Xs)
            assert list(res[5]) == [nat.STATUS_MAXITER] * B, (est, res[5])
            assert all(np.isnan(r).all() for r in res[1:5]), est
            # (log f, status and the operation count are the theta-call's own, bitwise: that call
            # reports a failed chain in its status, not as a NaN)
            assert _same([res[0], res[5], res[6]], list(ref)), est
    finally:
        ctx.close()


def test_null_optional_outputs(nat):
    """apm_predict without mean / var, apm_ep_eval without mu / var / tau / nu, apm_is_predict
    without ess / nops: the remaining outputs are bitwise the full call's."""
    ctx = _context(nat, 'probit')
    ctx.u_normal([0, 1], [11, 11], [0, 1])
    full, part = _Args(nat), _Args(nat)
    cases = {'apm_predict': (dict(mean=None, var=None), ('prob', 'status', 'n_iter')),
             'apm_ep_eval': (dict(mu=None, svar=None, tau=None, nu=None),
                             ('val', 'status', 'n_iter')),
             'apm_is_predict': (dict(ess=None, nops=None),
                                ('val', 'prob', 'mean', 'var', 'status'))}
    try:
        for name, (nulls, kept) in cases.items():
            assert full.call(name, ctx._h) == nat.APM_SUCCESS
            assert part.call(name, ctx._h, **nulls) == nat.APM_SUCCESS
            assert not full.good['status'].any()
            for k in kept:  # (written: -7 is what the buffers held before)
                if full.good[k].dtype == np.float64:
                    assert np.isfinite(full.good[k]).all() and (full.good[k] != -7.0).all(), k
            assert _same([full.good[k] for k in kept], [part.good[k] for k in kept]), name
    finally:
        ctx.close()
