"""Gradient of the Laplace log marginal likelihood with respect to theta on the device
(apm_laplace_grad, gradient.hip) against the numpy/scipy restatement of
tests/grad_restatement.py and against central differences of the oracle's LML, plus the
properties that need no oracle: exact zeros, the epsilon rule, batch neutrality, the lml
identity, failure mapping, untouched cache slots, leading dimensions and `maximise`."""
import math

import numpy as np
import pytest

import apm_oracle as orc
import cov_restatement as cr
import grad_restatement as gr
from cov_restatement import Cov

pytestmark = pytest.mark.gpu

EPS = 1e-8
# device-to-restatement tolerance of lml and grad (x max(1, max|ref grad|)): fp64 against fp64
# through the same factorisation, the yardstick of DESIGN.md §5 that test_gpu_predict uses. The
# measured maximum over all cases below is 2.4e-13, more than 10x below it, so
# the yardstick stands.
TOL = 1e-9
NEWTON_TOL = 1e-14
# (n, d, kind, seed): one point; a full tile with d across two LDS chunks; tiles that are not
# full; d = 40 in two chunks; the isotropic kernel; nb = 10 > one outer panel (the bottom rows
# take the rank-256 update) with 15 super-tiles to sum. Three thetas each (theta_0 = 0.3, 3.0,
# -1.0). The seeds are chosen so that the restatement's last Newton `diff` is at least 100x below
# NEWTON_TOL and the one before at least 100x above it (test_newton_margins): device and
# restatement then cannot disagree on the iteration count.
SHAPES = [(1, 1, 'ard', 200), (64, 33, 'ard', 215), (130, 5, 'ard', 221), (129, 40, 'ard', 230),
          (200, 3, 'iso', 240), (600, 4, 'ard', 265)]
I_130, I_64, I_ISO = 2, 1, 4


@pytest.fixture(scope='module')
def cases():
    """Data and restatement results per shape, computed once and left unchanged."""
    out = []
    for n, d, kind, seed in SHAPES:
        c = gr.make_case(n, d, kind, seed)
        c['ref'] = [cr.laplace_grad(Cov('se', kind), c['X'], c['y'], th, EPS, tol=NEWTON_TOL)
                    for th in c['thetas']]
        out.append(c)
    return out


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _gradient(c, eps=EPS, **kw):
    import gpdemo.gradients as gd
    import gpdemo.kernels as krn
    return gd.LaplaceGradient(c['X'], c['y'], krn.make_kernel_func(c['kind'], eps), **kw)


@pytest.fixture(scope='module')
def device(nat, cases):
    """Device results per shape (one call each, three thetas)."""
    out = []
    for c in cases:
        p = _gradient(c)
        lml, grad = p(c['thetas'])
        out.append(dict(lml=lml, grad=grad, n_iter=p.n_iter.copy()))
        p.close()
    return out


def _kind(nat, kind):
    return nat.KERNEL_ISO if kind == 'iso' else nat.KERNEL_ARD


def _parity(dev_lml, dev_grad, ref):
    scale = max(1.0, np.abs(ref['grad']).max())
    return max(abs(dev_lml - ref['lml']), np.abs(dev_grad - ref['grad']).max()) / scale


def test_newton_margins(cases):
    """The condition on the inputs: last diff <= NEWTON_TOL / 100, the one before >= 100 x
    NEWTON_TOL. At n = 1 the data cannot change the Newton path (K is the scalar s + epsilon and
    y's sign is a symmetry), and theta_0 = -1 has diff = 1.97e-14 before its last step: no seed
    can give that shape the factor 100. What the equal iteration counts need is a margin above
    diff's own relative error, about 1e-9 (f's rounding over the step |f_new - f| ~ 1e-7), so
    n = 1 asks for the factor 1.5."""
    for c in cases:
        for ref in c['ref']:
            last, prev = ref['diffs'][-1], ref['diffs'][-2]
            assert last <= NEWTON_TOL / 100.0
            assert prev >= (1.5 if c['n'] == 1 else 100.0) * NEWTON_TOL


@pytest.mark.parametrize('ci', range(len(SHAPES)))
def test_grad_vs_restatement(cases, device, ci):
    c, dev = cases[ci], device[ci]
    worst = 0.0
    for t, ref in enumerate(c['ref']):
        assert int(dev['n_iter'][t]) == ref['n_iter']
        err = _parity(dev['lml'][t], dev['grad'][t], ref)
        worst = max(worst, err)
        print('grad parity shape {0} theta {1}: {2:.3e} (max|grad| {3:.3e})'
              .format(SHAPES[ci][:3], t, err, np.abs(ref['grad']).max()))
    print('grad parity shape {0}: worst {1:.3e} (tol {2:.0e})'.format(SHAPES[ci][:3], worst, TOL))
    assert worst <= TOL


@pytest.mark.parametrize('ci', [I_130, I_ISO])
def test_grad_vs_central_differences_of_the_oracle(cases, device, ci):
    """Independent of the restatement's algebra: central differences (h = 1e-5) of the oracle's
    own laplace_approximation LML, converged (diff_f_tol = 1e-24), to 1e-6 of max(1, max|fd|) -
    the restatement's own central-difference error is at most 3.5e-9 over these shapes
    (test_grad_host), and a wrong sign or a factor of 2 is off by order one."""
    c = cases[ci]

    def lml(th):
        K = Cov('se', c['kind']).gram(c['X'], th, EPS)
        return orc.laplace_approximation(K, c['y'], calc_cov=False, calc_lml=True,
                                         diff_f_tol=1e-24)[1]
    for t, th in enumerate(c['thetas']):
        fd = gr.central_differences(lml, th)
        err = np.abs(device[ci]['grad'][t] - fd).max() / max(1.0, np.abs(fd).max())
        print('grad vs fd shape {0} theta {1}: {2:.3e}'.format(SHAPES[ci][:3], t, err))
        assert err <= 1e-6


def test_exact_zeros(cases, device):
    # one point: every length-scale derivative has a zero diagonal
    assert np.all(device[0]['grad'][:, 1:] == 0.0) and np.all(device[0]['grad'][:, 0] != 0.0)
    # an ARD feature that is the same in every row (index 32: the first of the second LDS chunk)
    c = gr.make_case(129, 40, 'ard', 231)
    c['X'][:, 32] = 0.7
    p = _gradient(c)
    _, grad = p(c['thetas'])
    p.close()
    assert np.all(grad[:, 33] == 0.0)
    assert np.all(grad[:, 1:33] != 0.0) and np.all(grad[:, 34:] != 0.0)


def test_iso_equals_ard_with_equal_length_scales(cases, device):
    """grad_iso[0] == grad_ard[0] and grad_iso[1] == sum grad_ard[1:], to 1e-12 of the summands'
    size max(1, sum |grad_ard[1:]|): both contexts build the same K (the same 1/tau on every
    feature) and the same w per pair; they differ in the order in which the features' sums are
    added (per super-tile first, or per feature first), i.e. by a few ulp of the summands."""
    c = cases[I_ISO]
    ard = dict(c, kind='ard')
    th_ard = np.array([np.r_[th[0], np.full(c['d'], th[1])] for th in c['thetas']])
    p = _gradient(ard)
    lml, grad = p(th_ard)
    p.close()
    iso = device[I_ISO]
    for t in range(3):
        scale = max(1.0, np.abs(grad[t, 1:]).sum())
        assert lml[t] == iso['lml'][t]
        assert abs(iso['grad'][t, 0] - grad[t, 0]) <= 1e-12 * max(1.0, abs(grad[t, 0]))
        assert abs(iso['grad'][t, 1] - grad[t, 1:].sum()) <= 1e-12 * scale


@pytest.mark.parametrize('ci', [I_130, I_64])
def test_epsilon_rule(cases, ci):
    """Contexts with epsilon = 1e-2: dK/dtheta_0's diagonal is s, not s + epsilon. The wrong
    reading moves the restatement's grad[0] by epsilon * trace(M), which must be visible."""
    c = cases[ci]
    p = _gradient(c, eps=1e-2)
    lml, grad = p(c['thetas'])
    nit = p.n_iter.copy()
    p.close()
    for t, th in enumerate(c['thetas']):
        ref = cr.laplace_grad(Cov('se', c['kind']), c['X'], c['y'], th, 1e-2, tol=NEWTON_TOL)
        wrong = cr.laplace_grad(Cov('se', c['kind']), c['X'], c['y'], th, 1e-2, tol=NEWTON_TOL,
                                wrong='eps_in_dk0')
        assert int(nit[t]) == ref['n_iter']
        err = _parity(lml[t], grad[t], ref)
        off = np.abs(grad[t] - wrong['grad']).max() / max(1.0, np.abs(ref['grad']).max())
        print('epsilon rule shape {0} theta {1}: parity {2:.3e}, wrong reading off by {3:.3e}'
              .format(SHAPES[ci][:3], t, err, off))
        assert err <= TOL
        assert off > 1e-6


def test_batches_are_bitwise_neutral(nat, cases):
    """theta alone, first of 3, last of 8 (max_batch = 8), and inside 5 thetas through
    LaplaceGradient with max_batch = 2: the same bits."""
    c = cases[I_130]
    rng = np.random.RandomState(5)
    other = c['thetas'][rng.randint(0, 3, size=7)] + rng.uniform(-0.2, 0.2, size=(7, 6))
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 1, max_batch=8, n_slots=1, n_ubufs=1)
    ctx.set_newton(NEWTON_TOL, 1000)
    p2 = _gradient(c, max_batch=2)
    for th in c['thetas']:
        alone = ctx.laplace_grad(th)
        first = ctx.laplace_grad(np.vstack([th[None], other[:2]]))
        last = ctx.laplace_grad(np.vstack([other, th[None]]))
        for pos in (0, 1, 3, 4):  # both places of a pair, and the odd one out
            five = np.insert(other[:4], pos, th, axis=0)
            l5, g5 = p2(five)
            assert l5[pos] == alone[0][0] and np.array_equal(g5[pos], alone[1][0])
        assert alone[2][0] == 0 and np.all(np.isfinite(alone[1]))
        assert first[0][0] == alone[0][0] and np.array_equal(first[1][0], alone[1][0])
        assert last[0][7] == alone[0][0] and np.array_equal(last[1][7], alone[1][0])
        assert first[3][0] == alone[3][0] == last[3][7]
    p2.close()
    ctx.close()


def test_lml_is_the_laplace_theta_calls(nat, cases, device):
    """apm_theta_eval(APM_EST_LAPLACE) always takes the fp64 Newton path (include/apm.h): the
    same bits at the same Newton settings, with no setting to pin."""
    for ci in (I_64, I_130, I_ISO):
        c = cases[ci]
        ctx = nat.Context(c['X'], c['y'], _kind(nat, c['kind']), EPS, 1, max_batch=4, n_slots=1,
                          n_ubufs=1)
        ctx.set_newton(NEWTON_TOL, 1000)
        val, st, nops = ctx.theta_eval(nat.EST_LAPLACE, c['thetas'])
        ctx.close()
        assert list(st) == [0, 0, 0]
        assert np.array_equal(val, device[ci]['lml'])
        assert np.array_equal(nops, device[ci]['n_iter'])


def test_failure_mapping(nat, cases):
    from gpdemo.latent_posterior_approximations import MaximumIterationsExceededError
    c = cases[I_130]
    easy = c['thetas'][0].copy()
    easy[0] = -12.0  # |f| ~ n sigma: the first Newton step already moves f by less than the tol
    thetas = np.array([easy, c['thetas'][0], easy + 0.01])
    p = _gradient(c, diff_f_tol=1e-4)
    good = p(thetas)
    assert list(p.n_iter[[0, 2]]) == [1, 1] and p.n_iter[1] > 1
    p.close()
    p1 = _gradient(c, diff_f_tol=1e-4, max_iters=1)
    with pytest.raises(MaximumIterationsExceededError):
        p1(thetas)
    got = p1(thetas, on_error='nan')
    assert list(p1.status) == [nat.STATUS_OK, nat.STATUS_MAXITER, nat.STATUS_OK]
    for g, r in zip(got, good):
        assert np.all(np.isnan(g[1])) and np.all(np.isfinite(r))
        assert np.array_equal(g[[0, 2]], r[[0, 2]])
    p1.close()


def test_invalid_arguments_and_leading_dimensions(nat, cases, device):
    c = cases[I_64]
    P = c['thetas'].shape[1]
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 1, max_batch=2, n_slots=1, n_ubufs=1)
    ctx.set_newton(NEWTON_TOL, 1000)
    ldt, ldg = P + 3, P + 2
    th = np.full((3, ldt), 1e300)  # (the padding must not be read as theta either)
    th[:, :P] = c['thetas']
    grad = np.full((3, ldg), 7.25)
    lml = np.full(3, 7.25)
    st = np.full(3, -1, dtype=np.int32)
    nit = np.full(3, -1, dtype=np.int64)

    def call(count, ldt_, ldg_, h=ctx._h, g=grad):
        return ctx.lib.apm_laplace_grad(h, count, th.ctypes.data, ldt_, lml.ctypes.data,
                                        None if g is None else g.ctypes.data, ldg_,
                                        st.ctypes.data, nit.ctypes.data)

    def err(h=ctx._h):
        return ctx.lib.apm_last_error(h)
    assert call(3, ldt, ldg) == nat.APM_E_INVALID and b'max_batch' in err()
    assert call(0, ldt, ldg) == nat.APM_E_INVALID and b'max_batch' in err()
    assert call(2, P - 1, ldg) == nat.APM_E_INVALID and b'ldt' in err()
    assert call(2, ldt, P - 1) == nat.APM_E_INVALID and b'ldg' in err()
    assert call(2, ldt, ldg, g=None) == nat.APM_E_INVALID and b'bad arguments' in err()
    assert np.all(grad == 7.25) and np.all(lml == 7.25) and np.all(st == -1)
    assert call(2, ldt, ldg) == 0
    assert list(st) == [0, 0, -1] and nit[2] == -1 and lml[2] == 7.25
    assert np.all(grad[:, P:] == 7.25) and np.all(grad[2] == 7.25)
    assert np.array_equal(grad[:2, :P], device[I_64]['grad'][:2])
    assert np.array_equal(lml[:2], device[I_64]['lml'][:2])
    assert np.array_equal(nit[:2], device[I_64]['n_iter'][:2])
    # lml and n_iter may be NULL
    g2 = np.full((2, P), np.nan)
    assert ctx.lib.apm_laplace_grad(ctx._h, 2, th.ctypes.data, ldt, None, g2.ctypes.data, P,
                                    st.ctypes.data, None) == 0
    assert np.array_equal(g2, grad[:2, :P])
    ctx.close()
    pre = nat.Context(None, c['y'], nat.KERNEL_PRECOMPUTED, EPS, 1)
    assert call(1, ldt, ldg, pre._h) == nat.APM_E_INVALID
    assert b'ISO or ARD' in err(pre._h)
    pre.close()


def test_grad_leaves_cache_slots_alone(nat, cases):
    """An IS theta-call into a slot, a gradient call on the same context (it shares the work
    matrix), then the slot read back and its u-call: the same bits as before the gradient call."""
    c = cases[I_130]
    ctx = nat.Context(c['X'], c['y'], nat.KERNEL_ARD, EPS, 8, max_batch=2, n_slots=2, n_ubufs=2)
    ctx.u_normal([0, 1], [5, 5], [0, 1])
    slot = ctx.slots.acquire()
    _, st, _ = ctx.theta_eval(nat.EST_IS, c['thetas'][:1], [0], [slot])
    assert st[0] == 0
    before, st = ctx.u_eval([slot], [1])
    state = ctx.slot_read(slot)
    assert st[0] == 0
    lml, grad, gst, _ = ctx.laplace_grad(c['thetas'])
    assert list(gst) == [0, 0, 0] and np.all(np.isfinite(grad)) and np.all(np.isfinite(lml))
    again = ctx.slot_read(slot)
    for a, b in zip(state, again):
        assert np.array_equal(a, b)
    after, st = ctx.u_eval([slot], [1])
    assert st[0] == 0 and np.array_equal(before, after)
    ctx.close()


def test_maximise(cases):
    """MAP fit on (130, 5, ard) from theta_0 = 0, length scales 1/2 log d, under a N(0, 3^2)
    prior: L-BFGS-B reports success, does not end below its start, and the device gradient of the
    log posterior at x is within gtol in the max-norm (unbounded: scipy's projected gradient)."""
    c = cases[I_130]
    p = _gradient(c)
    theta0 = np.r_[0.0, np.full(c['d'], 0.5 * math.log(c['d']))]
    start, _ = p.log_posterior(theta0, 0.0, 3.0)
    res = p.maximise(theta0, prior_mean=0.0, prior_std=3.0, gtol=1e-5)
    val, grad = p.log_posterior(res.x, 0.0, 3.0)
    lml, _ = p(res.x)
    p.close()
    print('maximise: {0} evaluations, {1} iterations, log posterior {2:.6f} -> {3:.6f}, '
          'max|grad| {4:.2e}'.format(res.nfev, res.nit, start[0], val[0], np.abs(grad).max()))
    assert res.success
    assert val[0] >= start[0]
    assert np.abs(grad[0]).max() <= 1e-5
    assert res.value == val[0] and np.array_equal(res.grad, grad[0]) and res.lml == lml[0]
    assert res.fun == -val[0]
