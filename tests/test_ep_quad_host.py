"""Host side of EP with the tilted moments by quadrature: the C-ABI / Python
surface without a device, the rule itself (tests/ep_quad_restatement.py, from the tables the
kernel includes) against mpmath.quad at 30 digits, and the restatement's logit fit against
independent routes - the exact n = 1 value, grid quadrature of a 2 x 2 problem and sequential EP."""
import math

import numpy as np
import pytest
from scipy.special import expit
from scipy.stats import multivariate_normal

import ep_quad_restatement as eq
from test_ep_host import _se_case

NEW_SYMBOLS = ('apm_set_ep_quadrature', 'apm_ep_quadrature', 'apm_ep_lik')

# The rule's acceptance grid and bound. The bound follows from the estimator tolerance of DESIGN.md
# §3.3, 5e-4 nats, for a log Z_EP that sums n = 16384 site terms: 5e-4 / 16384 = 3e-8 per site in
# log Z^, and the same figure for the mean (in tilted deviations) and the variance (relative).
S2 = (1e-2, 0.1, 0.5, 1.0, 2.0, 5.0, 8.0, 12.0, 20.0, 40.0, 100.0, math.exp(6), math.exp(8),
      math.exp(10))
A = (0, 1, -1, 2, -2, 3, -3, -4, 6, 8, -8)
SITE_TOL = 3e-8


def documented_uncovered(lik, s2, a):
    """The covered region as include/apm.h states it, written out again here: of the grid only
    the probit's wide branch leaves it, where -m = -a sd exceeds min(5 (1 + s_-), 300)."""
    sd = math.sqrt(s2)
    if lik == eq.LOGIT:
        return s2 > 5.0 and (-a * sd > s2 + 7.5 * sd + 20.0 or (-a * sd < s2 and a < -30.0))
    if s2 <= 5.0:
        return -a * sd * sd > 8.0 * math.sqrt(2.0) * (1.0 + s2)
    return -a * sd > min(5.0 * (1.0 + s2), 300.0)


def test_library_exports_and_binds_the_switch():
    """Fails without the feature: the three symbols and their bindings are new. Null contexts
    and a switch value other than 0 / 1 are refused before any device call; apm_version() stays
    3."""
    from gpdemo import _native
    syms = _native.exported_symbols()
    lib = _native.load_library(check_device=False)
    for name in NEW_SYMBOLS:
        assert name in syms and hasattr(lib, name)
    assert lib.apm_version() == 3
    bad = _native.APM_E_INVALID
    for on in (0, 1, 2):
        assert lib.apm_set_ep_quadrature(None, on) == bad
    assert lib.apm_ep_quadrature(None) < 0
    for name in ('set_ep_quadrature', 'set_ep'):
        assert callable(getattr(_native.Context, name))
    # apm_ep_lik: apm_ep's argument checks, and a likelihood code that does not exist
    one = np.ones(4)
    st = np.zeros(1, dtype=np.int32)

    def ep_lik(lik, n, ldk, damping):
        return lib.apm_ep_lik(0, lik, one.ctypes.data, n, ldk, one.ctypes.data, 0, damping, 1e-8,
                              100, None, None, None, None, None, n, None, None, st.ctypes.data)
    assert ep_lik(2, 2, 2, 0.8) == bad
    assert ep_lik(-1, 2, 2, 0.8) == bad
    assert ep_lik(_native.LIK_LOGIT, 2, 1, 0.8) == bad
    assert ep_lik(_native.LIK_LOGIT, 2, 2, 0.0) == bad


def test_header_declares_the_switch_and_the_covered_region():
    import os
    import re
    from conftest import REPO
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    for name, k in (('apm_set_ep_quadrature', 2), ('apm_ep_quadrature', 1), ('apm_ep_lik', 19)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)', txt)
        assert m and len(m.group(1).split(',')) == k, name
    assert 'covered region' in txt and 'APM_STATUS_EP_CAVITY' in txt


_exact_cache = {}


def _exact(lik, m, s2):
    """The tilted moments of p(t) N(t | m, s2) by mpmath.quad; y = -1 at mu_- = -m is the same
    integral, so the two labels share one evaluation."""
    key = (lik, m, s2)
    if key not in _exact_cache:
        _exact_cache[key] = eq.exact_moments(lik, 1.0, m, s2, dps=30)
    return _exact_cache[key]


@pytest.mark.parametrize('s2', S2)
@pytest.mark.parametrize('lik', (eq.LOGIT, eq.PROBIT))
def test_rule_against_mpmath(lik, s2):
    """Every (a, y) of the grid at one cavity variance: log Z^, the tilted mean in tilted
    deviations and the tilted variance relatively, each within 3e-8 of 30-digit quadrature - or
    the point is outside the covered region, and then it is one of the documented corners. The
    CPU study measured 9.6e-13 as the narrow branch's worst case and 3.9e-11 as the wide one's
    (DESIGN.md §27)."""
    sd = math.sqrt(s2)
    worst, uncovered = 0.0, set()
    for a in A:
        for y in (1.0, -1.0):
            mu_c = y * a * sd
            lz, mu_h, var_h, cov = (v[0] for v in eq.tilted_quad(lik, y, mu_c, s2))
            if not cov:
                uncovered.add((lik, s2, a))
                continue
            ex_lz, ex_m, ex_v = _exact(lik, a * sd, s2)
            ex_mu = y * ex_m  # (exact_moments ran with y = +1 at mu_- = m)
            errs = (abs(lz - ex_lz), abs(mu_h - ex_mu) / math.sqrt(ex_v), abs(var_h - ex_v) / ex_v)
            worst = max(worst, max(errs))
            assert max(errs) <= SITE_TOL, (lik, s2, a, y, errs)
    print('lik {0} s2 {1:.4g}: worst {2:.2e}, uncovered {3}'.format(lik, s2, worst,
                                                                    sorted(uncovered)))
    assert uncovered == {(lik, s2, a) for a in A if documented_uncovered(lik, s2, a)}
    # the logit, which the feature exists for, is covered on the whole grid; the probit leaves it
    # only at sd >= e^4 (-m = 8 sd, and at e^10 also 3 sd and 4 sd, above 300)
    assert not uncovered or (lik == eq.PROBIT and s2 >= math.exp(8))


def test_covered_region_is_what_the_header_states():
    """The masks of the restatement at points either side of each documented limit."""
    def cov(lik, m, s2):
        return bool(eq.tilted_quad(lik, 1.0, m, s2)[3][0])
    for s2 in (6.0, 100.0, math.exp(10)):
        sd = math.sqrt(s2)
        lim = s2 + 7.5 * sd + 20.0
        assert cov(eq.LOGIT, -0.999 * lim, s2) and not cov(eq.LOGIT, -1.001 * lim, s2)
        assert cov(eq.LOGIT, 1e3 * sd, s2)
    # where -m < s_-: alpha >= -30
    s2 = math.exp(10)
    assert cov(eq.LOGIT, -29.9 * math.sqrt(s2), s2) and not cov(eq.LOGIT, -30.1 * math.sqrt(s2), s2)
    assert cov(eq.LOGIT, -1e4, 5.0)  # the narrow branch covers the logit everywhere
    for s2 in (6.0, 100.0):
        lim = min(5.0 * (1.0 + s2), 300.0)
        assert cov(eq.PROBIT, -0.999 * lim, s2) and not cov(eq.PROBIT, -1.001 * lim, s2)
    for s2 in (0.01, 5.0):
        lim = 8.0 * math.sqrt(2.0) * (1.0 + s2) / math.sqrt(s2)
        assert cov(eq.PROBIT, -0.999 * lim, s2) and not cov(eq.PROBIT, -1.001 * lim, s2)


def test_single_point_gives_log_half():
    """n = 1 under the logit: int sigma(f) N(f | 0, k) df = 1/2 by symmetry, on either branch."""
    for k, yy in ((1.7, 1.0), (0.2, -1.0), (5.0, 1.0), (5.1, -1.0), (400.0, 1.0)):
        fit = eq.ep_fit(np.array([[k]]), np.array([yy]), eq.LOGIT)
        assert abs(fit['logz'] - math.log(0.5)) <= 1e-14, k


def test_two_points_against_grid_quadrature():
    """test_ep_host's 2 x 2 K under the logit: log Z_EP within 1e-3 of the evidence
    int sigma(y1 f1) sigma(y2 f2) N(f | 0, K) df on a grid: EP's own approximation error."""
    K = np.array([[2.0, 1.2], [1.2, 1.5]])
    y = np.array([1.0, -1.0])
    g = np.linspace(-12.0, 12.0, 1201)
    F1, F2 = np.meshgrid(g, g, indexing='ij')
    pdf = multivariate_normal(np.zeros(2), K).pdf(np.stack([F1, F2], -1))
    Z = (expit(y[0] * F1) * expit(y[1] * F2) * pdf).sum() * (g[1] - g[0]) ** 2
    fit = eq.ep_fit(K, y, eq.LOGIT)
    print('2x2 logit: log Z_EP {0:.8f} quadrature {1:.8f}'.format(fit['logz'], math.log(Z)))
    assert abs(fit['logz'] - math.log(Z)) <= 1e-3


def test_parallel_fixed_point_equals_sequential_ep():
    """n = 40 under the logit, diff_tol = 1e-22: tau~, nu~ and mu of the parallel scheme against
    sequential EP (R&W Alg. 3.5) with the same moments, within 1e-9."""
    K, y = _se_case(40, 2, 0.7, 0)
    par = eq.ep_fit(K, y, eq.LOGIT, diff_tol=1e-22, max_sweeps=1000)
    tau, nu, mu = eq.ep_sequential(K, y, eq.LOGIT)
    errs = [np.abs(par[k] - v).max() for k, v in (('tau', tau), ('nu', nu), ('mu', mu))]
    print('logit parallel vs sequential EP (tau, nu, mu):', errs, 'sweeps', par['n_sweeps'])
    assert par['covered'] and max(errs) <= 1e-9


def test_probit_by_quadrature_is_the_closed_form_fit():
    """The rule as the probit's second moment routine: the two restatement fits of one problem
    agree far inside the parity yardstick, sweep for sweep."""
    import ep_restatement as ep
    K, y = _se_case(40, 2, 0.7, 0)
    a, b = ep.ep_fit(K, y), eq.ep_fit(K, y, eq.PROBIT)
    assert a['n_sweeps'] == b['n_sweeps'] and b['covered']
    d = max(float(np.abs(a[k] - b[k]).max()) for k in ('logz', 'mu', 'var', 'tau', 'nu'))
    print('probit: closed form vs quadrature, restatement: {0:.3e}'.format(d))
    assert d <= 1e-10


def test_python_classes_refuse_the_logit_without_the_switch_and_take_it_with():
    """Refused before any device call without quadrature=True (as before the switch existed);
    with it the two lazily built classes construct, and the four that look for the device at
    once get past the refusal (on a host without a device they stop at the missing device)."""
    import gpdemo.estimators as est
    import gpdemo.gradients as grd
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    import gpdemo.loo as loo
    import gpdemo.predict as prd
    from gpdemo import _native
    X, y = np.zeros((3, 2)), np.ones(3)
    kf = krn.make_kernel_func('ard', 1e-8)
    lazy = (
        lambda **k: prd.ISPredictor(X, y, kf, X, 8, proposal='ep', likelihood='logit', **k),
        lambda **k: loo.ISLeaveOneOut(X, y, kf, 8, proposal='ep', likelihood='logit', **k),
    )
    eager = (
        lambda **k: est.LogMarginalLikelihoodEPEstimator(X, y, kf, likelihood='logit', **k),
        lambda **k: est.LogMarginalLikelihoodApproxPosteriorISEstimator(
            X, y, kf, lpa.ep_approximation, likelihood='logit', **k),
        lambda **k: prd.EPPredictor(X, y, kf, X, likelihood='logit', **k),
        lambda **k: grd.EPGradient(X, y, kf, likelihood='logit', **k),
    )
    for make in lazy + eager:
        with pytest.raises(NotImplementedError):
            make()
        with pytest.raises(NotImplementedError):
            make(quadrature=False)
    for make in lazy:
        assert make(quadrature=True).quadrature is True
    for make in eager:
        try:
            obj = make(quadrature=True)
        except _native.NativeUnavailableError:
            continue
        getattr(obj, 'close', lambda: None)()
    with pytest.raises(ValueError):
        lpa.ep_approximation(np.eye(2), np.ones(2), likelihood='cauchit')
