"""Host side of the Laplace-gradient path: the numpy restatement the device is compared with
(tests/grad_restatement.py) agrees with central differences of its own log marginal likelihood,
the Gaussian-prior arithmetic of gpdemo/gradients.py matches hand-computed values, arguments are
validated without a device, and the C-ABI declares the entry point."""
import math
import os
import re

import numpy as np
import pytest

import cov_restatement as cr
import grad_restatement as gr
from cov_restatement import Cov
from conftest import REPO

EPS = 1e-8
# (n, d, kind, seed): one point, a full tile with d across two LDS chunks, tiles that are not
# full, the isotropic kernel
SHAPES = [(1, 1, 'ard', 301), (64, 33, 'ard', 364), (130, 5, 'ard', 430), (200, 3, 'iso', 500)]


@pytest.mark.parametrize('n,d,kind,seed', SHAPES)
def test_restatement_vs_central_differences(n, d, kind, seed):
    """Formula against central differences (h = 1e-5) of the restatement's own LML at a Newton
    tolerance of 1e-24 (to convergence), at theta_0 = 0.3, 3.0, -1.0: 1e-6 of max(1, max|fd|).
    The worst measured over these shapes and n = 600 was 3.5e-9, so the bound leaves ~300x for
    another BLAS while a wrong sign or a factor of 2 misses it by six orders of magnitude."""
    c = gr.make_case(n, d, kind, seed)
    for th in c['thetas']:
        ref = cr.laplace_grad(Cov('se', kind), c['X'], c['y'], th, EPS, tol=1e-24)
        fd = gr.central_differences(lambda t: cr.lml(Cov('se', kind), c['X'], c['y'], t, EPS, tol=1e-24), th)
        err = np.abs(ref['grad'] - fd).max() / max(1.0, np.abs(fd).max())
        print('restatement vs fd {0}: {1:.3e}'.format((n, d, kind, th[0]), err))
        assert err <= 1e-6


def test_edge_case_seeds_keep_their_newton_margins():
    """The inputs of test_gpu_laplace_edges.py (tests/edge_cases.py), checked without a device:
    at every size and theta it uses, the restatement's last Newton diff is <= 1e-14 / 100 and the
    one before >= 100 x 1e-14 (the gradient's tolerance), and the first diff below 1e-4 (the
    predictor's and apm_laplace's) is <= 1e-4 / 3, the one before >= 3e-4: device and restatement
    cannot disagree on an iteration count at either tolerance."""
    import edge_cases as ec
    keys = [(None, 'ard', n) for n in ec.SIZES] + sorted(ec.MATERN)
    for family, kind, n in keys:
        c = ec.case(n, family, kind)
        assert len(c['thetas']) == (3 if n <= 513 else 2)
        for th in c['thetas']:
            diffs = gr.newton(ec.gram(c, th), c['y'], ec.GRAD_TOL)['diffs']
            k = ec.fit_iterations(diffs)
            print('edge margins {0}: {1} iterations, last diffs {2:.2e} {3:.2e}; {4} at 1e-4, '
                  'diffs {5:.2e} {6:.2e}'.format((family, kind, n, float(th[0])), len(diffs), diffs[-2],
                                                  diffs[-1], k, diffs[k - 2], diffs[k - 1]))
            assert diffs[-1] <= ec.GRAD_TOL / 100.0 and diffs[-2] >= 100.0 * ec.GRAD_TOL
            assert k >= 2 and diffs[k - 1] <= ec.FIT_TOL / 3.0 and diffs[k - 2] >= 3.0 * ec.FIT_TOL
            assert ec.margins_hold(diffs)


def test_restatement_epsilon_rule_is_visible():
    """With epsilon = 1e-2 the wrong reading (epsilon kept on dK/dtheta_0's diagonal) moves
    grad[0] by epsilon * trace(M), far above the central-difference error."""
    c = gr.make_case(64, 33, 'ard', 364)
    th = c['thetas'][0]
    fd = gr.central_differences(lambda t: cr.lml(Cov('se', 'ard'), c['X'], c['y'], t, 1e-2, tol=1e-24), th)
    right = cr.laplace_grad(Cov('se', 'ard'), c['X'], c['y'], th, 1e-2, tol=1e-24)['grad']
    wrong = cr.laplace_grad(Cov('se', 'ard'), c['X'], c['y'], th, 1e-2, tol=1e-24, wrong='eps_in_dk0')['grad']
    assert np.abs(right - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max())
    assert abs(wrong[0] - fd[0]) > 1e-4 and np.array_equal(wrong[1:], right[1:])


def test_gaussian_prior_combination_by_hand():
    import gpdemo.gradients as gd
    thetas = np.array([[1.0, -2.0], [0.5, 0.0]])
    lml = np.array([-3.0, 4.0])
    grad = np.array([[0.25, -0.5], [1.0, 2.0]])
    val, g = gd.add_gaussian_log_prior(thetas, lml, grad, [0.0, 1.0], [2.0, 3.0])
    c = -math.log(2.0) - math.log(3.0) - math.log(2.0 * math.pi)
    want = [-3.0 + c - 0.5 * (0.25 + 1.0), 4.0 + c - 0.5 * (0.0625 + 1.0 / 9.0)]
    assert np.allclose(val, want, rtol=0, atol=1e-15)
    assert np.allclose(g, [[0.25 - 0.25, -0.5 + 3.0 / 9.0], [1.0 - 0.125, 2.0 + 1.0 / 9.0]],
                       rtol=0, atol=1e-15)
    # scalars broadcast over the components; a single theta is one row
    v1, g1 = gd.add_gaussian_log_prior(thetas[0], lml[:1], grad[:1], 0.0, 3.0)
    assert abs(v1[0] - (-3.0 - 2.0 * math.log(3.0) - math.log(2.0 * math.pi) - 2.5 / 9.0)) <= 1e-15
    assert np.allclose(g1, [[0.25 - 1.0 / 9.0, -0.5 + 2.0 / 9.0]], rtol=0, atol=1e-15)
    # inputs are left unchanged
    assert grad[0, 0] == 0.25 and lml[0] == -3.0


def test_argument_validation_without_a_device():
    import gpdemo
    import gpdemo.gradients as gd
    assert gpdemo.LaplaceGradient is gd.LaplaceGradient
    with pytest.raises(NotImplementedError, match='make_kernel_func'):
        gd.LaplaceGradient(np.zeros((4, 2)), np.ones(4), lambda K, X, theta: None)
    th = np.zeros((2, 3))
    with pytest.raises(ValueError):
        gd.add_gaussian_log_prior(th, np.zeros(3), np.zeros((2, 3)), 0.0, 1.0)
    with pytest.raises(ValueError):
        gd.add_gaussian_log_prior(th, np.zeros(2), np.zeros((2, 2)), 0.0, 1.0)
    with pytest.raises(ValueError):
        gd.add_gaussian_log_prior(th, np.zeros(2), np.zeros((2, 3)), 0.0, 0.0)
    with pytest.raises(ValueError):
        gd.add_gaussian_log_prior(th, np.zeros(2), np.zeros((2, 3)), np.zeros(2), 1.0)


def test_entry_point_is_declared_and_bound():
    from gpdemo import _native
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    m = re.search(r'int\s+apm_laplace_grad\s*\(([^)]*)\)', txt)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 9 and args[0].startswith('apm_ctx') and 'ldg' in args[6]
    assert 'apm_laplace_grad' in _native.exported_symbols()
    assert hasattr(_native.load_library(check_device=False), 'apm_laplace_grad')
    assert hasattr(_native.Context, 'laplace_grad')
