"""Inputs of tests/test_gpu_laplace_edges.py: sizes at the panel boundaries of the solve-only form
of the fp64 schedule (host_chol64.cpp chol_solve_rows), the data seeds, and the condition those seeds were chosen by. A plain
module, shared with test_grad_host.py, which asserts the condition without a device.

nb = ceil(N / 64) tile rows, outer panels of 8 tiles: N = 65 and 128 (nb = 2: the first depth-2
super-tile update of the gradient's second pass, padded and full), 512 (nb = 8: one full panel,
no padding row), 513 (nb = 9: a one-tile-column trailing part, a depth-8 update on the 64 x 64
kernel, a last panel of one tile), 1024, 1025, 1089 (nb = 16, 17, 18: two and three panels).

Data and thetas are grad_restatement.make_case(N, 4, kind, seed): theta_0 = 0.3, 3.0, -1.0, length
scales around sqrt(d). N <= 513 uses all three thetas, N >= 1024 the first two (the restatement
takes about 2 s per theta there). The seeds were searched on the CPU so that device and
restatement cannot disagree on a Newton iteration count (`margins_hold`): every size uses its
full set of thetas.
"""
import numpy as np

import grad_restatement as gr
from cov_restatement import Cov

EPS = 1e-8
D = 4
GRAD_TOL = 1e-14       # the gradient's Newton tolerance: a factor 100 on both sides
FIT_TOL = 1e-4         # the predictor's and apm_laplace's: a factor 3 on both sides
SIZES = (65, 128, 512, 513, 1024, 1025, 1089)
# the first seed from 3065, 3128, 3513, 3513, 4027, 4025, 4095 upwards that meets both conditions
# for every theta of the size (N = 65 needed 32 tries; 3128 meets the 1e-14 one only)
SEEDS = {65: 3096, 128: 3130, 512: 3513, 513: 3513, 1024: 4027, 1025: 4025, 1089: 4095}
# (family, kind, N) -> seed: the two-pass k_grad_reduce of the Matern kinds (from 5513, 6025)
MATERN = {('52', 'ard', 513): 5517, ('32', 'iso', 1025): 6025}
# test-row counts per size: mb = 2 everywhere; at N = 513 (np = 576) one row, mb = 3, mb = nb and
# a second block of one row; at N = 1025 an odd mb against two panels
PREDICT_M = {n: (70,) for n in SIZES}
PREDICT_M[513] = (1, 70, 129, 576, 577)
PREDICT_M[1025] = (70, 129)
COV_SIZES = (128, 513, 1025)
I_EQ, I_FAR = 7, 3     # test row 0 coincides with training row I_EQ; the last one is far from I_FAR


def n_thetas(n):
    return 3 if n <= 513 else 2


_CASES = {}


def case(n, family=None, kind='ard'):
    """make_case's dict with the thetas the size uses, drawn once and left unchanged."""
    key = (family, kind, n)
    if key not in _CASES:
        seed = SEEDS[n] if family is None else MATERN[key]
        c = gr.make_case(n, D, kind, seed)
        c['thetas'] = c['thetas'][:n_thetas(n)].copy()
        c['family'] = family
        _CASES[key] = c
    return _CASES[key]


def cov(c):
    return Cov(c['family'] or 'se', c['kind'])


def gram(c, theta):
    return cov(c).gram(c['X'], theta, EPS)


def gram_cross(c, Xs, theta):
    """k(Xs_i, X_j) without epsilon: the SE one as test_gpu_predict forms it, from the C oracle's
    Gram of the stacked points."""
    if c['family'] is not None:
        return cov(c).gram_cross(Xs, c['X'], theta)
    n = c['n']
    G = cov(c).gram(np.concatenate([c['X'], Xs]), theta, EPS)
    return G[n:, :n].copy()


def predict_inputs(c, m, shift=50.0):
    """As test_gpu_predict._make_case: normal rows; for m >= 3 row 0 coincides with a training row
    and the last row is `shift` away in every coordinate (k* underflows to exactly 0; the Matern
    kinds decay exponentially only and need shift = 1000, as test_gpu_matern). m = 577 (np + 1 at
    N = 513) is the m = 576 set and one more far row."""
    if m == 577:
        return np.concatenate([predict_inputs(c, 576, shift), c['X'][I_FAR + 1][None] + shift])
    Xs = np.random.RandomState(90000 + c['n']).normal(size=(m, c['d']))
    if m >= 3:
        Xs[0] = c['X'][I_EQ]
        Xs[-1] = c['X'][I_FAR] + shift
    return Xs


def fit_iterations(diffs, tol=FIT_TOL):
    """Iterations the Newton loop takes at `tol`, read from the diffs of a run at a tighter one."""
    return next(i for i, x in enumerate(diffs) if x < tol) + 1


def margins_hold(diffs):
    """The condition on a seed, from the diffs of one restatement Newton run at GRAD_TOL: the last
    diff <= GRAD_TOL / 100 and the one before >= 100 GRAD_TOL; the first diff below FIT_TOL <=
    FIT_TOL / 3 and the one before >= 3 FIT_TOL. diff's own relative error is ~1e-9 (f's rounding
    over the step), far inside either factor."""
    k = fit_iterations(diffs)
    return (diffs[-1] <= GRAD_TOL / 100.0 and diffs[-2] >= 100.0 * GRAD_TOL and
            diffs[k - 1] <= FIT_TOL / 3.0 and (k < 2 or diffs[k - 2] >= 3.0 * FIT_TOL))
