"""Inputs and fp64 references of the batch-count tests (test_batch_counts_host.py checks their
preconditions on the CPU, test_gpu_batch_counts.py runs them on the device). A plain module.

Per shape (N, S) a fixed family of chains: chain b has its own theta (theta_0 from a shuffled
grid over T0_RANGE, length scales around sqrt(D)) and its own two U buffers; a batch of B chains is
the first B of the family, so every reference is computed once per shape and shared by all B."""
import math

import numpy as np

import apm_oracle as orc
import grad_restatement as gr
from test_gpu_is_predict import _draws
from test_gpu_predict import _make_case

D = 5
EPS = 1e-8
M_TEST = 5
TOL = 5e-4          # nats: an IS / PriorMC estimate against the oracle
NEWTON_TOL = 1e-4   # the library's default diff_f_tol, the oracle's too
T0_RANGE = (-1.5, 3.5)
U_SCALE_STEP = 0.1
KF = orc.make_kernel_func('ard', EPS)

# (N, S) -> batch counts. (130, 64): nb = 3, nsb = 1, total = 3 B; (65, 130): nb = 2, nsb = 3 with a
# padded sample block, total = 6 B; (577, 64): nb = 10, a far update and an outer panel boundary
BATCHES = {(130, 64): tuple(range(7, 18)), (65, 130): (7, 8, 9, 12, 17), (577, 64): (9, 11)}
SHAPES = tuple(BATCHES)
SEEDS = {130: 100, 65: 365, 577: 877}
# offsets of the draws' seeds, fixed on the CPU so that test_batch_counts_host.py's separations
# hold (at N = 577 the first choice left one pair of buffers 3.6e-3 nats apart)
DRAW_SEEDS = {130: 0, 65: 0, 577: 2000}
LOO_BATCHES = {(130, 64): (9, 12, 17), (65, 130): (9,)}
DIAG_BATCHES = (9, 12)     # apm_u_eval_diag / apm_is_spread, (130, 64)
FAMILY_BATCHES = (9, 13)   # gradient, predictives, EP and EP-IS, (130, 64)


def grid(n, s, b):
    """(np, sp, nb, nsb, total) as host_ctx.cpp forms them: N and S padded to 64, and the 1-D grid
    of the fp32 u-path kernels, nb nsb nchains (ugemm_tile.h)."""
    np_, sp = (n + 63) // 64 * 64, (s + 63) // 64 * 64
    nb, nsb = np_ // 64, sp // 64
    return np_, sp, nb, nsb, nb * nsb * b


def n_chains(shape):
    return max(BATCHES[shape])


def perm(b, salt):
    """A fixed permutation of range(b) that is not the identity."""
    p = np.random.RandomState(1000 * salt + b).permutation(b)
    if (p == np.arange(b)).all():
        p = np.roll(p, 1)
    return p.astype(np.int64)


def make_thetas(n, count):
    rng = np.random.RandomState(4000 + n)
    t0 = np.linspace(T0_RANGE[0], T0_RANGE[1], count)[rng.permutation(count)]
    ls = 0.5 * math.log(D) + rng.uniform(-0.3, 0.1, size=(count, D))
    return np.column_stack([t0, ls])


def chain_draws(n, s, seed, b):
    """Chain b's U buffer: standard-normal draws times 1 + U_SCALE_STEP b, held exactly by fp32
    (the device keeps U in both precisions). The scale is what tells the buffers apart: where the
    Gaussian proposal fits well (small theta_0) the log weights barely depend on u, and with
    N(0, 1) draws in every buffer an estimate formed with another chain's buffer would lie within
    2e-5 nats of the right one. A log weight is a function of (theta, U) whatever U's law, so the
    oracle and the device are compared on it as on any other input."""
    u = _draws(n, s, seed + b) * (1.0 + U_SCALE_STEP * b)
    return u.astype(np.float32).astype(np.float64)


_REFS = {}


def refs(shape):
    """The shape's case, thetas, draws and oracle values, computed once and left unchanged.
    Per chain b: st (theta_state_pushthrough with K, z and cst added), diffs (the Newton loop's
    mean squared steps), ops / lops (cubic-op counts of the IS and Laplace theta-calls), is1 / is2
    (IS estimates on U1[b] / U2[b]), pm1 / pm2 (PriorMC), lml (the Laplace estimator); rc is the
    reference's cache tuple (K_chol, C_chol, f_post)."""
    if shape in _REFS:
        return _REFS[shape]
    n, s = shape
    T = n_chains(shape)
    c = _make_case(n, D, M_TEST, 'ard', SEEDS[n])
    X, y = c['X'], c['y']
    th = make_thetas(n, T)
    U1 = [chain_draws(n, s, 50000 + 100 * n + DRAW_SEEDS[n], b) for b in range(T)]
    U2 = [chain_draws(n, s, 60000 + 100 * n + DRAW_SEEDS[n], b) for b in range(T)]
    r = dict(c=c, thetas=th, U1=U1, U2=U2, n=n, s=s, T=T)
    for key in ('st', 'rc', 'diffs', 'ops', 'lops', 'is1', 'is2', 'pm1', 'pm2', 'lml', 'cst_bound'):
        r[key] = []
    for b in range(T):
        K = np.empty((n, n))
        KF(K, X, th[b])
        st = orc.theta_state_pushthrough(K, y)
        st['K'] = K
        st['z'] = st['a'] + st['W'] * st['f_post']
        st['cst'] = 0.5 * st['f_post'].dot(st['z']) - 0.5 * st['logdet_B']
        v1, rc, ops = orc.is_estimate(X, y, KF, U1[b], th[b])
        lml, lops = orc.laplace_estimate(X, y, KF, th[b])
        r['st'].append(st)
        r['rc'].append(rc)
        r['diffs'].append(gr.newton(K, y, NEWTON_TOL)['diffs'])
        r['ops'].append(ops)
        r['lops'].append(lops)
        r['is1'].append(v1)
        r['is2'].append(orc.is_estimate(X, y, KF, U2[b], None, rc)[0])
        r['pm1'].append(orc.priormc_estimate(X, y, KF, U1[b], K_chol=rc[0])[0])
        r['pm2'].append(orc.priormc_estimate(X, y, KF, U2[b], K_chol=rc[0])[0])
        r['lml'].append(lml)
        # test_slot_state_vs_oracle's bound on |d cst|
        r['cst_bound'].append(1e-8 * np.abs(st['f_post']).max() * np.abs(st['z']).sum() +
                              1e-8 * max(1., abs(st['cst'])))
    _REFS[shape] = r
    return r


def cross_estimates(r, which='U1'):
    """(T, T): the IS estimate of chain b's state formed with chain c's buffer."""
    X, y, T = r['c']['X'], r['c']['y'], r['T']
    return np.array([[orc.is_estimate(X, y, KF, r[which][c], None, r['rc'][b])[0]
                      for c in range(T)] for b in range(T)])
