"""The left-looking far updates of the Newton factorisation (host_newton.cpp chol_range32,
far_update_left32; k_chol_update32_q256's multi-panel depth loop) against the right-looking
schedule they replace (APM_FAR_LEFT=0) and against the fp64 oracle.

Behind outer panel p the far tiles of panel p + 2's columns take the contributions of panels
0 .. p in one launch; the right-looking schedule gives every column right of panel p + 1 panel
p's alone. A tile receives the same fp16x3 slices in the same order either way, so every result
must be bitwise the same. The two schedules differ from the fourth outer panel (nb > 24) on:
  N = 1537  nb = 25: the last panel is one tile wide (quad launch + the 64x64 kernel's launch)
  N = 1601  nb = 26: the smallest size with a launch of depth two (a two-tile last panel)
  N = 2049  nb = 33: five panels, the last one tile wide
  N = 2113  nb = 34: five panels, an odd number of quad rows, a ragged last panel and tile
Inputs and helpers are those of test_gpu_slot_state.py; the third chain is the bench's
stationary state (tests/golden/stationary_thetas.npy row 45) cut to D length-scales.
"""
import os

import numpy as np
import pytest

import test_gpu_slot_state as ss

pytestmark = pytest.mark.gpu

D = ss.D
SIZES = (1537, 1601, 2049, 2113)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _thetas3():
    st = np.load(os.path.join(HERE, 'golden', 'stationary_thetas.npy'))[45, :D + 1]
    return np.vstack([ss._thetas(), st])


_RUNS = {}


def _run(nat, monkeypatch, n, thetas, key, **env):
    """One IS theta-call of the chains `thetas` at size n into slots 0 .. (their own context):
    (values, status, n_cubic_ops, [slot_read of every chain]); kept per (n, key, env)."""
    k = (n, key, tuple(sorted(env.items())))
    if k not in _RUNS:
        X, y = ss._data(n)
        nch = len(thetas)
        for name, v in env.items():
            monkeypatch.setenv(name, str(v))
        ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, 8, max_batch=nch, n_slots=nch, n_ubufs=1)
        for name in env:
            monkeypatch.delenv(name)
        ctx.u_upload(0, ss._draws(n)[0])
        out, st, nops = ctx.theta_eval(nat.EST_IS, thetas, [0] * nch, list(range(nch)))
        slots = [ctx.slot_read(b) if st[b] == 0 else None for b in range(nch)]
        ctx.close()
        _RUNS[k] = (out, st, nops, slots)
    return _RUNS[k]


def _assert_same_chain(a, b, ia, ib):
    """chain ia of run a is bitwise chain ib of run b"""
    assert a[1][ia] == 0 and b[1][ib] == 0, (a[1], b[1])
    assert a[0][ia] == b[0][ib], (a[0][ia], b[0][ib])
    assert a[2][ia] == b[2][ib]
    for x, y in zip(a[3][ia], b[3][ib]):  # L, f_post, g, cst
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('n', SIZES)
def test_left_looking_is_bitwise_right_looking(nat, monkeypatch, n):
    th = _thetas3()
    new = _run(nat, monkeypatch, n, th, 'three')
    old = _run(nat, monkeypatch, n, th, 'three', APM_FAR_LEFT=0)
    np.testing.assert_array_equal(new[1], np.zeros(3, new[1].dtype))
    np.testing.assert_array_equal(new[0], old[0])
    np.testing.assert_array_equal(new[1], old[1])
    np.testing.assert_array_equal(new[2], old[2])
    for b in range(3):
        _assert_same_chain(new, old, b, b)


@pytest.mark.parametrize('skew', [1, 3])
def test_left_looking_edges_under_stream_skew(nat, monkeypatch, skew):
    """The schedule's edges (df[p] main -> stream3 ahead of the far launch that reads panels
    0 .. p's planes, far[p] stream3 -> main ahead of the narrow update of the same tiles) with
    the far stream, or both streams, held back by delay kernels (APM_SKEW): bitwise the
    undelayed results at five panels."""
    n = 2113
    th = _thetas3()
    new = _run(nat, monkeypatch, n, th, 'three')
    skewed = _run(nat, monkeypatch, n, th, 'three', APM_SKEW=skew)
    for b in range(3):
        _assert_same_chain(skewed, new, b, b)


@pytest.mark.parametrize('n', SIZES[1:])
def test_slot_state_vs_oracle_past_four_panels(nat, monkeypatch, n):
    """The default path's slot state of the chains theta_0 = 0, 2 against
    theta_state_pushthrough under test_gpu_slot_state.py's bounds (N = 1537 is checked there)."""
    new = _run(nat, monkeypatch, n, _thetas3(), 'three')
    for ti in range(2):
        st = ss._state(n, ti)
        assert new[1][ti] == 0
        L, f, g, cst = new[3][ti]
        dl, dg = ss._rel(L, np.tril(st['C_chol'])), ss._rel(g, st['g'])
        df, dc = ss._rel(f, st['f_post']), abs(cst - st['cst'])
        cst_bound = (1e-8 * np.abs(st['f_post']).max() * np.abs(st['z']).sum() +
                     1e-8 * max(1., abs(st['cst'])))
        print('n = {0} t0 = {1}: |d cst| = {2:.3e} (bound {3:.3e}), max|dL|/max|L| = {4:.3e}, '
              'max|dg|/max|g| = {5:.3e}, max|df|/max|f| = {6:.3e}'
              .format(n, ss.T0S[ti], dc, cst_bound, dl, dg, df))
        assert new[2][ti] == st['n_ops'] + 2
        assert df <= 1e-8
        assert dl <= 1e-5
        assert dg <= 2e-6
        assert dc <= cst_bound, (dc, cst_bound)


def test_out_of_range_chain_falls_back(nat, monkeypatch):
    """A chain outside fp16x3's range (theta_0 >= 19) sends the batch to the right-looking
    schedule on the 128-row super-tiles: every status is 0 and the in-range chains are bitwise
    those of the batch without it."""
    n = 1537
    th = _thetas3()
    big = np.vstack([th, th[1]])
    big[-1, 0] = 19.5
    alone = _run(nat, monkeypatch, n, th, 'three')
    mixed = _run(nat, monkeypatch, n, big, 'three+out-of-range')
    np.testing.assert_array_equal(mixed[1], np.zeros(4, mixed[1].dtype))
    for b in range(3):
        _assert_same_chain(mixed, alone, b, b)


def test_converged_chain_leaves_early(nat, monkeypatch):
    """theta_0 = 0 converges two Newton iterations before theta_0 = 2 (7 and 9 cubic operations
    by the oracle): the last factorisations run with one live chain, whose results are bitwise
    those it has alone."""
    n = 1537
    th = ss._thetas()
    both = _run(nat, monkeypatch, n, th, 'two')
    slow = _run(nat, monkeypatch, n, th[1:], 'slow')
    assert both[2][0] < both[2][1], both[2]
    _assert_same_chain(both, slow, 1, 0)
