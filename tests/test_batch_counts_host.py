"""The preconditions of test_gpu_batch_counts.py, on the CPU with the oracle alone: the grid
arithmetic that makes 7 to 17 chains reach every remainder branch of the XCD-aware work-item
orders, that the chains' reference values lie far enough apart for a device that answered with
another chain's state or buffer to fail the oracle comparison (not only the bitwise one), that
chains with different Newton iteration counts coexist in a batch, and that no chain is left
out."""
import numpy as np
import pytest

import batch_counts_cases as bc

SEP = 10.0  # separation of distinct chains' references, in units of the comparison's tolerance


@pytest.fixture(scope='module', params=bc.SHAPES, ids=lambda s: 'N{0}-S{1}'.format(*s))
def r(request):
    return bc.refs(request.param)


def test_grid_arithmetic_reaches_every_remainder():
    """np, sp, nb, nsb and total = nb nsb B as host_ctx.cpp forms them; total & 7 over the batch
    counts covers 0 .. 7 at (130, 64) and at least three values at (65, 130); 7 is the last plain
    order, 17 the first count past two chains per XCD."""
    assert bc.grid(130, 64, 9) == (192, 64, 3, 1, 27)
    assert bc.grid(65, 130, 9) == (128, 192, 2, 3, 54)
    assert bc.grid(577, 64, 11) == (640, 64, 10, 1, 110)
    rem = {shape: {bc.grid(shape[0], shape[1], b)[4] & 7 for b in bs}
           for shape, bs in bc.BATCHES.items()}
    assert rem[130, 64] == set(range(8))
    assert {b: bc.grid(130, 64, b)[4] & 7 for b in range(9, 16)} == \
        {9: 3, 10: 6, 11: 1, 12: 4, 13: 7, 14: 2, 15: 5}
    assert bc.grid(130, 64, 8)[4] & 7 == 0 and bc.grid(130, 64, 16)[4] & 7 == 0
    assert len(rem[65, 130]) >= 3
    assert all(r != 0 for r in (bc.grid(577, 64, b)[4] & 7 for b in bc.BATCHES[577, 64]))
    for bs in bc.BATCHES.values():
        assert min(bs) >= 7 and max(bs) <= 17
    assert min(bc.BATCHES[130, 64]) == 7 and max(bc.BATCHES[130, 64]) == 17
    # the sub-lists are batches of the sweep, and every one has a nonzero remainder in it
    for shape, bs in bc.LOO_BATCHES.items():
        assert set(bs) <= set(bc.BATCHES[shape])
        assert any(bc.grid(shape[0], shape[1], b)[4] & 7 for b in bs)
    assert set(bc.DIAG_BATCHES) | set(bc.FAMILY_BATCHES) <= set(bc.BATCHES[130, 64])


def test_index_permutations_are_not_the_identity():
    for b in range(7, 18):
        for salt in (1, 2, 3):
            p = bc.perm(b, salt)
            assert sorted(p) == list(range(b)) and (p != np.arange(b)).any()
        assert (bc.perm(b, 1) != bc.perm(b, 2)).any()


def _min_gap(v):
    v = np.asarray(v, dtype=np.float64)
    d = np.abs(v[:, None] - v[None])
    d[np.diag_indices_from(d)] = np.inf
    return float(d.min())


def test_every_reference_is_finite_and_every_chain_converges(r):
    """Zero exclusions: every chain of every shape has a converged oracle fit (the oracle raises
    where its Newton loop does not converge, so refs() returning is the statement) with finite
    references, distinct thetas and distinct buffers."""
    excluded = []
    for b in range(r['T']):
        vals = [r[k][b] for k in ('is1', 'is2', 'pm1', 'pm2', 'lml')] + [r['st'][b]['cst']]
        if not (np.isfinite(vals).all() and np.isfinite(r['st'][b]['C_chol']).all() and
                r['diffs'][b][-1] < bc.NEWTON_TOL):
            excluded.append(b)
    assert excluded == []
    assert r['T'] == max(bc.BATCHES[r['n'], r['s']])
    assert len({tuple(t) for t in r['thetas']}) == r['T']
    assert bc.T0_RANGE[0] <= r['thetas'][:, 0].min() and r['thetas'][:, 0].max() <= bc.T0_RANGE[1]
    for which in ('U1', 'U2'):
        assert len({u.tobytes() for u in r[which]}) == r['T']
        assert all((u == u.astype(np.float32)).all() for u in r[which])


def test_newton_counts_differ_and_cannot_flip(r):
    """At least three distinct Newton iteration counts among the chains (so converged and
    iterating chains coexist under the Live gate of every batch size that holds them), the
    reference's op counts follow them, and the stop measure of the last iteration is below 0.99
    tol and the one before above 1.01 tol: the mixed-precision Newton's mode agrees to 1e-8
    relative, which moves mean((f_new - f)^2) ~ 1e-4 by parts in 1e-6, so the device cannot take
    another count."""
    iters = [len(d) for d in r['diffs']]
    assert len(set(iters)) >= 3
    assert len(set(iters[:7])) >= 2  # already in the smallest batch
    for b, d in enumerate(r['diffs']):
        assert d[-1] < 0.99 * bc.NEWTON_TOL and d[-2] > 1.01 * bc.NEWTON_TOL, (b, d[-2:])
        assert r['st'][b]['n_ops'] == iters[b] + 1
        assert r['ops'][b] == iters[b] + 3 and r['lops'][b] == iters[b]


def test_references_of_distinct_chains_are_far_apart(r):
    """IS, PriorMC and Laplace estimates and cst of distinct chains differ pairwise by at least
    10 x the tolerance they are compared under, and so does a chain's IS estimate formed with
    any other chain's buffer from its own."""
    T = r['T']
    for key in ('is1', 'is2', 'pm1', 'pm2'):
        gap = _min_gap(r[key])
        print('{0}: smallest pairwise gap {1:.3e} nats'.format(key, gap))
        assert gap >= SEP * bc.TOL, (key, gap)
    lml = np.array(r['lml'])
    assert _min_gap(lml) >= SEP * 1e-7 * max(1.0, np.abs(lml).max())
    cst = [st['cst'] for st in r['st']]
    print('cst: smallest pairwise gap {0:.3e}, largest bound {1:.3e}'.format(
        _min_gap(cst), max(r['cst_bound'])))
    assert _min_gap(cst) >= SEP * max(r['cst_bound'])
    for which, own in (('U1', 'is1'), ('U2', 'is2')):
        M = bc.cross_estimates(r, which)
        assert np.isfinite(M).all()
        np.testing.assert_allclose(np.diag(M), r[own], rtol=0, atol=1e-9)
        d = np.abs(M - np.diag(M)[:, None])
        d[np.diag_indices(T)] = np.inf
        print('{0}: a chain with another chain\'s buffer is off by at least {1:.3e} nats'
              .format(which, d.min()))
        assert d.min() >= SEP * bc.TOL, (which, d.min())
