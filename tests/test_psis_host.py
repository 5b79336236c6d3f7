"""Pareto-smoothed leave-one-out densities and the Pareto k-hat on the host: the
numpy restatement of include/apm.h's steps 1-6 on rows whose tail shape is known, its tail sizes
and fallback, the bound that the cap implies, and that combine_loo without khat is what it was."""
import numpy as np
import pytest
from scipy.special import logsumexp

import psis_restatement as pr


@pytest.mark.parametrize('k', [0.2, 0.7])
def test_khat_recovers_the_shape_of_exact_pareto_ratios(k):
    """200 rows of S = 256 log ratios t = k Exp(1): the ratios are Pareto with shape k, and the
    mean khat is within 0.1 of k (the prior pulls towards 0.5 with the weight of 10 of M + 10 = 58
    points, so the mean lies between k and 0.5). Measured: 0.265 at k = 0.2, 0.652 at k = 0.7."""
    t = k * np.random.RandomState(0).exponential(size=(200, 256))
    loo, khat = pr.psis_rows(t)
    print('k {0}: mean khat {1:.3f}'.format(k, khat.mean()))
    assert np.isfinite(khat).all() and np.isfinite(loo).all()
    assert abs(khat.mean() - k) <= 0.1


@pytest.mark.parametrize('S,M', [(4, 0), (24, 4), (25, 5), (64, 12), (100, 20), (130, 26),
                                 (256, 48)])
def test_tail_sizes_fallback_and_bound(S, M):
    """M at every S' the GPU tests use; below M = 5 khat is NaN and loo_psis is the raw
    -logsumexp exactly; always loo_psis >= -(mx + log S') (every smoothed ratio is capped at the
    largest raw one) and the results are finite. -inf entries (padding, weightless samples) do
    not count towards S'."""
    rs = np.random.RandomState(S)
    t = 1.5 * rs.standard_normal((20, S)) - np.log(S)
    padded = np.concatenate([t, np.full((20, 7), -np.inf)], axis=1)[:, rs.permutation(S + 7)]
    for row, prow in zip(t, padded):
        loo, khat, m = pr.psis_row(row)
        assert m == M == pr.tail_size(S)
        ploo, pkhat, pm = pr.psis_row(prow)
        assert pm == m
        np.testing.assert_allclose([ploo, pkhat], [loo, khat], rtol=1e-13, equal_nan=True)
        assert np.isfinite(loo) and loo >= -(row.max() + np.log(S))
        if M < 5:
            assert np.isnan(khat)
            assert loo == -(row.max() + logsumexp(row - row.max()))
        else:
            assert np.isfinite(khat)


def test_degenerate_tails_fall_back():
    """A tail of equal ratios (x_M <= x_1) and a tail level with the cut (x_1 <= 0) give NaN and
    the raw value; so does an empty row (S' = 0: +inf, the density of no sample)."""
    row = np.r_[np.linspace(-9.0, -4.0, 80), np.zeros(20)]
    loo, khat, M = pr.psis_row(row)
    assert M == 20 and np.isnan(khat) and loo == -logsumexp(row)
    flat = np.zeros(100)
    loo, khat, _ = pr.psis_row(flat)
    assert np.isnan(khat) and loo == -np.log(100.0)
    loo, khat, M = pr.psis_row(np.full(64, -np.inf))
    assert M == 0 and np.isnan(khat) and loo == np.inf


def test_mutations_move_the_restatement():
    """The two mutations test_gpu_psis.py must catch change khat by far more than its 1e-8."""
    t = 0.6 * np.random.RandomState(1).exponential(size=(8, 130))
    _, k0 = pr.psis_rows(t)
    _, k1 = pr.psis_rows(t, tail_shift=1)
    _, k2 = pr.psis_rows(t, drop_prior=True)
    assert np.abs(k1 - k0).min() > 1e-6 and np.abs(k2 - k0).min() > 1e-6


def test_combine_loo_without_khat_is_unchanged_and_with_it_counts():
    """Without khat the dict has exactly the keys and values it had; with it, khat is the
    per-point mean over the kept states that ignores NaN and n_bad counts the means above 0.7."""
    from gpdemo.loo import combine_loo
    rs = np.random.RandomState(3)
    loo, lpd = -1.0 + 0.3 * rs.standard_normal((7, 5)), -0.4 + 0.1 * rs.standard_normal((7, 5))
    old = combine_loo(loo, lpd, burn=1, thin=2)
    T = 3  # states 1, 3, 5
    lo_i = -(logsumexp(-loo[1::2], axis=0) - np.log(T))
    lp_i = logsumexp(lpd[1::2], axis=0) - np.log(T)
    assert sorted(old) == ['elpd_loo', 'loo', 'lpd', 'p_loo', 'se']
    np.testing.assert_array_equal(old['loo'], lo_i)
    np.testing.assert_array_equal(old['lpd'], lp_i)
    assert old['elpd_loo'] == float(lo_i.sum()) and old['se'] == float(np.sqrt(5 * np.var(lo_i)))
    assert old['p_loo'] == float(lp_i.sum()) - float(lo_i.sum())
    khat = np.full((7, 5), 0.4)
    khat[1::2, 1] = [0.9, np.nan, 0.6]      # mean of the two seen values: 0.75
    khat[1::2, 2] = np.nan                  # never fitted
    khat[0::2, 3] = 5.0                     # states that are not kept
    khat[1::2, 4] = [0.7, 0.7, 0.7]         # not above 0.7
    new = combine_loo(loo, lpd, burn=1, thin=2, khat=khat)
    for key in old:
        np.testing.assert_array_equal(new[key], old[key])
    assert sorted(set(new) - set(old)) == ['khat', 'n_bad']
    np.testing.assert_allclose(new['khat'][[0, 1, 3, 4]], [0.4, 0.75, 0.4, 0.7], rtol=1e-15)
    assert np.isnan(new['khat'][2]) and new['n_bad'] == 1
    with pytest.raises(ValueError):
        combine_loo(loo, lpd, khat=khat[:, :4])
