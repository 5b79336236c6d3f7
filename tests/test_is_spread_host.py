"""Replicate spread and weight diagnostics of the IS estimate on the host: the
restatement's block quantities (tests/is_spread_restatement.py) against is_consistent and their
own identities, the delta-method statement at the study's size, the selection logic of
tune_n_imp, the C-ABI declarations and the refusals made before any device call. No device."""
import os
import re

import numpy as np
import pytest

import epis_restatement as eis
import is_spread_restatement as sr
from cov_restatement import Cov
from conftest import REPO

EPS = 1e-8
# the study's problem: n = 130, d = 5, SE-ARD, length scales e^0.5; 64 replicates x 256 samples.
# Seeds recorded for the delta-method test: data 2003, draws 2010. The restatement alone gives,
# at B = 64, sd vs sqrt(mean(1/ess - 1/B)): 0.161 vs 0.148 (theta_0 = 0.3, Laplace), 0.055 vs
# 0.054 (0.3, EP), 1.66 vs 0.72 (3, Laplace); seeds 2001 and 2002 gave 0.186 / 0.178, 0.060 /
# 0.059, 2.05 / 0.75 and 0.195 / 0.169, 0.063 / 0.061, 2.03 / 0.74.
STUDY_SEED, DRAW_SEED = 2003, 2010
N_REP, S, B = 64, 256, 64


@pytest.fixture(scope='module')
def study():
    """Log weights of the 64 x 256 draws per (theta_0, proposal), computed once."""
    rng = np.random.RandomState(STUDY_SEED)
    X = rng.normal(size=(130, 5))
    y = np.where(X[:, 0] + 0.5 * rng.normal(size=130) > 0, 1.0, -1.0)
    ns = np.random.RandomState(DRAW_SEED).normal(size=(130, N_REP * S))
    out = {'y': y, 'ns': ns}
    for s0 in (0.3, 3.0):
        K = Cov('se', 'ard').gram(X, np.r_[s0, np.full(5, 0.5)], EPS)
        for name, st in (('laplace', eis.laplace_state(K, y)), ('ep', eis.state(K, y))):
            out[s0, name] = dict(st=st, lw=sr.log_weights(y, st, ns))
    return out


def test_full_block_is_is_consistent(study):
    """B = S: the one block's logf is is_consistent's value, per replicate."""
    for key in ((0.3, 'laplace'), (3.0, 'ep')):
        c = study[key]
        for r in (0, 17, 63):
            ns = study['ns'][:, r * S:(r + 1) * S]
            logf, ess, wmax = sr.blocks(c['lw'][r * S:(r + 1) * S], S)
            ref = eis.is_consistent(study['y'], c['st'], ns)
            assert logf.shape == (1,) and abs(logf[0] - ref) <= 1e-12 * max(1.0, abs(ref))
            assert 1.0 <= ess[0] <= S and 1.0 / S <= wmax[0] <= 1.0


def test_block_estimates_average_to_the_full_estimate(study):
    """The log-mean-exp of equal-size block estimates is the full estimate, to 1e-12; leftover
    samples are ignored."""
    lw = study[3.0, 'laplace']['lw'][:S]
    full = sr.blocks(lw, S)[0][0]
    for b in (1, 16, 64, 128):
        logf = sr.blocks(lw, b)[0]
        assert logf.shape == (S // b,)
        assert abs(sr.log_mean_exp(logf) - full) <= 1e-12 * max(1.0, abs(full))
    logf, ess, wmax = sr.blocks(lw[:50], 16)  # S = 50: three blocks, two samples left over
    assert logf.shape == (3,)
    assert np.array_equal(logf, sr.blocks(lw[:48], 16)[0])


def test_single_sample_blocks_and_degenerate_blocks(study):
    lw = study[0.3, 'ep']['lw'][:S]
    logf, ess, wmax = sr.blocks(lw, 1)
    assert np.array_equal(logf, lw)
    assert np.array_equal(ess, np.ones(S)) and np.array_equal(wmax, np.ones(S))
    bad = lw[:8].copy()
    bad[:4] = -np.inf
    logf, ess, wmax = sr.blocks(bad, 4)
    assert logf[0] == -np.inf and ess[0] == 0.0 and wmax[0] == 0.0
    assert np.isfinite(logf[1]) and ess[1] >= 1.0


def test_delta_method_holds_until_the_weights_degenerate(study):
    """With healthy weights (theta_0 = 0.3, both proposals) the spread of the B = 64 block
    estimates over independent draws and the one-call figure sqrt(mean(1/ess - 1/B)) agree within
    a factor 1.5; at theta_0 = 3 with the Laplace proposal (a median of 2 effective samples out of
    64) the spread exceeds it by more than 1.5x."""
    got = {}
    for key in ((0.3, 'laplace'), (0.3, 'ep'), (3.0, 'laplace')):
        logf, ess, _ = sr.blocks(study[key]['lw'], B)
        assert logf.shape == (N_REP * S // B,)
        got[key] = (float(np.std(logf, ddof=1)), sr.delta_sd(ess, B), float(np.median(ess)))
        print('theta_0 {0} {1}: sd {2:.4f} delta {3:.4f} median ess {4:.1f}'
              .format(*key + got[key]))
    for key in ((0.3, 'laplace'), (0.3, 'ep')):
        sd, dl, _ = got[key]
        assert dl / 1.5 <= sd <= 1.5 * dl
    sd, dl, med = got[3.0, 'laplace']
    assert sd > 1.5 * dl and med < 4.0
    assert got[0.3, 'ep'][0] < got[0.3, 'laplace'][0]


def _curve(sds):
    return {b: {'sd': sd, 'block': b} for b, sd in sds.items()}


def test_select_n_imp_on_synthetic_curves():
    from gpdemo import estimators as est
    easy = _curve({64: 0.4, 128: 0.3, 256: 0.2})
    mid = _curve({64: 1.4, 128: 0.9, 256: 0.7})
    hard = _curve({64: 1.7, 128: 1.4, 256: 1.3})
    assert est.select_n_imp([easy]) == 64
    assert est.select_n_imp([easy, mid]) == 128          # every theta must meet the target
    assert est.select_n_imp([easy, mid], target_sd=0.8) == 256
    assert est.select_n_imp([easy, mid, hard]) is None   # even n_imp misses: no extrapolation
    assert est.select_n_imp([easy, mid], target_sd=0.1) is None
    assert est.select_n_imp([mid], target_sd=0.9) == 128  # the bound is met with equality
    assert est.select_n_imp([_curve({64: float('nan'), 128: 0.5})]) == 128
    assert est.select_n_imp([]) is None
    # not monotone (a noisy measurement): the smallest length that meets it, as documented
    assert est.select_n_imp([_curve({64: 0.9, 128: 1.1, 256: 0.5})]) == 64
    assert 'extrapolat' in est.tune_n_imp.__doc__


class _FakeEstimator(object):
    """What n_imp_curve needs of an estimator: sd = c / sqrt(block) at theta = log c."""

    _last_n_imp = 256

    def __init__(self):
        self.calls = []

    def _spread_blocks(self, theta, n_rep, blocks, seed=0, n_imp=None):
        self.calls.append((float(np.atleast_1d(theta)[0]), n_rep, list(blocks), seed, n_imp))
        c = float(np.exp(np.atleast_1d(theta)[0]))
        return [{'sd': c / np.sqrt(b), 'block': b} for b in blocks]


def test_tune_n_imp_and_n_imp_curve_drive_the_estimator():
    from gpdemo import estimators as est
    fake = _FakeEstimator()
    curve = est.n_imp_curve(fake, np.log(8.0), n_rep=4)
    assert list(curve) == [64, 128, 256] and fake.calls[-1][1:] == (4, [64, 128, 256], 0, 256)
    assert list(est.n_imp_curve(fake, 0.0, n_rep=4, n_imp=192)) == [64, 128, 192]
    assert list(est.n_imp_curve(fake, 0.0, n_rep=4, n_imp=50)) == [50]
    curves, block = est.tune_n_imp(fake, np.log([[4.0], [10.0]]), target_sd=1.0, n_rep=8)
    assert len(curves) == 2 and block == 128  # 10 / sqrt(128) = 0.88 <= 1 < 10 / sqrt(64)
    curves, block = est.tune_n_imp(fake, np.log([[4.0], [20.0]]), target_sd=1.0, n_rep=8)
    assert block is None  # 20 / sqrt(256) = 1.25


def test_header_declares_the_entry_points():
    """Fails without the feature: the header lines are new. apm_version() stays 3."""
    txt = open(os.path.join(REPO, 'include', 'apm.h')).read()
    m = re.search(r'\bint\s+apm_u_eval_diag\s*\(([^)]*)\)', txt)
    assert m and len(m.group(1).split(',')) == 10
    m = re.search(r'\bint\s+apm_is_spread\s*\(([^)]*)\)', txt)
    assert m and len(m.group(1).split(',')) == 13
    assert re.search(r'#define\s+APM_SPREAD_MAX_BLOCKS\s+4096\b', txt)


def test_library_exports_binds_and_refuses_null_contexts():
    from gpdemo import _native
    lib = _native.load_library(check_device=False)
    for name in ('apm_u_eval_diag', 'apm_is_spread'):
        assert name in _native.exported_symbols() and hasattr(lib, name)
    assert lib.apm_version() == 3
    assert _native.SPREAD_MAX_BLOCKS == 4096
    one = np.zeros(1, dtype=np.int64)
    key = np.zeros(1, dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    out = np.full(1, 7.0)
    p = out.ctypes.data
    assert lib.apm_u_eval_diag(None, 1, one.ctypes.data, one.ctypes.data, 1, p, p, p, 1,
                               st.ctypes.data) == _native.APM_E_INVALID
    assert lib.apm_is_spread(None, 1, one.ctypes.data, one.ctypes.data, key.ctypes.data,
                             key.ctypes.data, 1, 1, p, p, p, 1,
                             st.ctypes.data) == _native.APM_E_INVALID
    assert out[0] == 7.0


def _bare_context(n_imp=64, max_batch=2):
    """A Context without a device behind it: the argument checks come before any library call
    (lib and the handle are None, so reaching one raises AttributeError instead)."""
    from gpdemo import _native
    ctx = object.__new__(_native.Context)
    ctx.n_imp, ctx.max_batch, ctx.lib, ctx._h = n_imp, max_batch, None, None
    return ctx


def test_argument_errors_come_before_any_device_call():
    from gpdemo import _native
    from gpdemo import estimators as est
    ctx = _bare_context()
    for kw in (dict(block=0), dict(block=65), dict(n_rep=0), dict(n_rep=4097),
               dict(n_rep=65, block=1)):
        a = dict(n_rep=2, block=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.is_spread([0], [0], [1], [0], a['n_rep'], a['block'])
    with pytest.raises(ValueError):
        ctx.is_spread([0, 1, 0], [0, 1, 0], [1] * 3, [0] * 3, 2)  # count > max_batch
    with pytest.raises(ValueError):
        ctx.is_spread([0, 1], [0], [1, 1], [0, 0], 2)             # one U buffer per slot
    with pytest.raises(ValueError):
        ctx.is_spread([0], [0], [1, 2], [0], 2)                   # one seed per chain
    with pytest.raises(ValueError):
        ctx.u_eval_diag([0], [0], block=65)
    with pytest.raises(ValueError):
        ctx.u_eval_diag([], [])
    with pytest.raises(AttributeError):  # valid arguments do reach the (absent) library
        ctx.is_spread([0], [0], [1], [0], 2, 16)
    # the estimators' spread(): n_imp unknown, bad n_rep / block - checked before the context
    e = object.__new__(est.LogMarginalLikelihoodPriorMCEstimator)
    with pytest.raises(ValueError):
        e.spread(np.zeros(3))
    for kw in (dict(n_rep=0), dict(block=0), dict(block=65), dict(n_rep=100, block=1)):
        with pytest.raises(ValueError):
            e.spread(np.zeros(3), n_imp=64, **kw)
    with pytest.raises(ValueError):
        est.n_imp_curve(e, np.zeros(3), n_rep=0, n_imp=64)
    assert not hasattr(est.LogMarginalLikelihoodLaplaceEstimator, 'spread')
    assert hasattr(est.LogMarginalLikelihoodApproxPosteriorISEstimator, 'spread')
    # the batched samplers refuse the Laplace estimator and bad arguments alike
    from auxpm import batched
    s = object.__new__(batched.BatchedAPMEllSSPlusMHSampler)
    s.est, s.n_imp = _native.EST_LAPLACE, 64
    with pytest.raises(ValueError):
        s.estimate_spread()
    s.est = _native.EST_IS
    for kw in (dict(n_rep=0), dict(block=0), dict(block=65)):
        with pytest.raises(ValueError):
            s.estimate_spread(**kw)
