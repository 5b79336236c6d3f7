"""Reference failure semantics on the device path (SURVEY.md §5 "Failure detection"):

* Newton non-convergence -> MaximumIterationsExceededError with the reference's message
  (lpa.py:100-102; tests/golden/errors.npz laplace_maxiter_msg);
* chol(K) failing at an extreme theta -> numpy LinAlgError (estimators.py:206, uncaught in the
  reference), at the theta where the reference raised it;
* a failing chain inside a batched theta-call is masked: its status is reported, every other
  chain's value is unchanged (the reference notebook skips a failed chain,
  E-SS+RD-SS.ipynb:213-217), and the batched sampler counts it in `failed`;
* InvalidCovarianceMatrixError (estimators.py:208-215): the reference raises it where its
  explicitly formed C = K - V^T V is numerically indefinite. The estimate's route factors
  M = I + L_K^T W L_K (SPD for any W >= 0); chains whose C is small
  against K also form C the reference's way (host_theta.cpp icm_check) and fail as the reference does,
  after chol(K) has been retried in LAPACK's order where the blocked factorisation rounds K to
  indefinite;
* cross-stream edges (APM_SKEW) and the device-side guard (APM_STATUS_GUARD).
"""
import numpy as np
import pytest

import apm_oracle as orc
import gpdemo.estimators as est
import gpdemo.kernels as krn
import gpdemo.latent_posterior_approximations as lpa
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def test_laplace_max_iters_raises_reference_message(nat):
    e = golden('errors')
    with pytest.raises(lpa.MaximumIterationsExceededError) as ei:
        lpa.laplace_approximation(e['K'], e['y'], max_iters=1)
    assert str(ei.value) == str(e['laplace_maxiter_msg'])
    # the raw C-ABI reports it as a status, not an error code
    f, C, lml, nit, st = nat.laplace(e['K'], e['y'], True, True, 1e-4, 1)
    assert st == nat.STATUS_MAXITER and nit == 1


def test_is_estimator_max_iters_status(nat):
    """apm_set_newton caps the fused Newton loop of a theta-call: the chain's status is
    MAXITER and the estimator raises the reference's exception type."""
    e = golden('errors')
    X, y = e['X'], e['y']
    ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, 2, max_batch=1, n_slots=1, n_ubufs=1)
    ctx.set_newton(1e-4, 1)
    ctx.u_upload(0, np.zeros((X.shape[0], 2)))
    out, st, _ = ctx.theta_eval(nat.EST_IS, np.r_[1., 0., 0., 0.][None], [0], [0])
    assert st[0] == nat.STATUS_MAXITER
    ctx.close()


@pytest.mark.parametrize('mixed', [None, '0'], ids=['mixed-default', 'mixed-0'])
def test_chol_k_failure_raises_linalgerror(nat, monkeypatch, mixed):
    """Under the default mixed-precision Newton path and under the all-fp64 one (APM_MIXED=0)."""
    if mixed is not None:
        monkeypatch.setenv('APM_MIXED', mixed)
    e = golden('errors')
    assert str(e['cholk_raised']) == 'LinAlgError'
    X, y, ns = e['extreme_X'], e['extreme_y'], e['extreme_ns']
    ctx = nat.Context(X, y, nat.KERNEL_ISO, 1e-8, ns.shape[1], max_batch=1, n_slots=1, n_ubufs=1)
    ctx.u_upload(0, ns)
    for kind in (nat.EST_IS, nat.EST_PRIORMC):
        _, st, _ = ctx.theta_eval(kind, e['cholk_theta'][None], [0], [0])
        assert st[0] == nat.STATUS_CHOL_K, (kind, st)
    ctx.close()
    es = est.LogMarginalLikelihoodApproxPosteriorISEstimator(
        X, y, krn.make_kernel_func('iso', 1e-8), lpa.laplace_approximation)
    with pytest.raises(np.linalg.LinAlgError):
        es(ns, e['cholk_theta'])
    pm = est.LogMarginalLikelihoodPriorMCEstimator(X, y, krn.make_kernel_func('iso', 1e-8))
    with pytest.raises(np.linalg.LinAlgError):
        pm(ns, e['cholk_theta'])
    # the estimator is still usable after the failure
    v, _ = es(ns, np.array([0.3, 0.4]))
    r, _, _ = orc.is_estimate(X, y, orc.make_kernel_func('iso', 1e-8), ns, np.array([0.3, 0.4]))
    assert abs(v - r) <= 5e-4


def test_failing_chain_masked_in_batch(nat):
    e = golden('errors')
    X, y, ns = e['extreme_X'], e['extreme_y'], e['extreme_ns']
    good = [np.array([0.3, 0.4]), np.array([1.0, 0.2]), np.array([-0.5, 0.9])]
    th = np.stack([good[0], e['cholk_theta'], good[1], good[2]])
    ctx = nat.Context(X, y, nat.KERNEL_ISO, 1e-8, ns.shape[1], max_batch=4, n_slots=8, n_ubufs=1)
    ctx.u_upload(0, ns)
    out, st, _ = ctx.theta_eval(nat.EST_IS, th, [0] * 4, [0, 1, 2, 3])
    assert st[1] == nat.STATUS_CHOL_K
    assert (st[[0, 2, 3]] == 0).all()
    for b, t in zip((0, 2, 3), good):
        o, s, _ = ctx.theta_eval(nat.EST_IS, t[None], [0], [4])
        assert s[0] == 0
        assert abs(o[0] - out[b]) <= 1e-9 * max(1., abs(out[b])), (b, o[0], out[b])
    # the batched sampler masks the failed chain and advances the others (auxpm/batched.py)
    from auxpm.batched import BatchedAPMEllSSPlusRandDirSliceSampler
    smp = BatchedAPMEllSSPlusRandDirSliceSampler(
        X, y, 4, ns.shape[1], dict(a_tau=1., b_tau=1. / 3 ** 0.5, a_sigma=1.1, b_sigma=0.1),
        kernel='iso', seed=3)
    smp.initialise(th)
    assert smp.failed.tolist() == [False, True, False, False]
    assert smp.fail_status[1] == nat.STATUS_CHOL_K
    traces, done = smp.run_async(3)
    assert done[1] == 0 and (done[[0, 2, 3]] >= 3).all()
    ctx.close()


@pytest.mark.parametrize('name', ['icm_a', 'icm_b'])
def test_invalid_covariance_raises_where_the_reference_raises(nat, name):
    """At both thetas where the reference raises InvalidCovarianceMatrixError
    (estimators.py:208-215; tests/golden/errors.npz) the device raises it too. K's definiteness
    is decided by rounding there: the device's blocked chol(K) fails, so the chain's K is
    factored again in LAPACK's dpotf2 order (chol.hip k_chol_unblocked: the order of the
    reference's own LinAlgError check, estimators.py:206), which passes as the reference's does;
    then, C being small against K, the library forms C the reference's way (C = K - V^T V from
    the last Newton iteration's fp64 B factor, host_theta.cpp icm_check), whose Cholesky fails as the
    reference's does (a property of the route: it fails under 1-ulp perturbations of B as well,
    profiles/r05_icm_route_study.txt), and the chain reports APM_STATUS_CHOL_C."""
    e = golden('errors')
    assert str(e[name + '_raised']) == 'InvalidCovarianceMatrixError'
    X, y, ns = e['extreme_X'], e['extreme_y'], e['extreme_ns']
    th = e[name + '_theta']
    es = est.LogMarginalLikelihoodApproxPosteriorISEstimator(
        X, y, krn.make_kernel_func('iso', 1e-8), lpa.laplace_approximation)
    with pytest.raises(est.InvalidCovarianceMatrixError):
        es(ns, th)


@pytest.mark.parametrize('name', ['icm_a', 'icm_b'])
def test_invalid_covariance_from_the_references_K(nat, name):
    """The same thetas with the reference's own K uploaded (its Cython Gram's output,
    tests/golden/icm_k.npz from make_golden_icm.py; any kernel callable other than
    make_kernel_func's takes the host-K path, apm_theta_eval_K): on that exact K the reference's
    chol(K) passes and its chol(C) fails, and so do the device's (the dpotf2-order retry of
    chol(K), then the reference-route check)."""
    e = golden('errors')
    Kref = golden('icm_k')[name + '_K']
    X, y, ns = e['extreme_X'], e['extreme_y'], e['extreme_ns']

    def ref_k(K, X_, theta):
        K[...] = Kref

    es = est.LogMarginalLikelihoodApproxPosteriorISEstimator(X, y, ref_k,
                                                             lpa.laplace_approximation)
    with pytest.raises(est.InvalidCovarianceMatrixError):
        es(ns, e[name + '_theta'])


@pytest.mark.parametrize('name', ['icm_a', 'icm_b'])
def test_invalid_covariance_check_off_is_pushthrough(nat, monkeypatch, name):
    """APM_ICM_Q=0 (no reference-route check): the device either fails chol(K) as above or
    returns the push-through estimate, pinned to the oracle's fp64 statement of that route."""
    e = golden('errors')
    X, y, ns = e['extreme_X'], e['extreme_y'], e['extreme_ns']
    th = e[name + '_theta']
    K = np.empty((X.shape[0],) * 2)
    orc.make_kernel_func('iso', 1e-8)(K, X, th)
    monkeypatch.setenv('APM_ICM_Q', '0')
    es = est.LogMarginalLikelihoodApproxPosteriorISEstimator(
        X, y, krn.make_kernel_func('iso', 1e-8), lpa.laplace_approximation)
    try:
        v, cache = es(ns, th)
    except np.linalg.LinAlgError as err:
        assert 'Cholesky of K' in str(err)
        return
    st = orc.theta_state_pushthrough(K, y)
    r = orc.is_estimate_reformulated(y, st, ns)
    assert np.isfinite(v)
    assert abs(v - r) <= 5e-4, (v, r)


def test_forced_spin_timeouts_never_return_wrong_values(nat, monkeypatch):
    """The Newton solve's in-launch hand-overs (the dataflow panel k_chol_panel_df32, the
    multi-workgroup TRSV k_trsv32_mw) wait with bounded spins (SpinCtl, apm_internal.h). With the
    bound forced to one poll (APM_SPIN_LIMIT=1, read at context creation) the waits time out:
    every exit must be counted and must fail its chain, which the Newton loop reruns in fp64 -
    so each chain comes back with status 0 and the value of an undisturbed context (within the
    5e-4-nat estimator tolerance, n_cubic_ops equal), or reports a failure; never a wrong value
    with status 0 (round-4 verdict: an intermittent 2-rank parity failure)."""
    from gpdemo.utils import synthetic_gp_data
    n, d, s, B = 700, 8, 32, 6
    X, y = synthetic_gp_data(n, d, 11)
    base = np.log(np.sqrt(d))
    th = np.stack([np.r_[0.3 * k - 0.6, np.full(d, base + 0.2 * (k % 3))] for k in range(B)])
    rng = np.random.RandomState(4)
    U1, U2 = rng.normal(size=(n, s)), rng.normal(size=(n, s))

    def run():
        ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, s, max_batch=B, n_slots=B, n_ubufs=2)
        try:
            for k in range(nat.PROF_NKINDS):
                ctx.prof_read(k, reset=True)
            ctx.u_upload(0, U1)
            ctx.u_upload(1, U2)
            v1, st1, nops = ctx.theta_eval(nat.EST_IS, th, [0] * B, list(range(B)))
            v2, st2 = ctx.u_eval(list(range(B)), [1] * B)
            ctr = [ctx.prof_read(k)[1] for k in (nat.PROF_STATS, nat.PROF_DF_TIMEOUTS,
                                                 nat.PROF_TRSV_TIMEOUTS)]
        finally:
            ctx.close()
        return v1, v2, st1, st2, nops, ctr

    r1, r2, rs1, rs2, rops, rctr = run()
    assert (rs1 == 0).all() and (rs2 == 0).all()
    assert rctr[1] == 0 and rctr[2] == 0  # an undisturbed context: no spin exits
    monkeypatch.setenv('APM_SPIN_LIMIT', '1')
    v1, v2, st1, st2, nops, ctr = run()
    reruns, df_to, trsv_to = ctr
    assert df_to + trsv_to > 0, 'the forced bound produced no timeout: the path was not exercised'
    assert reruns > 0  # every timed-out chain went to the fp64 rerun
    ok = (st1 == 0) & (st2 == 0)
    # a chain either failed visibly or carries the undisturbed value
    assert ok.all(), (st1, st2)  # (the fp64 rerun has no spin-waits, so none should fail)
    np.testing.assert_array_equal(nops[ok], rops[ok])
    assert np.abs(v1[ok] - r1[ok]).max() <= 5e-4, (v1, r1)
    assert np.abs(v2[ok] - r2[ok]).max() <= 5e-4, (v2, r2)


# ------------------------------------------------------------------ cross-stream edges and the guard
def _stationary_calls(nat, monkeypatch, shifts=(0, 7), B=64, **env):
    """configs[2] (N=4096 D=32 N_imp=256) at the long-chain record's 64 stationary chain states
    (tests/golden/stationary_thetas.npy: the bench's headline regime, 7-8 Newton iterations).
    Each call evaluates the same 64 (theta, u) pairs with pair k at chain position
    (k + shift) mod B (its slot, workspace rows and U buffer with it), so a read of state a
    previous call left behind changes a value. Returns per call, indexed by pair: theta-call and
    u-call values, statuses, n_cubic_ops, the guard's residuals."""
    import os
    from gpdemo.utils import synthetic_gp_data
    X, y = synthetic_gp_data(4096, 32, 20151009)
    th = np.load(os.path.join(os.path.dirname(__file__), 'golden',
                              'stationary_thetas.npy'))[:B].astype(np.float64)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, 256, max_batch=B, n_slots=B, n_ubufs=B)
    for k in env:
        monkeypatch.delenv(k)
    res = []
    try:
        idx = np.arange(B)
        ctx.u_normal(idx, np.full(B, 7), idx)
        for sh in shifts:
            order = np.argsort((idx + sh) % B)  # the pair at each chain position
            out, st, nops = ctx.theta_eval(nat.EST_IS, th[order], order, idx)
            out2, st2 = ctx.u_eval(idx, order)
            g = ctx.guard_read(B)
            r = {k: np.empty_like(v) for k, v in (('v1', out), ('v2', out2), ('st', st),
                                                 ('st2', st2), ('nops', nops), ('g', g))}
            for k, v in (('v1', out), ('v2', out2), ('st', st), ('st2', st2), ('nops', nops),
                         ('g', g)):
                r[k][order] = v
            res.append(r)
    finally:
        ctx.close()
    return res


def test_stream_skew_is_bitwise_neutral(nat, monkeypatch):
    """Every cross-stream edge of a theta-call is an event of its own (apm_host.h Edges: Gram ->
    chol(K), chol(K) -> posterior, L_K J -> fp32 bottom block, each panel of L' -> its bottom
    panel, bottom -> slot writer, each Newton panel -> its far update and back). APM_SKEW puts a
    delay kernel in front of every launch on the secondary streams (1: 1 ms each), on the main
    stream (2: 40 us each) or both (3): whichever side of an edge is held back, a missing or
    misplaced wait would then read stale or unfinished data. Results must be bitwise those of the
    undelayed context, in two calls with the (theta, u) pairs moved to other chain positions
    between them (a stale read of the previous call's state would change a value). APM_SKEW=5
    drops the one wait of the bottom -> slot-writer edge with the secondary streams delayed: the
    slot writer then reads an unfinished fp32 bottom block, and the guard (k_guard_check: C_chol's
    log-diagonal against 1/2 log|K| - 1/2 log|M|, every row of C_chol g against f_post) must
    fail every chain whose value it moves beyond the estimator tolerance (5e-4 nats): no chain
    may come back with status 0 and a value outside it (measured: DESIGN.md §11)."""
    base = _stationary_calls(nat, monkeypatch)
    for r in base:
        assert (r['st'] == 0).all() and (r['st2'] == 0).all()
    for k in ('v1', 'v2', 'nops'):  # the pairs' values do not depend on their chain positions
        np.testing.assert_array_equal(base[1][k], base[0][k])
    for mode in (1, 2, 3):
        res = _stationary_calls(nat, monkeypatch, APM_SKEW=mode)
        for c, (r, b) in enumerate(zip(res, base)):
            for k in ('v1', 'v2', 'st', 'st2', 'nops'):
                np.testing.assert_array_equal(r[k], b[k], err_msg='APM_SKEW={0} call {1} {2}'
                                              .format(mode, c, k))
    sab = _stationary_calls(nat, monkeypatch, shifts=(0,), APM_SKEW=5)[0]
    caught = sab['st'] == nat.STATUS_GUARD
    moved = (sab['v1'] != base[0]['v1']) | (sab['v2'] != base[0]['v2'])
    dv = np.maximum(np.abs(sab['v1'] - base[0]['v1']), np.abs(sab['v2'] - base[0]['v2']))
    print('dropped bottom_done wait: {0} of {1} chains failed by the guard (r3 up to {2:.3e}, r4 '
          'up to {3:.3e}); {4} returned with status 0 and a changed value, |d log f| up to {5:.3e} '
          '(their r4 up to {6:.3e})'.format(
              int(caught.sum()), len(caught), float(np.nanmax(sab['g'][caught, 2], initial=0)),
              float(np.nanmax(sab['g'][caught, 3], initial=0)), int((moved & ~caught).sum()),
              float(dv[~caught].max(initial=0)), float(sab['g'][moved & ~caught, 3].max(initial=0))))
    assert caught.any(), 'the dropped wait was not exercised (no chain read an unfinished block)'
    # never a value outside the estimator tolerance returned with status 0
    assert (dv[~caught] <= 5e-4).all(), np.flatnonzero((dv > 5e-4) & ~caught)


def test_guard_residuals_are_rounding_sized(nat, monkeypatch):
    """The guard's residuals (k_guard_check) stay far below its bounds (GUARD_T1..T4 = 1 nat,
    1e-6 relative, 0.05 nats, 1e-4 relative) where nothing is corrupted: at the bench's stationary states, at
    configs[2]'s four fixture thetas (sigma = e^18.5 included: its posterior bottom block is
    recomputed in fp64, r3 skipped) and on the small mixed-precision cases; printed for
    DESIGN.md §11."""
    from gpdemo.utils import synthetic_gp_data
    worst = np.zeros(4)
    r = _stationary_calls(nat, monkeypatch, shifts=(0,))[0]
    assert (r['st'] == 0).all()
    worst = np.maximum(worst, r['g'].max(axis=0))
    print('stationary (64 chains) max r1 r2 r3 r4:', r['g'].max(axis=0))
    z = golden('config2_ref')
    X, y = synthetic_gp_data(int(z['n']), int(z['d']), int(z['data_seed']))
    th = z['thetas'].astype(np.float64)
    B = th.shape[0]
    U = np.random.RandomState(int(z['u_seed'])).normal(size=(int(z['n']), int(z['s'])))
    ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, int(z['s']), max_batch=B, n_slots=B, n_ubufs=1)
    try:
        ctx.u_upload(0, U)
        out, st, _ = ctx.theta_eval(nat.EST_IS, th, [0] * B, list(range(B)))
        g = ctx.guard_read(B)
    finally:
        ctx.close()
    assert (st == 0).all()
    print('configs[2] fixture thetas r1 r2 r3 r4:\n', g)
    worst = np.maximum(worst, g.max(axis=0))
    for n in (700, 1100):
        X, y = synthetic_gp_data(n, 5, 4242, 'ard')
        rng = np.random.RandomState(7)
        base = 0.5 * np.log(5)
        th = np.array([np.r_[t0, rng.normal(scale=0.3, size=5) + base]
                       for t0 in (0.0, 2.0, 4.0, 9.0, 14.0)])
        ns = rng.normal(size=(n, 32))
        for env in ({}, {'APM_MIXED': 0}):
            for k, v in env.items():
                monkeypatch.setenv(k, str(v))
            ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, 32, max_batch=5, n_slots=5, n_ubufs=1)
            for k in env:
                monkeypatch.delenv(k)
            try:
                ctx.u_upload(0, ns)
                out, st, _ = ctx.theta_eval(nat.EST_IS, th, [0] * 5, list(range(5)))
                g = ctx.guard_read(5)
            finally:
                ctx.close()
            assert (st == 0).all(), (n, env, st)
            print('n = {0} {1} r1 r2 r3 r4:\n'.format(n, env), g)
            worst = np.maximum(worst, g.max(axis=0))
    print('worst r1 r2 r3 r4:', worst)
    assert worst[0] <= 1.0 / 20 and worst[1] <= 1e-6 / 20 and worst[2] <= 0.05 / 20, worst
    assert worst[3] <= 1e-4 / 20, worst


def test_chol_k_pacing_is_bitwise_neutral(nat):
    """The concurrent chol(K) releases its panels over the Newton iterations the context's
    previous theta-call took (host_newton.cpp newton: cholk_quota), so its schedule depends on what the
    context did before. A sequence of stationary states (7-8 iterations) -> theta* (fewer: panels
    left for the drain before the posterior) -> stationary again (paced from the short call) must
    give, call by call, the bitwise values of a fresh context (no previous call: no pacing)."""
    import os
    from gpdemo.utils import synthetic_gp_data
    B = 16
    X, y = synthetic_gp_data(4096, 32, 20151009)
    st = np.load(os.path.join(os.path.dirname(__file__), 'golden',
                              'stationary_thetas.npy'))[:B].astype(np.float64)
    star = np.zeros_like(st)
    star[:, 1:] = 0.5 * np.log(32.0)
    seq = [st, star, st]
    idx = np.arange(B)

    def run(ctx, th):
        out, status, nops = ctx.theta_eval(nat.EST_IS, th, idx, idx)
        out2, status2 = ctx.u_eval(idx, idx)
        return out.copy(), out2.copy(), status.copy(), status2.copy(), nops.copy()

    def fresh(th):
        ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, 256, max_batch=B, n_slots=B, n_ubufs=B)
        try:
            ctx.u_normal(idx, np.full(B, 11), idx)
            return run(ctx, th)
        finally:
            ctx.close()

    ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, 256, max_batch=B, n_slots=B, n_ubufs=B)
    try:
        ctx.u_normal(idx, np.full(B, 11), idx)
        got = [run(ctx, th) for th in seq]
    finally:
        ctx.close()
    for c, (g, th) in enumerate(zip(got, seq)):
        ref = fresh(th)
        assert (g[2] == 0).all() and (g[3] == 0).all()
        for a, b, name in zip(g, ref, ('theta-call', 'u-call', 'status', 'u status', 'nops')):
            np.testing.assert_array_equal(a, b, err_msg='call {0}: {1}'.format(c, name))
    assert got[1][4].max() < got[0][4].max(), 'theta* should need fewer Newton iterations'
