"""Parity at the BASELINE.json configurations themselves (not only at small N):

* configs[2] — N=4096 D=32 ARD-SE, N_imp=256: one batched theta-call of 4 chains (the bench's
  theta*, a long length-scale, sigma = e^18.5 next to the fp16x3 guard, a prior-like draw) and a
  cached u-call, against the REFERENCE's own outputs on the same (theta, u)
  (tests/golden/config2_ref.npz, made by tests/golden/make_golden_fullsize.py). This is the size the bench runs, with its multi-panel fp16x3 Newton updates, the
  4-workgroup TRSV, the concurrent chol(K) and the single-launch SYRK.
* configs[4] — N=16384 D=64 N_imp=1024: against the REFERENCE's own outputs at full size
  (tests/golden/config4_ref.npz), and the default path against the all-fp32-operand (APM_H3=0)
  and all-fp64 Newton (APM_MIXED=0) paths on the same inputs.
* configs[0] — PM-MH, iso kernel, N=768 D=8, N_imp=1, Laplace-estimator adaptive phase then the
  IS main phase (Pseudo-Marginal MH.ipynb cells 12-14): the reference's own chain
  (tests/golden/pmmh_chain.npz) replayed with the GPU estimators and the API-compatible
  PMMHSampler, call by call.

Tolerance for estimator values: |d log f| <= 5e-4 nats absolute; at a theta
where the reference's own value is not reproducible to that (sigma = e^18.5: it moves by 11 / 25
nats between one and several BLAS threads, recorded in the fixture), twice the reference's own
spread. n_cubic_ops must
be equal and f_post within 1e-8 of its maximum (fp64-refined Newton modes).
"""
import os
import sys

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

TOL_NATS = 5e-4   # |d log f| of every theta-call / u-call, no relative term
FPOST_REL = 1e-8  # max |d f_post| / max |f_post|


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


def _fixture(name, X, y):
    """The reference's own outputs at a BASELINE configuration (tests/golden/
    make_golden_fullsize.py); refuses when this host's data differ from the fixture's."""
    import hashlib
    z = golden(name)
    assert hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest() == str(z['x_sha256']), \
        'X differs from the fixture data (numpy RandomState / normalise_inputs changed?)'
    np.testing.assert_array_equal(z['y'].astype(np.float64), y)
    return z


def _theta_tol(z, b):
    """TOL_NATS, or - where the reference's own estimate moves by more than that between BLAS
    thread counts (the fixture's one-thread values: sigma = e^18.5, cond(K) ~ 1e24, ~11 / 25
    nats) - twice that spread: no fp64 implementation other than the reference's own LAPACK
    call sequence on the same thread count reproduces it more closely."""
    if 'logf1_t1' not in z.files or not np.isfinite(z['logf1_t1'][b]):
        return TOL_NATS
    spread = max(abs(z['logf1'][b] - z['logf1_t1'][b]), abs(z['logf2'][b] - z['logf2_t1'][b]))
    return max(TOL_NATS, 2.0 * spread)


def _vs_reference(nat, X, y, z, s, u_seed, max_batch):
    n = X.shape[0]
    th = z['thetas']
    B = th.shape[0]
    rng = np.random.RandomState(u_seed)
    U1, U2 = rng.normal(size=(n, s)), rng.normal(size=(n, s))
    out, out2, nops, fpost, cld = [], [], [], [], []
    for b0 in range(0, B, max_batch):
        bb = list(range(b0, min(B, b0 + max_batch)))
        ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, s, max_batch=len(bb), n_slots=len(bb),
                          n_ubufs=2)
        ctx.u_upload(0, U1)
        ctx.u_upload(1, U2)
        o, st, nop = ctx.theta_eval(nat.EST_IS, th[bb], [0] * len(bb), list(range(len(bb))))
        o2, st2 = ctx.u_eval(list(range(len(bb))), [1] * len(bb))
        assert (st == 0).all() and (st2 == 0).all(), (st, st2)
        for q in range(len(bb)):
            L, f, _, _ = ctx.slot_read(q)
            fpost.append(f)
            cld.append(np.log(np.diagonal(L)))
        ctx.close()
        out += list(o)
        out2 += list(o2)
        nops += list(nop)
    report = []
    for b in range(B):
        assert int(z['status'][b]) == 0, 'the reference failed at this theta'
        d1, d2 = out[b] - z['logf1'][b], out2[b] - z['logf2'][b]
        report.append((b, d1, d2))
        tol = _theta_tol(z, b)
        assert nops[b] == int(z['n_cubic_ops'][b]), (b, nops[b], z['n_cubic_ops'][b])
        assert abs(d1) <= tol, (b, out[b], z['logf1'][b])
        assert abs(d2) <= tol, (b, out2[b], z['logf2'][b])
        fr = z['f_post'][b]
        np.testing.assert_allclose(fpost[b], fr, rtol=0, atol=FPOST_REL * np.abs(fr).max())
        # C_chol's diagonal (fp32 in the slot): log-diagonal to fp32 resolution
        np.testing.assert_allclose(cld[b], z['c_logdiag'][b], rtol=0, atol=2e-6)
    return report


def test_config2_full_size_vs_reference(nat):
    """configs[2] at full size against the REFERENCE's own outputs (tests/golden/config2_ref.npz:
    the reference estimator run on these inputs in the build container; the oracle equals it
    bit for bit there): 4 thetas in one batched call — the bench's theta*, a long length-scale,
    sigma = e^18.5 next to the fp16x3 guard (|log f| = 2e10), a prior-like draw."""
    from gpdemo.utils import synthetic_gp_data
    z = golden('config2_ref')
    X, y = synthetic_gp_data(int(z['n']), int(z['d']), int(z['data_seed']))
    z = _fixture('config2_ref', X, y)
    rep = _vs_reference(nat, X, y, z, int(z['s']), int(z['u_seed']), 4)
    print('configs[2] vs reference d(theta-call), d(u-call):', rep)


def _stress_data(n, d, seed):
    """tools/stress.py's data (synthetic_gp_data's recipe, distances from one BLAS product)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    'tools'))
    from stress import stress_data
    return stress_data(n, d, seed)


def _run(nat, X, y, th, s, U, monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    B = th.shape[0]
    ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, s, max_batch=B, n_slots=B, n_ubufs=1)
    for k in env:
        monkeypatch.delenv(k)
    ctx.u_upload(0, U)
    out, st, nops = ctx.theta_eval(nat.EST_IS, th, [0] * B, list(range(B)))
    out2, st2 = ctx.u_eval(list(range(B)), [0] * B)
    f = [ctx.slot_read(b)[1] for b in range(B)]
    ctx.close()
    return out, st, nops, out2, f


def test_config4_full_size_vs_reference(nat):
    """configs[4] at full size, N=16384 D=64 N_imp=1024, against the REFERENCE's own outputs
    (tests/golden/config4_ref.npz; the reference's theta-call takes ~15 CPU-minutes each here):
    two thetas in one batched call, theta-call + cached u-call values, n_cubic_ops, f_post and
    C_chol's diagonal."""
    z = golden('config4_ref')
    X, y = _stress_data(int(z['n']), int(z['d']), int(z['data_seed']))
    z = _fixture('config4_ref', X, y)
    rep = _vs_reference(nat, X, y, z, int(z['s']), int(z['u_seed']), 2)
    print('configs[4] vs reference d(theta-call), d(u-call):', rep)


def test_config4_full_size_paths_agree(nat, monkeypatch):
    n, d, s = 16384, 64, 1024
    X, y = _stress_data(n, d, 20151009)
    base = np.log(np.sqrt(d))
    th = np.stack([np.r_[0.0, np.full(d, base)],
                   np.r_[2.0, np.random.RandomState(3).normal(scale=0.2, size=d) + base + 0.5]])
    U = np.random.RandomState(4).normal(size=(n, s))
    ref = _run(nat, X, y, th, s, U, monkeypatch)
    assert (ref[1] == 0).all() and np.isfinite(ref[0]).all() and np.isfinite(ref[3]).all()
    for env in (dict(APM_H3=0), dict(APM_MIXED=0)):
        o, st, nops, o2, f = _run(nat, X, y, th, s, U, monkeypatch, **env)
        assert (st == 0).all(), env
        np.testing.assert_array_equal(nops, ref[2])
        for b in range(th.shape[0]):
            assert abs(o[b] - ref[0][b]) <= 1e-5 * max(1., abs(ref[0][b])), (env, b)
            assert abs(o2[b] - ref[3][b]) <= 1e-5 * max(1., abs(ref[3][b])), (env, b)
            # the Newton modes of the three paths agree to the refinement's acceptance level
            # (measured 7e-9 of max|f| at N=16384; 1e-9 at N <= 8192)
            np.testing.assert_allclose(f[b], ref[4][b], rtol=1e-9,
                                       atol=2e-8 * np.abs(ref[4][b]).max())


def test_config2_stationary_states_match_fp64_newton(nat, monkeypatch):
    """The regime the bench's headline is timed in: configs[2] (N=4096 D=32 N_imp=256) at 8 of
    the long-chain record's stationary chain states (tests/golden/stationary_thetas.npy, a copy
    of profiles/r04_stationary_thetas.npy: log sigma 3.1-4.3, 7-8 Newton iterations, two
    refinement rounds per iteration), the default mixed-precision path (fp16x3 explicit-inverse
    panels, fp32 posterior bottom block) against the all-fp64 Newton iteration (APM_MIXED=0) on
    the same (theta, u): estimates within TOL_NATS, n_cubic_ops equal, f_post within FPOST_REL
    (measured 5.5e-11 over 16 chains, profiles/r05_refine_tol_study.txt)."""
    from gpdemo.utils import synthetic_gp_data
    X, y = synthetic_gp_data(4096, 32, 20151009)
    th = np.load(os.path.join(os.path.dirname(__file__), 'golden',
                              'stationary_thetas.npy'))[::8].astype(np.float64)
    U = np.random.RandomState(5).normal(size=(4096, 256))
    ref = _run(nat, X, y, th, 256, U, monkeypatch, APM_MIXED=0)
    o, st, nops, o2, f = _run(nat, X, y, th, 256, U, monkeypatch)
    assert (ref[1] == 0).all() and (st == 0).all()
    np.testing.assert_array_equal(nops, ref[2])
    for b in range(th.shape[0]):
        assert abs(o[b] - ref[0][b]) <= TOL_NATS, b
        assert abs(o2[b] - ref[3][b]) <= TOL_NATS, b
        assert np.abs(f[b] - ref[4][b]).max() <= FPOST_REL * np.abs(ref[4][b]).max(), b


def test_config2_reference_route_check_passes_everywhere(nat, monkeypatch):
    """The reference-route check of chol(C) (host_theta.cpp icm_check) forced on
    every chain (APM_ICM_Q=1: trace(C) < n K_ii holds for every chain, C being below K) at
    configs[2]'s four thetas, sigma = e^18.5 included: C = K - V^T V of the last Newton
    iteration factors on every chain (status 0, as in the reference, which returned values
    there), the check ran on all of them (APM_PROF_ICM_CHECKS), and the estimates are bitwise
    those of the default call (the check writes nothing the estimate reads)."""
    from gpdemo.utils import synthetic_gp_data
    z = golden('config2_ref')
    X, y = synthetic_gp_data(int(z['n']), int(z['d']), int(z['data_seed']))
    th = z['thetas'][:4].astype(np.float64)
    U = np.random.RandomState(int(z['u_seed'])).normal(size=(int(z['n']), int(z['s'])))
    ref = _run(nat, X, y, th, int(z['s']), U, monkeypatch)
    monkeypatch.setenv('APM_ICM_Q', '1')
    B = th.shape[0]
    ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, int(z['s']), max_batch=B, n_slots=B, n_ubufs=1)
    monkeypatch.delenv('APM_ICM_Q')
    try:
        ctx.u_upload(0, U)
        o, st, nops = ctx.theta_eval(nat.EST_IS, th, [0] * B, list(range(B)))
        checked = ctx.prof_read(nat.PROF_ICM_CHECKS)[1]
        o2, st2 = ctx.u_eval(list(range(B)), [0] * B)
    finally:
        ctx.close()
    assert checked == B, checked
    assert (ref[1] == 0).all() and (st == 0).all() and (st2 == 0).all()
    np.testing.assert_array_equal(o, ref[0])
    np.testing.assert_array_equal(o2, ref[3])
    np.testing.assert_array_equal(nops, ref[2])


def test_config0_pmmh_chain_matches_reference(nat):
    import auxpm.samplers as smp
    import gpdemo.estimators as est
    import gpdemo.kernels as krn
    import gpdemo.latent_posterior_approximations as lpa
    import gpdemo.utils as utils
    g = golden('pmmh_chain')
    X, y = g['X'], g['y']
    d = X.shape[1]
    prior = dict(a_tau=1., b_tau=1. / d ** 0.5, a_sigma=1.1, b_sigma=0.1)
    kf = krn.make_kernel_func('iso', 1e-8)
    prng = np.random.RandomState()
    det = est.LogMarginalLikelihoodLaplaceEstimator(X, y, kf)
    imp = est.LogMarginalLikelihoodApproxPosteriorISEstimator(X, y, kf, lpa.laplace_approximation)
    calls = []

    def lp(theta):
        return (utils.log_gamma_log_pdf(theta[0], prior['a_sigma'], prior['b_sigma']) +
                utils.log_gamma_log_pdf(theta[1], prior['a_tau'], prior['b_tau']))

    def log_f_adapt(theta):
        v = det(theta)
        calls.append(v)
        return v + lp(theta)

    def log_f_main(theta):
        v = imp(prng.normal(size=(y.shape[0], 1)), theta)[0]
        calls.append(v)
        return v + lp(theta)

    def prop_sampler(theta, sc):
        return np.r_[theta[0] + sc[0] * prng.normal(), theta[1] + sc[1] * prng.normal()]

    def log_prop_density(tp, tc, sc):
        return -0.5 * (((tp[0] - tc[0]) / sc[0]) ** 2 + ((tp[1] - tc[1]) / sc[1]) ** 2)

    sampler = smp.PMMHSampler(log_f_adapt, log_prop_density, prop_sampler, np.array([0.5, 0.5]),
                              prng)
    prng.seed(int(g['seed']))
    theta_init = np.array([np.log(prng.gamma(prior['a_sigma'], 1. / prior['b_sigma'])),
                           np.log(prng.gamma(prior['a_tau'], 1. / prior['b_tau']))])
    np.testing.assert_array_equal(theta_init, g['theta_init'])
    ath, aps, aar = sampler.adaptive_run(theta_init, 10, 3, 0.15, 0.30, utils.adapt_factor_func,
                                         False)
    na = int(g['n_adapt_calls'])
    assert len(calls) == na
    # Laplace phase: fp64 on the device, deterministic
    np.testing.assert_allclose(calls, g['calls'][:na], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(ath, g['adapt_thetas'])
    np.testing.assert_array_equal(aps, g['adapt_scales'])
    np.testing.assert_array_equal(aar, g['adapt_rates'])
    sampler.log_f_estimator = log_f_main
    imp.reset_cubic_op_count()
    thetas, n_reject = sampler.get_samples(ath[-1], g['thetas'].shape[0])
    dv = np.abs(np.array(calls[na:]) - g['calls'][na:])
    assert (dv <= TOL_NATS).all(), dv.max()
    np.testing.assert_array_equal(thetas, g['thetas'])
    assert n_reject == int(g['n_reject'])
    assert imp.n_cubic_ops == int(g['n_cubic_ops'])
