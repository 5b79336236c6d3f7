"""The cached per-theta state (apm_slot_read: factor, f_post, g, cst) and the u-path's sample
edges at the panel and tile boundaries of the factorisations, against the fp64 oracle.

The full-size tests compare estimates; an estimate is a log-mean over samples of a sum over rows,
so one wrong tile of the factor, a wrong cst or one dropped sample column moves it by less than
its 5e-4 nats tolerance. Here every lower entry of the slot's factor, its g row and cst are
compared with the oracle at the block counts nb = ceil(N / 64) where the code takes another path
(host_chol64.cpp, host_newton.cpp, host_theta.cpp: one 8-block outer panel, the first trailing block, the first partial-Gram copy, the
first far update, the explicit-inverse panel, odd super-tile counts), and the sample loop of
k_ugemm / k_ugemm64 / k_lme is pinned with probe columns at its block edges (ugemm.hip).

Tolerances are the suite's own: 5e-4 nats for estimates, 1e-8 max|f_post|
for the mode, 1e-5 max|C_chol| for the factor with the fp32 bottom block and 2e-6 for an
fp32-rounded fp64 factor, 2e-6 for the fp32 g row, 1e-8 for cst (a Laplace-LML-like scalar).
"""
import numpy as np
import pytest

import apm_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 5e-4  # nats
D = 5
T0S = (0.0, 2.0)
# nb = 1, 1, 1, 1, 2, 3, 8, 9, 10, 16, 17, 18, 25
SIZES = (1, 2, 63, 64, 65, 129, 512, 513, 577, 1024, 1025, 1089, 1537)
KF = orc.make_kernel_func('ard', 1e-8)


@pytest.fixture(scope='module')
def nat(gpu_available):
    from gpdemo import _native
    _native.load_library()
    return _native


# ----------------------------------------------------------------------------- inputs, oracle

_DATA, _STATE, _REF = {}, {}, {}


def _thetas():
    return np.array([np.r_[t0, np.full(D, 0.5 * np.log(D))] for t0 in T0S])


def _data(n):
    if n not in _DATA:
        if n >= 63:
            from gpdemo import utils
            X, y = utils.synthetic_gp_data(n, D, 7000 + n, 'ard')
        else:  # (synthetic_gp_data normalises by the spread of the rows: zero at n = 1)
            X = np.random.RandomState(7000 + n).normal(size=(n, D))
            y = np.where(np.arange(n) % 2 == 0, 1., -1.)
        _DATA[n] = (X, y)
    return _DATA[n]


def _draws(n, s=8):
    rng = np.random.RandomState(n)
    return rng.normal(size=(n, s)), rng.normal(size=(n, s))


def _state(n, ti):
    """The fp64 slot state of (n, T0S[ti]): the oracle's push-through factor, z and cst."""
    if (n, ti) not in _STATE:
        X, y = _data(n)
        K = np.empty((n, n))
        KF(K, X, _thetas()[ti])
        st = orc.theta_state_pushthrough(K, y)
        st['K'] = K
        st['z'] = st['a'] + st['W'] * st['f_post']
        st['cst'] = 0.5 * st['f_post'].dot(st['z']) - 0.5 * st['logdet_B']
        _STATE[(n, ti)] = st
    return _STATE[(n, ti)]


def _ref(n, ti):
    """The reference's own cache tuple at (n, T0S[ti]), its cubic-op count, and lw_0, the
    log-weight of a zero column (an estimate from one sample is that sample's log-weight)."""
    if (n, ti) not in _REF:
        X, y = _data(n)
        lw0, rc, ops = orc.is_estimate(X, y, KF, np.zeros((n, 1)), _thetas()[ti])
        _REF[(n, ti)] = (rc, ops, lw0)
    return _REF[(n, ti)]


def _ctx(nat, monkeypatch, n, s, n_slots=4, n_ubufs=2, **env):
    X, y = _data(n)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = nat.Context(X, y, nat.KERNEL_ARD, 1e-8, s, max_batch=2, n_slots=n_slots,
                      n_ubufs=n_ubufs)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


def _is_call(nat, ctx, ubuf=0):
    out, st, nops = ctx.theta_eval(nat.EST_IS, _thetas(), [ubuf, ubuf], [0, 1])
    assert (st == 0).all(), st
    return out, nops


# ----------------------------------------------------------------------------- A. slot state

def _rel(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize('n', SIZES)
def test_slot_state_vs_oracle(nat, monkeypatch, n):
    """(L, f_post, g, cst) of an IS theta-call against theta_state_pushthrough, every lower entry
    of L. Measured on MI355X over these sizes (maxima): see the table there."""
    ns1, _ = _draws(n)
    ctx = _ctx(nat, monkeypatch, n, 8)
    ctx.u_upload(0, ns1)
    _, nops = _is_call(nat, ctx)
    for ti in range(2):
        st = _state(n, ti)
        L, f, g, cst = ctx.slot_read(ti)
        dl, dg, dc = _rel(L, np.tril(st['C_chol'])), _rel(g, st['g']), abs(cst - st['cst'])
        df = _rel(f, st['f_post'])
        cst_bound = (1e-8 * np.abs(st['f_post']).max() * np.abs(st['z']).sum() +
                     1e-8 * max(1., abs(st['cst'])))
        print('n = {0} t0 = {1}: |d cst| = {2:.3e} (bound {3:.3e}), max|dL|/max|L| = {4:.3e}, '
              'max|dg|/max|g| = {5:.3e}, max|df|/max|f| = {6:.3e}'
              .format(n, T0S[ti], dc, cst_bound, dl, dg, df))
        assert nops[ti] == st['n_ops'] + 2 == _ref(n, ti)[1]
        assert df <= 1e-8
        assert dl <= 1e-5
        assert dg <= 2e-6
        assert dc <= cst_bound, (dc, cst_bound)
    # PriorMC into two more slots: the estimate, and chol(K) by its backward residual (cond(K)
    # reaches ~1e10 here: an entrywise bound would measure the conditioning, not the kernel)
    X, y = _data(n)
    pm, stp, pops = ctx.theta_eval(nat.EST_PRIORMC, _thetas(), [0, 0], [2, 3])
    assert (stp == 0).all() and (pops == 1).all()
    for ti in range(2):
        st = _state(n, ti)
        K, K_chol = st['K'], _ref(n, ti)[0][0]
        r, _, _ = orc.priormc_estimate(X, y, KF, ns1, K_chol=K_chol)
        assert abs(pm[ti] - r) <= TOL, (ti, pm[ti], r)
        L, _, g, cst = ctx.slot_read(2 + ti)
        assert cst == 0.0 and not g.any()
        L32 = K_chol.astype(np.float32).astype(np.float64)
        res, res_ref = (np.abs(F.dot(F.T) - K).max() / np.abs(K).max() for F in (L, L32))
        print('n = {0} t0 = {1}: PriorMC max|L L^T - K|/max|K| = {2:.3e} (fp32-rounded LAPACK '
              'factor {3:.3e})'.format(n, T0S[ti], res, res_ref))
        assert res <= 8 * res_ref, (res, res_ref)
    ctx.close()


@pytest.mark.parametrize('n', SIZES)
def test_slot_cst_fp64_newton_vs_oracle(nat, monkeypatch, n):
    """cst = 1/2 f_post^T z - 1/2 log|B| of the all-fp64 Newton path (APM_MIXED=0) to the
    Laplace LML's bound, 1e-8 max(1, |cst|)."""
    ctx = _ctx(nat, monkeypatch, n, 8, APM_MIXED=0)
    ctx.u_upload(0, _draws(n)[0])
    _is_call(nat, ctx)
    for ti in range(2):
        st = _state(n, ti)
        cst = ctx.slot_read(ti)[3]
        print('n = {0} t0 = {1} APM_MIXED=0: |d cst| = {2:.3e}, cst = {3:.6f}'
              .format(n, T0S[ti], abs(cst - st['cst']), st['cst']))
        assert abs(cst - st['cst']) <= 1e-8 * max(1., abs(st['cst'])), (cst, st['cst'])
    ctx.close()


@pytest.mark.parametrize('n', [129, 513, 1025])
def test_slot_factor_fp64_bottom_vs_oracle(nat, monkeypatch, n):
    """The fp64 bottom block (APM_POST32_Q=0) is an fp64 factor rounded once to fp32: 2e-6."""
    ctx = _ctx(nat, monkeypatch, n, 8, APM_POST32_Q=0)
    ctx.u_upload(0, _draws(n)[0])
    _is_call(nat, ctx)
    for ti in range(2):
        st = _state(n, ti)
        L = ctx.slot_read(ti)[0]
        dl = _rel(L, np.tril(st['C_chol']))
        print('n = {0} t0 = {1} APM_POST32_Q=0: max|dL|/max|L| = {2:.3e}'.format(n, T0S[ti], dl))
        assert dl <= 2e-6
    ctx.close()


# ----------------------------------------------------------------------------- B. estimates

@pytest.mark.parametrize('n', SIZES)
def test_estimates_at_panel_edges_vs_oracle(nat, monkeypatch, n):
    """IS theta-call, cached u-call and the Laplace estimator at the block counts above
    (test_estimators_multi_panel_vs_oracle's checks at nb = 3, 8, 9, 10, 16, 17, 25 and N < 60)."""
    X, y = _data(n)
    ns1, ns2 = _draws(n)
    ctx = _ctx(nat, monkeypatch, n, 8)
    ctx.u_upload(0, ns1)
    ctx.u_upload(1, ns2)
    out, nops = _is_call(nat, ctx)
    out2, st2 = ctx.u_eval([0, 1], [1, 1])
    lml, stl, lops = ctx.theta_eval(nat.EST_LAPLACE, _thetas())
    assert (st2 == 0).all() and (stl == 0).all()
    for ti in range(2):
        rc, rops, _ = _ref(n, ti)
        r1, _, _ = orc.is_estimate(X, y, KF, ns1, None, rc)
        r2, _, _ = orc.is_estimate(X, y, KF, ns2, None, rc)
        rl, rlops = orc.laplace_estimate(X, y, KF, _thetas()[ti])
        assert nops[ti] == rops and lops[ti] == rlops
        assert abs(out[ti] - r1) <= TOL, (ti, out[ti], r1)
        assert abs(out2[ti] - r2) <= TOL, (ti, out2[ti], r2)
        assert abs(lml[ti] - rl) < 1e-7 * max(1., abs(rl)), (ti, lml[ti], rl)
    ctx.close()


# ----------------------------------------------------------------------------- C. sample edges

@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('s', [63, 65, 130, 1030])
@pytest.mark.parametrize('n', [65, 129])
def test_sample_count_edges_vs_oracle(nat, monkeypatch, n, s, wide):
    """Sample counts that are no multiple of 64 (padded sample blocks, sp > S, one and several of
    them) and above 1024 (k_lme's recomputed samples), on k_ugemm and on k_ugemm64 (APM_WIDE_Q=0:
    every slot wide, fp64 factor and U)."""
    X, y = _data(n)
    rng = np.random.RandomState(1000 * n + s)
    ns1, ns2 = rng.normal(size=(n, s)), rng.normal(size=(n, s))
    ctx = _ctx(nat, monkeypatch, n, s, **({'APM_WIDE_Q': 0} if wide else {}))
    ctx.u_upload(0, ns1)
    ctx.u_upload(1, ns2)
    out, _ = _is_call(nat, ctx)
    out2, st2 = ctx.u_eval([0, 1], [1, 1])
    pm, stp, _ = ctx.theta_eval(nat.EST_PRIORMC, _thetas(), [0, 0], [2, 3])
    pm2, stp2 = ctx.u_eval([2, 3], [1, 1])
    ctx.close()
    assert (st2 == 0).all() and (stp == 0).all() and (stp2 == 0).all()
    for ti in range(2):
        rc = _ref(n, ti)[0]
        refs = (orc.is_estimate(X, y, KF, ns1, None, rc)[0],
                orc.is_estimate(X, y, KF, ns2, None, rc)[0],
                orc.priormc_estimate(X, y, KF, ns1, K_chol=rc[0])[0],
                orc.priormc_estimate(X, y, KF, ns2, K_chol=rc[0])[0])
        for v, r in zip((out[ti], out2[ti], pm[ti], pm2[ti]), refs):
            assert abs(v - r) <= TOL, (ti, v, r)


def test_u_normal_odd_total_matches_philox(nat, monkeypatch):
    """N S = 129 x 65 is odd: the last Philox group of 4 is cut after its first normal."""
    n, s = 129, 65
    ctx = _ctx(nat, monkeypatch, n, s)
    ctx.u_normal([0, 1], [123, 2 ** 63 + 12345], [0, 2 ** 33 + 5])
    for b, (seed, ctr) in enumerate(((123, 0), (2 ** 63 + 12345, 2 ** 33 + 5))):
        np.testing.assert_allclose(ctx.u_download(b), orc.u_normal(seed, ctr, n, s), rtol=2e-6,
                                   atol=2e-6)
    ctx.close()


# Probe columns: U is zero except column j. With lw_0 the log-weight of a zero column and
# Delta = lw_j - lw_0, the estimate is lw_0 + log(1 + (e^Delta - 1) / S); a kernel that dropped
# column j, read zeros for it or read another column in its place returns lw_0 (or is further
# off). The column is seed's standard-normal draw times scale, chosen on the CPU so that this
# shift is at least 10 x the tolerance: (seed, scale) per (n, t0), fixed.
PROBE_MIN_SHIFT = 5e-3
PROBE_COLS = {130: (0, 63, 64, 127, 128, 129), 1030: (1023, 1024, 1029)}
PROBE_DRAWS = {  # (n, ti, S) -> (seed, scale) per probe column of PROBE_COLS[S]
    (65, 0, 130): ((650002, 3.0), (656300, 3.0), (656401, 3.0), (653002, 3.0), (653101, 3.0),
                   (653201, 3.0)),
    (65, 0, 1030): ((655300, 3.0), (655400, 3.0), (655901, 3.0)),
    (65, 1, 130): ((650014, 1.0), (656307, 1.0), (656403, 1.0), (653002, 1.0), (653101, 1.0),
                   (653201, 1.0)),
    (65, 1, 1030): ((655311, 2.0), (655412, 1.0), (655905, 2.0)),
    (129, 0, 130): ((1290002, 3.0), (1296301, 3.0), (1296400, 3.0), (1293002, 3.0),
                    (1293102, 3.0), (1293202, 3.0)),
    (129, 0, 1030): ((1295300, 3.0), (1295406, 3.0), (1295903, 3.0)),
    (129, 1, 130): ((1290003, 1.0), (1296300, 1.0), (1296402, 1.0), (1293002, 1.0),
                    (1293104, 1.0), (1293202, 1.0)),
    (129, 1, 1030): ((1295309, 1.0), (1295436, 1.0), (1295910, 2.0)),
}  # Delta = +0.90 .. +11.5 by the oracle: lost-column shifts 1.0e-2 .. 6.6 nats


def _probe_column(n, seed, scale):
    return scale * np.random.RandomState(seed).normal(size=n)


def _probe_oracle(n, ti, s, j, seed, scale):
    """(reference estimate of the probe U, the shift a lost column j would cause)."""
    X, y = _data(n)
    rc, _, lw0 = _ref(n, ti)
    col = _probe_column(n, seed, scale)
    lwj = orc.is_estimate(X, y, KF, col[:, None], None, rc)[0]
    shift = abs(np.log1p(np.expm1(lwj - lw0) / s))
    U = np.zeros((n, s))
    U[:, j] = col
    return orc.is_estimate(X, y, KF, U, None, rc)[0], shift, lwj - lw0


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('s', [130, 1030])
@pytest.mark.parametrize('n', [65, 129])
def test_probe_columns_vs_oracle(nat, monkeypatch, n, s, wide):
    """One probe column per cached u-call at the first and last column of each 64-sample block,
    of the padded last block, and at k_lme's s = 1023 | 1024 edge and its last sample; through
    k_ugemm and through k_ugemm64 (APM_WIDE_Q=0)."""
    ctx = _ctx(nat, monkeypatch, n, s, **({'APM_WIDE_Q': 0} if wide else {}))
    ctx.u_upload(0, np.zeros((n, s)))
    _is_call(nat, ctx)
    for ti in range(2):
        for j, (seed, scale) in zip(PROBE_COLS[s], PROBE_DRAWS[(n, ti, s)]):
            ref, shift, delta = _probe_oracle(n, ti, s, j, seed, scale)
            assert shift >= PROBE_MIN_SHIFT, (n, ti, s, j, shift)  # of the inputs, not the device
            U = np.zeros((n, s))
            U[:, j] = _probe_column(n, seed, scale)
            ctx.u_upload(1, U)
            v, st = ctx.u_eval([ti], [1])
            print('n = {0} t0 = {1} S = {2} wide = {7:d} j = {3}: Delta = {4:+.3f}, lost-column shift {5:.2e}, '
                  'device - oracle = {6:+.2e}'.format(n, T0S[ti], s, j, delta, shift, v[0] - ref,
                                                    wide))
            assert st[0] == 0
            assert abs(v[0] - ref) <= TOL, (n, ti, s, j, v[0], ref)
    ctx.close()


@pytest.mark.parametrize('wide', [False, True])
def test_u_combine_mirror_is_the_fp64_buffer_rounded(nat, monkeypatch, wide):
    """apm_u_combine writes the fp64 buffer and its fp32 mirror (base32, what k_ugemm reads): a
    u-call on the combined buffer is bitwise the u-call on its download uploaded again."""
    n, s = 129, 65
    ctx = _ctx(nat, monkeypatch, n, s, n_ubufs=4, **({'APM_WIDE_Q': 0} if wide else {}))
    ctx.u_normal([0, 1], [7, 8], [0, 0])
    _is_call(nat, ctx)
    ctx.u_combine([2], [0], [1], [np.cos(0.7)], [np.sin(0.7)])
    Uc = ctx.u_download(2)
    A, B = np.cos(0.7) * ctx.u_download(0), np.sin(0.7) * ctx.u_download(1)
    # fp64 buffer: ca a + cb b, where the device may contract into an fma: the two forms differ
    # by at most the roundings of the products and of the two sums, 2^-53 (3 |A| + 4 |B|)
    assert (np.abs(Uc - (A + B)) <= 2.0 ** -51 * (np.abs(A) + np.abs(B))).all()
    ctx.u_upload(3, Uc)
    a, sta = ctx.u_eval([0, 1], [2, 2])
    b, stb = ctx.u_eval([0, 1], [3, 3])
    ctx.close()
    assert (sta == 0).all() and (stb == 0).all()
    assert a[0] == b[0] and a[1] == b[1], (a, b)


# ----------------------------------------------------------------------------- D. leading dims

SENTINEL = -7.25e77


def _padded(a, ld):
    """(buffer of shape (rows, ld) filled with the sentinel, a copied into its leading columns)"""
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    buf = np.full((a.shape[0], ld), SENTINEL)
    buf[:, :a.shape[1]] = a
    return buf


def _padding_intact(buf, cols):
    return bool((buf[:, cols:] == SENTINEL).all())


def test_leading_dimensions_through_the_c_abi(nat):
    """Every ld* argument of include/apm.h with a stride other than the row length: results are
    bitwise those of the contiguous calls and the padding of every output is left alone."""
    lib = nat.load_library()
    n, s, P = 65, 5, D + 1
    X, y = _data(n)
    thetas = _thetas()
    U = np.random.RandomState(5).normal(size=(n, s))
    p = lambda a: a.ctypes.data

    def run(ldx, ldt, ldu, ldl):
        Xb, Tb, Ub = _padded(X, ldx), _padded(thetas, ldt), _padded(U, ldu)
        h = lib.apm_create(0, nat.KERNEL_ARD, p(Xb), n, D, ldx, p(y), 1e-8, s, 2, 2, 1)
        assert h
        assert lib.apm_u_upload(h, 0, p(Ub), ldu) == 0
        out, st, nops = np.zeros(2), np.zeros(2, np.int32), np.zeros(2, np.int64)
        ub, sl = np.zeros(2, np.int64), np.arange(2, dtype=np.int64)
        assert lib.apm_theta_eval(h, nat.EST_IS, 2, p(Tb), ldt, p(ub), p(sl), p(out), p(st),
                                  p(nops)) == 0
        assert (st == 0).all()
        Ud = np.full((n, ldu), SENTINEL)
        assert lib.apm_u_download(h, 0, p(Ud), ldu) == 0
        Lb = np.full((n, ldl), SENTINEL)
        f, g, c = np.zeros(n), np.zeros(n), np.zeros(1)
        assert lib.apm_slot_read(h, 1, p(Lb), ldl, p(f), p(g), p(c)) == 0
        lib.apm_destroy(h)
        for buf, cols in ((Xb, D), (Tb, P), (Ub, s), (Ud, s), (Lb, n)):
            assert _padding_intact(buf, cols)
        return out, Ud[:, :s].copy(), Lb[:, :n].copy(), f, g, c[0]

    ref = run(D, P, s, n)
    got = run(D + 3, P + 2, s + 5, n + 1)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ref[1], U)  # (fp64 buffer: the upload itself)

    def gram(ldx, ldk):
        Xb = _padded(X, ldx)
        Kb = np.full((n, ldk), SENTINEL)
        assert lib.apm_gram(0, nat.KERNEL_ARD, p(Xb), n, D, ldx, p(thetas[1]), P, 1e-8, p(Kb),
                            ldk) == 0
        assert _padding_intact(Kb, n) and _padding_intact(Xb, D)
        return Kb[:, :n].copy()

    K = gram(D, n)
    np.testing.assert_array_equal(gram(D + 3, n + 7), K)
    np.testing.assert_array_equal(K, K.T)

    def laplace(ldk, ldc):
        Kb = _padded(K, ldk)
        Cb = np.full((n, ldc), SENTINEL)
        f, lml = np.zeros(n), np.zeros(1)
        nit, st = np.zeros(1, np.int64), np.zeros(1, np.int32)
        assert lib.apm_laplace(0, p(Kb), n, ldk, p(y), 1, 1, 1e-4, 1000, p(f), p(Cb), ldc, p(lml),
                               p(nit), p(st)) == 0
        assert st[0] == 0 and _padding_intact(Cb, n) and _padding_intact(Kb, n)
        return f, Cb[:, :n].copy(), lml[0], nit[0]

    for a, b in zip(laplace(n + 7, n + 2), laplace(n, n)):
        np.testing.assert_array_equal(a, b)

    def eval_k(ldk):
        Kb = _padded(K, ldk)
        h = lib.apm_create(0, nat.KERNEL_PRECOMPUTED, None, n, 0, 0, p(y), 1e-8, s, 1, 1, 1)
        assert h
        assert lib.apm_u_upload(h, 0, p(U), s) == 0
        out, st, nops = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int64)
        assert lib.apm_theta_eval_K(h, nat.EST_IS, p(Kb), ldk, 0, 0, p(out), p(st), p(nops)) == 0
        Lb = np.zeros((n, n))
        assert lib.apm_slot_read(h, 0, p(Lb), n, None, None, None) == 0
        lib.apm_destroy(h)
        assert st[0] == 0 and _padding_intact(Kb, n)
        return out[0], nops[0], Lb

    for a, b in zip(eval_k(n + 7), eval_k(n)):
        np.testing.assert_array_equal(a, b)
    v = eval_k(n)[0]  # the caller's K is the library's own Gram at thetas[1]
    assert abs(v - ref[0][1]) <= 1e-9 * max(1., abs(v)), (v, ref[0][1])

    # apm_predict: m = 130 test rows in two blocks (np = 128), two chains of a max_batch = 3
    # context into three-row outputs: the third row is padding too
    m = 130
    Xs = np.random.RandomState(6).normal(size=(m, D))

    def predict(ldxs, ldo, with_mean=True):
        Xsb = _padded(Xs, ldxs)
        h = lib.apm_create(0, nat.KERNEL_ARD, p(X), n, D, D, p(y), 1e-8, s, 3, 1, 1)
        assert h
        outs = [np.full((3, ldo), SENTINEL) for _ in range(3)]
        st, nit = np.full(3, -1, np.int32), np.full(3, -1, np.int64)
        assert lib.apm_predict(h, 2, p(thetas), P, p(Xsb), m, ldxs,
                               p(outs[0]) if with_mean else None, p(outs[1]), p(outs[2]), ldo,
                               p(st), p(nit)) == 0
        lib.apm_destroy(h)
        assert list(st) == [0, 0, -1] and nit[2] == -1 and (nit[:2] > 0).all()
        assert _padding_intact(Xsb, D)
        for o in outs:
            assert _padding_intact(o, m) and (o[2] == SENTINEL).all()
        if not with_mean:
            assert (outs[0] == SENTINEL).all()
        return [o[:2, :m].copy() for o in outs] + [nit[:2].copy()]

    pref = predict(D, m)
    assert all(np.isfinite(o).all() for o in pref)
    for a, b in zip(predict(D + 3, m + 4), pref):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(predict(D + 3, m + 4, with_mean=False)[1:], pref[1:]):
        np.testing.assert_array_equal(a, b)

    # apm_gram_cross: ldx is the row stride of both point sets
    def gram_cross(ldx, ldk):
        Xb, Xsb = _padded(X, ldx), _padded(Xs, ldx)
        Kb = np.full((m, ldk), SENTINEL)
        assert lib.apm_gram_cross(0, nat.KERNEL_ARD, p(Xsb), m, p(Xb), n, D, ldx, p(thetas[1]), P,
                                  p(Kb), ldk) == 0
        assert _padding_intact(Kb, n) and _padding_intact(Xb, D) and _padding_intact(Xsb, D)
        return Kb[:, :n].copy()

    Ks = gram_cross(D, n)
    assert np.isfinite(Ks).all() and (Ks > 0.0).all()
    np.testing.assert_array_equal(gram_cross(D + 3, n + 7), Ks)
