"""Device time of apm_is_spread against the loop it replaces - apm_u_normal +
apm_u_eval per replicate from Python, the same replicates in the same run - at the bench's size:
HIP events on the context's stream (apm_stream) around each, the median of `reps` runs after a
cold one. It also prints n_rep times the difference between one apm_u_eval_diag and one apm_u_eval
as a share of apm_is_spread: an upper bound of k_lme_blocks's share (the difference holds that
kernel and the three read-back copies of a call; a kernel trace of this tool gives the kernel's
own time). apm_is_spread must not be slower than the loop: the tool exits non-zero
if it is.

With --table it also prints, for the first `--table` thetas and both proposals (EST_IS slots and
EST_IS_EP slots), the sd of the log-estimate, the median weight ESS and the delta-method figure
sqrt(mean(1/ESS - 1/N)) at block lengths 64 * 2^k <= n_imp on the same draws. The thetas are the
long-chain record's stationary states (tests/golden/stationary_thetas.npy, every 8th row) unless
--theta0 is given. Development tool."""
import argparse
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))
from gpdemo import _native  # noqa: E402
from gpdemo import utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=4096)
ap.add_argument('--d', type=int, default=32)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--n-imp', type=int, default=256)
ap.add_argument('--n-rep', type=int, default=32)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--theta0', type=float, default=None,
                help='log signal variance of synthetic thetas (default: the stationary states)')
ap.add_argument('--table', type=int, default=4, help='thetas of the sd / ESS table (0: none)')
a = ap.parse_args()

try:
    hip = ctypes.CDLL('libamdhip64.so')
except OSError:
    hip = ctypes.CDLL(os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib',
                                   'libamdhip64.so'))
for name, args in (('hipEventCreate', [ctypes.POINTER(ctypes.c_void_p)]),
                   ('hipEventRecord', [ctypes.c_void_p, ctypes.c_void_p]),
                   ('hipEventSynchronize', [ctypes.c_void_p]),
                   ('hipEventElapsedTime', [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                            ctypes.c_void_p])):
    getattr(hip, name).argtypes = args
    getattr(hip, name).restype = ctypes.c_int


def _ok(rc):
    if rc != 0:
        raise RuntimeError('HIP error {0}'.format(rc))


B, R, S = a.batch, a.n_rep, a.n_imp
X, y = utils.synthetic_gp_data(a.n, a.d, 20151009)
ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, S, max_batch=B, n_slots=2 * B, n_ubufs=2 * B)
if a.theta0 is None:
    th = np.load(os.path.join(REPO, 'tests', 'golden', 'stationary_thetas.npy'))
    th = th[(np.arange(B) * 8) % th.shape[0]].astype(np.float64)
else:
    th = np.tile(np.r_[a.theta0, np.full(a.d, np.log(np.sqrt(a.d)))], (B, 1))
    th += np.random.RandomState(0).normal(scale=0.1, size=th.shape)
ev = [ctypes.c_void_p() for _ in range(2)]
for e in ev:
    _ok(hip.hipEventCreate(ctypes.byref(e)))


def timed(fn):
    _ok(hip.hipEventRecord(ev[0], ctx.stream_ptr))
    out = fn()
    _ok(hip.hipEventRecord(ev[1], ctx.stream_ptr))
    _ok(hip.hipEventSynchronize(ev[1]))
    ms = ctypes.c_float()
    _ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]))
    return float(ms.value), out


idx = np.arange(B)
seeds = np.full(B, 20151009, dtype=np.uint64) + idx.astype(np.uint64)
ctrs = np.full(B, 100, dtype=np.uint64)
sl_is, sl_ep = idx, idx + B
ub, ub2 = idx, idx + B
ctx.u_normal(ub, seeds, np.zeros(B, dtype=np.uint64))
_, st, nops = ctx.theta_eval(_native.EST_IS, th, ub, sl_is)
assert not st.any(), st
print('EST_IS theta-call: Newton iterations {0}'.format(sorted((nops - 3).tolist())), flush=True)


def loop():
    out = np.empty((B, R))
    for r in range(R):
        ctx.u_normal(ub2, seeds, ctrs + np.uint64(r))
        out[:, r], s = ctx.u_eval(sl_is, ub2)
        assert not s.any()
    return out


t = dict(spread=[], loop=[], diag=[], u=[])
for rep in range(a.reps + 1):  # rep 0 is cold (first launches, lazy buffers)
    ms_s, (logf, ess, wmax, s) = timed(lambda: ctx.is_spread(sl_is, ub, seeds, ctrs, R))
    ms_l, ref = timed(loop)
    ms_d, _ = timed(lambda: ctx.u_eval_diag(sl_is, ub2))
    ms_u, _ = timed(lambda: ctx.u_eval(sl_is, ub2))
    assert not s.any() and np.array_equal(logf[:, :, 0], ref)  # the same replicates, bitwise
    print('rep {0}: apm_is_spread {1:.2f} ms  loop {2:.2f} ms  u_eval_diag {3:.3f} ms  u_eval '
          '{4:.3f} ms'.format(rep, ms_s, ms_l, ms_d, ms_u), flush=True)
    if rep:
        for k, v in (('spread', ms_s), ('loop', ms_l), ('diag', ms_d), ('u', ms_u)):
            t[k].append(v)
m = dict((k, float(np.median(v))) for k, v in t.items())
share = max(0.0, R * (m['diag'] - m['u'])) / m['spread']
print('median of {0}: N {1} D {2} S {3}, {4} thetas, {5} replicates: apm_is_spread {6:.2f} ms '
      '({7:.3f} ms per replicate)  loop {8:.2f} ms ({9:.3f} ms per replicate)  ratio {10:.2f}  '
      'k_lme_blocks share < {11:.1%}'.format(a.reps, a.n, a.d, S, B, R, m['spread'],
                                           m['spread'] / R, m['loop'], m['loop'] / R,
                                           m['loop'] / m['spread'], share))

if a.table > 0:
    ctx.u_normal(ub, seeds, np.zeros(B, dtype=np.uint64))
    _, st_e, nops_e = ctx.theta_eval(_native.EST_IS_EP, th, ub, sl_ep)
    assert not st_e.any(), st_e
    print('EST_IS_EP theta-call: sweeps {0}'.format(sorted(((nops_e - 3) // 2).tolist())))
    blocks = [b for b in (64 << k for k in range(20)) if b <= S]
    print('theta_0 | proposal | sd of log p at N = {0} | median weight ESS | sqrt(mean(1/ESS - '
          '1/N))'.format(' / '.join(str(b) for b in blocks)))
    for name, sl in (('Laplace', sl_is), ('EP', sl_ep)):
        res = [ctx.is_spread(sl, ub2, seeds, ctrs, R, b) for b in blocks]
        for c in range(min(a.table, B)):
            sd = [np.std(r[0][c], ddof=1) for r in res]
            med = [np.median(r[1][c]) for r in res]
            dl = [np.sqrt(np.mean(1.0 / r[1][c] - 1.0 / b)) for r, b in zip(res, blocks)]
            print('{0:.2f} | {1} | {2} | {3} | {4}'.format(
                th[c, 0], name, ' / '.join('{0:.3f}'.format(v) for v in sd),
                ' / '.join('{0:.0f}'.format(v) for v in med),
                ' / '.join('{0:.3f}'.format(v) for v in dl)))
ctx.close()
if m['spread'] > m['loop']:
    sys.exit('apm_is_spread ({0:.2f} ms) is slower than the loop ({1:.2f} ms)'.format(
        m['spread'], m['loop']))
