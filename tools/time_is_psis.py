"""Device time of the Pareto-smoothed leave-one-out densities (apm_is_loo_psis) beside
the cached u-call it contains and beside apm_is_loo: HIP events on the context's stream
(apm_stream) around each call, the median of `reps` runs after a cold one. A tail's time is the
difference of its call's median and the u-call's (both calls run exactly the u-call first). The
PSIS tail stores and sorts N S log ratios per chain where apm_is_loo's reduces them in registers.
Development tool; no threshold is attached."""
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
ap.add_argument('--batch', type=int, default=8, help='slots per call')
ap.add_argument('--theta-batch', type=int, default=8, help='thetas per theta-call that fills them')
ap.add_argument('--n-imp', type=int, default=256)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--theta0', type=float, default=0.0, help='log signal variance of the thetas')
ap.add_argument('--proposal', choices=('laplace', 'ep'), default='laplace')
ap.add_argument('--likelihood', choices=('probit', 'logit'), default='probit')
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


B = a.batch
X, y = utils.synthetic_gp_data(a.n, a.d, 20151009)
ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, a.n_imp, max_batch=B, n_slots=B, n_ubufs=B,
                      likelihood=a.likelihood)
est = _native.EST_IS_EP if a.proposal == 'ep' else _native.EST_IS
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
ctx.u_normal(idx, np.full(B, 20151009, dtype=np.uint64), idx.astype(np.uint64))
for t0 in range(0, B, a.theta_batch):  # the slots' state, written once
    sl = idx[t0:t0 + a.theta_batch]
    assert not ctx.theta_eval(est, th[sl], sl, sl)[1].any()
t = dict(u=[], loo=[], psis=[])
for r in range(a.reps + 1):  # rep 0 is cold (first launches, lazy buffers)
    ms_u, (lf0, st0) = timed(lambda: ctx.u_eval(idx, idx))
    ms_l, out = timed(lambda: ctx.is_loo(idx, idx))
    ms_p, ps = timed(lambda: ctx.is_loo_psis(idx, idx))
    assert not st0.any() and not out[6].any() and not ps[5].any()
    assert np.array_equal(lf0, out[0]) and np.array_equal(lf0, ps[0])
    print('rep {0}: u-call {1:.2f} ms  apm_is_loo {2:.2f} ms  apm_is_loo_psis {3:.2f} ms  (khat '
          'median {4:.2f} max {5:.2f}, above 0.7: {6} of {7}; khat_w {8:.2f} .. {9:.2f}; largest '
          '|loo - loo_psis| {10:.2f})'.format(
              r, ms_u, ms_l, ms_p, np.nanmedian(ps[2]), np.nanmax(ps[2]), int((ps[2] > 0.7).sum()),
              ps[2].size, np.nanmin(ps[3]), np.nanmax(ps[3]), np.abs(out[1] - ps[1]).max()),
          flush=True)
    if r:
        t['u'].append(ms_u)
        t['loo'].append(ms_l)
        t['psis'].append(ms_p)
m = dict((k, float(np.median(v))) for k, v in t.items())
tail, tail_p = m['loo'] - m['u'], m['psis'] - m['u']
print('median of {0}: N {1} D {2} S {3}, {4} slots, {5}/{6}: u-call {7:.2f} ms  apm_is_loo {8:.2f} '
      'ms (tail {9:.2f} ms)  apm_is_loo_psis {10:.2f} ms (tail {11:.2f} ms: {12:.2f} x the u-call, '
      "{13:.2f} x apm_is_loo's tail)".format(a.reps, a.n, a.d, a.n_imp, B, a.proposal,
                                             a.likelihood, m['u'], m['loo'], tail, m['psis'],
                                             tail_p, tail_p / m['u'], tail_p / tail))
