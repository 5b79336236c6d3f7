"""Device time of the importance-sampling predictive (apm_is_predict) beside the IS
theta-call it contains: HIP events on the context's stream (apm_stream) around each call, the
median of `reps` runs after a cold one. The tail's time is the difference of the two medians (the
call runs exactly the theta-call first). Development tool; no threshold is attached."""
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
ap.add_argument('--m', type=int, default=1024)
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
Xs = np.random.RandomState(1).normal(size=(a.m, a.d))
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
t = dict(theta=[], predict=[])
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    ms_t, (lf0, st0, _) = timed(lambda: ctx.theta_eval(est, th, idx, idx))
    ms_p, out = timed(lambda: ctx.is_predict(est, th, idx, idx, Xs))
    assert not st0.any() and not out[5].any() and np.array_equal(lf0, out[0])
    print('rep {0}: theta-call {1:.2f} ms  apm_is_predict {2:.2f} ms  (ess {3:.1f} .. {4:.1f} of '
          '{5})'.format(r, ms_t, ms_p, out[4].min(), out[4].max(), a.n_imp), flush=True)
    if r:
        t['theta'].append(ms_t)
        t['predict'].append(ms_p)
m = dict((k, float(np.median(v))) for k, v in t.items())
print('median of {0}: N {1} D {2} S {3} m {4}, {5} thetas, {6}/{7}: theta-call {8:.2f} ms  '
      'apm_is_predict {9:.2f} ms  tail {10:.2f} ms ({11:.2f} x the theta-call)'.format(
          a.reps, a.n, a.d, a.n_imp, a.m, B, a.proposal, a.likelihood, m['theta'], m['predict'],
          m['predict'] - m['theta'], (m['predict'] - m['theta']) / m['theta']))
