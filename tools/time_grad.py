"""Device time of the Laplace-gradient path (Context.laplace_grad) against the Laplace theta-call
it contains, at a given size: HIP events on the context's stream (apm_stream) around each call,
both at the gradient's tight Newton tolerance.

Reports the ratio gradient / laplace, and the time of k_grad_reduce alone (APM_PROF_GRAD_REDUCE:
an event pair around that one launch) with the bytes it has to read - the lower triangles of R
and K - as a fraction of the 8 TB/s HBM peak that DESIGN.md uses (development tool; no threshold
is attached)."""
import argparse
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))
from gpdemo import _native  # noqa: E402
from gpdemo import utils  # noqa: E402

PEAK_HBM_TBS = 8.0

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=4096)
ap.add_argument('--d', type=int, default=32)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--tol', type=float, default=1e-14, help='Newton tolerance of both calls')
ap.add_argument('--theta0', type=float, default=0.0, help='log signal variance of the thetas')
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


X, y = utils.synthetic_gp_data(a.n, a.d, 20151009)
ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, 1, max_batch=a.batch, n_slots=1, n_ubufs=1)
ctx.set_newton(a.tol, 1000)
th = np.tile(np.r_[a.theta0, np.full(a.d, np.log(np.sqrt(a.d)))], (a.batch, 1))
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


t_lap, t_grad, t_red = [], [], []
red_bytes = 0.0
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    ms_l, (val, st, nops) = timed(lambda: ctx.theta_eval(_native.EST_LAPLACE, th))
    ctx.prof_read(_native.PROF_GRAD_REDUCE, reset=True)
    ctx.prof_enable(1)
    ms_g, (lml, grad, gst, nit) = timed(lambda: ctx.laplace_grad(th))
    ctx.prof_enable(0)
    ms_r, launches, red_bytes = ctx.prof_read(_native.PROF_GRAD_REDUCE, reset=True)
    assert not st.any() and not gst.any() and np.array_equal(nops, nit)
    assert np.array_equal(val, lml) and launches == 1 and np.all(np.isfinite(grad))
    print('rep {0}: laplace {1:.2f} ms  gradient {2:.2f} ms  k_grad_reduce {3:.3f} ms  '
          'iterations {4}'.format(r, ms_l, ms_g, ms_r, sorted(nit.tolist())), flush=True)
    if r:
        t_lap.append(ms_l)
        t_grad.append(ms_g)
        t_red.append(ms_r)
lap, grd, red = (float(np.median(t)) for t in (t_lap, t_grad, t_red))
rate = red_bytes / (red * 1e-3) / 1e12
print('max |grad| per theta: {0}'.format(np.array2string(np.abs(grad).max(1), precision=3)))
print('median of {0}: laplace {1:.2f} ms  gradient {2:.2f} ms  gradient / laplace = {3:.3f}'
      .format(a.reps, lap, grd, grd / lap))
print('k_grad_reduce {0:.3f} ms for {1:.3g} bytes (lower triangles of R and K, {2} chains): '
      '{3:.3f} TB/s = {4:.1f}% of {5} TB/s HBM'
      .format(red, red_bytes, a.batch, rate, 100.0 * rate / PEAK_HBM_TBS, PEAK_HBM_TBS))
