"""Device time of the Laplace predictive path (Context.predict) against the Laplace theta-call it
contains, at a given size: HIP events on the context's stream (apm_stream) around each call.

Reports the ratio (predict - laplace) / laplace and the f64 rate of the predictive solve (N^2 M
flops per theta) against the 78.6 TFLOP/s peak that DESIGN.md uses (development tool)."""
import argparse
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))
from gpdemo import _native  # noqa: E402
from gpdemo import utils  # noqa: E402

PEAK_F64_TFLOPS = 78.6

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=4096)
ap.add_argument('--d', type=int, default=32)
ap.add_argument('--m', type=int, default=4096)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--reps', type=int, default=3)
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
Xs = np.random.RandomState(1).normal(size=(a.m, a.d))  # test inputs from the inputs' law
ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, 1, max_batch=a.batch, n_slots=1, n_ubufs=1)
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


t_lap, t_pred = [], []
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    ms_l, (_, st, nops) = timed(lambda: ctx.theta_eval(_native.EST_LAPLACE, th))
    ms_p, (mean, var, prob, pst, nit) = timed(lambda: ctx.predict(th, Xs))
    assert not st.any() and not pst.any() and np.array_equal(nops, nit)
    print('rep {0}: laplace {1:.2f} ms  predict {2:.2f} ms  iterations {3}'
          .format(r, ms_l, ms_p, sorted(nit.tolist())), flush=True)
    if r:
        t_lap.append(ms_l)
        t_pred.append(ms_p)
lap, pred = float(np.median(t_lap)), float(np.median(t_pred))
extra = pred - lap
flops = float(a.n) ** 2 * a.m * a.batch
rate = flops / (extra * 1e-3) / 1e12
print('var in (0, sigma]: {0}  prob range [{1:.3g}, {2:.3g}]'.format(
    bool(np.all((var > 0) & (var <= np.exp(th[:, :1])))), prob.min(), prob.max()))
print('median of {0}: laplace {1:.2f} ms  predict {2:.2f} ms  (predict - laplace) / laplace = '
      '{3:.3f}'.format(a.reps, lap, pred, extra / lap))
print('predictive part {0:.2f} ms for {1:.3g} f64 flops: {2:.2f} TFLOP/s = {3:.1f}% of {4}'
      .format(extra, flops, rate, 100.0 * rate / PEAK_F64_TFLOPS, PEAK_F64_TFLOPS))
