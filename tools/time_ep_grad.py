"""Device time of the gradient of log Z_EP (Context.ep_grad) at a given size: HIP events on the
context's stream (apm_stream) around each call, the median of `reps` runs after a cold one.

Times the EP fit alone (Context.ep) against fit plus gradient pass (Context.ep_grad) at the same
EP settings, which isolates the cost of the extra pass; the Laplace gradient
(Context.laplace_grad) beside them; and the share of the contraction kernel (k_grad_reduce, timed
by the library's own event pairs: APM_PROF_GRAD_REDUCE) in the ep_grad call, with its read rate
against the streaming-read rate of one MI355X (development tool; no threshold is attached)."""
import argparse
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))
from gpdemo import _native  # noqa: E402
from gpdemo import utils  # noqa: E402

STREAM_READ_TBPS = 6.3  # achievable streaming-read rate of HBM3E on one MI355X (8 TB/s peak)

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=4096)
ap.add_argument('--d', type=int, default=32)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--theta0', type=float, default=0.0, help='log signal variance of the thetas')
ap.add_argument('--diff-tol', type=float, default=1e-16, help="EP stop tolerance (EPGradient's)")
ap.add_argument('--newton-tol', type=float, default=1e-14, help="LaplaceGradient's diff_f_tol")
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
ctx.set_ep(0.8, a.diff_tol, 1000)
ctx.set_newton(a.newton_tol, 1000)
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


ctx.prof_enable(1)
t_ep, t_eg, t_lg, t_red, t_lred, b_red = [], [], [], [], [], []
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    ms_e, fit = timed(lambda: ctx.ep(th))
    ctx.prof_read(_native.PROF_GRAD_REDUCE, reset=True)
    ms_g, (logz, grad, st, nsw) = timed(lambda: ctx.ep_grad(th))
    ms_r, launches, nbytes = ctx.prof_read(_native.PROF_GRAD_REDUCE, reset=True)
    ms_l, (lml, lgrad, lst, nit) = timed(lambda: ctx.laplace_grad(th))
    ms_lr = ctx.prof_read(_native.PROF_GRAD_REDUCE, reset=True)[0]
    assert not st.any() and not lst.any() and not fit[5].any()
    assert np.array_equal(logz, fit[0]) and np.array_equal(nsw, fit[6])
    print('rep {0}: ep {1:.2f} ms  ep_grad {2:.2f} ms (sweeps {3})  laplace_grad {4:.2f} ms '
          '({5} iterations)  k_grad_reduce {6:.3f} ms in {7} launch(es); {8:.3f} ms in '
          'laplace_grad'.format(r, ms_e, ms_g, sorted(nsw.tolist()), ms_l, sorted(nit.tolist()),
                                ms_r, launches, ms_lr), flush=True)
    if r:
        t_ep.append(ms_e)
        t_eg.append(ms_g)
        t_lg.append(ms_l)
        t_red.append(ms_r)
        t_lred.append(ms_lr)
        b_red.append(nbytes)
epm, egm, lgm, red, lred = (float(np.median(t)) for t in (t_ep, t_eg, t_lg, t_red, t_lred))
rate = float(np.median(b_red)) / (red * 1e-3) / 1e12
print('log Z_EP range [{0:.3f}, {1:.3f}]  max|grad| {2:.3f}  (Laplace LML range [{3:.3f}, '
      '{4:.3f}], max|grad| {5:.3f})'.format(logz.min(), logz.max(), np.abs(grad).max(),
                                            lml.min(), lml.max(), np.abs(lgrad).max()))
print('median of {0}: ep {1:.2f} ms  ep_grad {2:.2f} ms  the gradient pass {3:.2f} ms = {4:.1f}% '
      'on top of the fit = {5:.2f} sweeps'.format(a.reps, epm, egm, egm - epm,
                                                   100.0 * (egm - epm) / epm,
                                                   (egm - epm) / (epm / max(1, int(nsw.max())))))
print('laplace_grad {0:.2f} ms  ep_grad / laplace_grad = {1:.2f}'.format(lgm, egm / lgm))
print('k_grad_reduce {0:.3f} ms = {1:.2f}% of the ep_grad call ({2:.3f} ms = {3:.2f}% of '
      'laplace_grad), {4:.2f} TB/s = {5:.0f}% of the {6} TB/s streaming-read rate'
      .format(red, 100.0 * red / egm, lred, 100.0 * lred / lgm, rate,
              100.0 * rate / STREAM_READ_TBPS, STREAM_READ_TBPS))
