"""Device time of the expectation-propagation fit (Context.ep) against the Laplace theta-call at a
given size: HIP events on the context's stream (apm_stream) around each call, the median of
`reps` runs after a cold one.

Reports the sweeps per chain, the share of the site kernel (k_ep_sites, timed by the library's
own event pairs: APM_PROF_EP_SITES) in the EP call and its read rate against the streaming-read
rate of one MI355X (development tool; no threshold is attached)."""
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
t_lap, t_ep, t_site, b_site = [], [], [], []
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    ms_l, (_, st, nit) = timed(lambda: ctx.theta_eval(_native.EST_LAPLACE, th))
    ctx.prof_read(_native.PROF_EP_SITES, reset=True)
    ms_e, (logz, _, var, _, _, est, nsw) = timed(lambda: ctx.ep(th))
    ms_s, launches, nbytes = ctx.prof_read(_native.PROF_EP_SITES, reset=True)
    assert not st.any() and not est.any()
    print('rep {0}: laplace {1:.2f} ms ({2} iterations)  ep {3:.2f} ms (sweeps {4}), site kernel '
          '{5:.3f} ms in {6} launches'.format(r, ms_l, sorted(nit.tolist()), ms_e,
                                              sorted(nsw.tolist()), ms_s, launches), flush=True)
    if r:
        t_lap.append(ms_l)
        t_ep.append(ms_e)
        t_site.append(ms_s)
        b_site.append(nbytes)
lap, epm, site = (float(np.median(t)) for t in (t_lap, t_ep, t_site))
rate = float(np.median(b_site)) / (site * 1e-3) / 1e12
print('log Z_EP range [{0:.3f}, {1:.3f}]  var > 0: {2}'.format(logz.min(), logz.max(),
                                                             bool(np.all(var > 0))))
print('median of {0}: laplace {1:.2f} ms  ep {2:.2f} ms  ep / laplace = {3:.2f}  ep per sweep '
      '{4:.2f} ms'.format(a.reps, lap, epm, epm / lap, epm / max(1, int(nsw.max()))))
print('site kernel {0:.3f} ms = {1:.2f}% of the ep call, {2:.2f} TB/s = {3:.0f}% of the {4} TB/s '
      'streaming-read rate'.format(site, 100.0 * site / epm, rate,
                                   100.0 * rate / STREAM_READ_TBPS, STREAM_READ_TBPS))
