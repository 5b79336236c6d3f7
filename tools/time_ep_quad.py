"""Device time of the EP fit with the tilted moments by quadrature (k_ep_sites_q)
against the closed-form probit fit (k_ep_sites) of the same build, on the same data and thetas:
HIP events on the context's stream around each Context.ep call, the median of `reps` runs after a
cold one (tools/time_ep.py's method).

Three fits per rep: the probit by its closed form, the probit by quadrature (the same fixed point,
so the same sweeps: the site kernels compare launch for launch) and the logit by quadrature.
Reports each call's time, sweeps and the share of its site kernel (the library's own event pairs,
APM_PROF_EP_SITES). Development tool; no threshold is attached."""
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
th = np.tile(np.r_[a.theta0, np.full(a.d, np.log(np.sqrt(a.d)))], (a.batch, 1))
th += np.random.RandomState(0).normal(scale=0.1, size=th.shape)
ev = [ctypes.c_void_p() for _ in range(2)]
for e in ev:
    _ok(hip.hipEventCreate(ctypes.byref(e)))
RUNS = (('probit closed form', 'probit', False), ('probit quadrature', 'probit', True),
        ('logit quadrature', 'logit', True))
ctxs = {}
for label, lik, quad in RUNS:
    ctxs[label] = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, 1, max_batch=a.batch, n_slots=1,
                                  n_ubufs=1, likelihood=lik, ep_quadrature=quad)
    ctxs[label].prof_enable(1)


def timed(ctx):
    ctx.prof_read(_native.PROF_EP_SITES, reset=True)
    _ok(hip.hipEventRecord(ev[0], ctx.stream_ptr))
    out = ctx.ep(th)
    _ok(hip.hipEventRecord(ev[1], ctx.stream_ptr))
    _ok(hip.hipEventSynchronize(ev[1]))
    ms = ctypes.c_float()
    _ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]))
    site_ms, launches, _ = ctx.prof_read(_native.PROF_EP_SITES, reset=True)
    return float(ms.value), site_ms, launches, out


res = {label: [] for label, _, _ in RUNS}
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    for label, _, _ in RUNS:
        ms, site_ms, launches, out = timed(ctxs[label])
        assert not out[5].any(), (label, out[5])
        print('rep {0} {1}: ep {2:.2f} ms (sweeps {3}), site kernel {4:.3f} ms in {5} launches'
              .format(r, label, ms, sorted(out[6].tolist()), site_ms, launches), flush=True)
        if r:
            res[label].append((ms, site_ms, launches))
base = None
for label, _, _ in RUNS:
    ms, site, launches = (float(np.median([t[k] for t in res[label]])) for k in range(3))
    base = base or (ms, site / launches)
    print('median of {0}, {1}: ep {2:.2f} ms ({3:.2f} x the closed form), site kernel {4:.3f} ms = '
          '{5:.2f}% of the call, {6:.1f} us per launch ({7:.2f} x the closed form)'
          .format(a.reps, label, ms, ms / base[0], site, 100.0 * site / ms,
                  1e3 * site / launches, site / launches / base[1]))
