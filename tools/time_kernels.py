"""Device time of the covariance-dependent kernels for every covariance kind the library builds
(SE, Matérn 3/2, Matérn 5/2; iso and ARD): the Gram builder inside the Laplace theta-call
(APM_PROF_GRAM) and k_grad_reduce (APM_PROF_GRAD_REDUCE), each an event pair around its one
launch, and the whole Context.laplace_grad call (HIP events on the context's stream), at a given
size. Median of `reps` calls after a cold one, as tools/time_grad.py; the spread of the
repetitions (max - min) is printed beside every median so that two libraries' rows can be told
apart from run-to-run noise.

The six kinds are followed by their biased twins (APM_COV_BIAS: the constant term exp(theta[-1])
with log beta = --log-beta), whose k_grad_reduce is another instantiation.

APM_LIB selects the library, so an older build can be timed with the same tool; kinds it does
not know (apm_version() < 2: SE only; a library without APM_COV_BIAS refuses the biased kinds at
apm_create) are left out. Development tool; no threshold is attached."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))
from gpdemo import _native  # noqa: E402
from gpdemo import utils  # noqa: E402

KINDS = [('se_iso', _native.KERNEL_ISO, True), ('se_ard', _native.KERNEL_ARD, False),
         ('matern32_iso', _native.KERNEL_M32_ISO, True),
         ('matern32_ard', _native.KERNEL_M32_ARD, False),
         ('matern52_iso', _native.KERNEL_M52_ISO, True),
         ('matern52_ard', _native.KERNEL_M52_ARD, False)]
KINDS += [(name + '+bias', kind | _native.COV_BIAS, iso) for name, kind, iso in KINDS]

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=4096)
ap.add_argument('--d', type=int, default=32)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--tol', type=float, default=1e-14, help='Newton tolerance')
ap.add_argument('--theta0', type=float, default=0.0, help='log signal variance of the thetas')
ap.add_argument('--log-beta', type=float, default=1.5, help='log beta of the biased kinds')
ap.add_argument('--kinds', default='', help='comma-separated subset of the kind names')
ap.add_argument('--json', default='', help='also write the result rows to this file')
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


lib = _native.load_library()
version = int(lib.apm_version())
want = [k for k in a.kinds.split(',') if k]
kinds = [k for k in KINDS if (not want or k[0] in want) and (version >= 2 or k[0].startswith('se_'))]
X, y = utils.synthetic_gp_data(a.n, a.d, 20151009)
ev = [ctypes.c_void_p() for _ in range(2)]
for e in ev:
    _ok(hip.hipEventCreate(ctypes.byref(e)))
print('library {0} (apm_version {1}), N = {2}, D = {3}, {4} thetas, Newton tolerance {5:g}, '
      'median of {6} after a cold call'.format(_native.LIB_PATH, version, a.n, a.d, a.batch,
                                               a.tol, a.reps), flush=True)
rows = []
for name, kind, iso in kinds:
    try:
        ctx = _native.Context(X, y, kind, 1e-8, 1, max_batch=a.batch, n_slots=1, n_ubufs=1)
    except _native.NativeError as e:
        print('{0:18s} NOT TIMED: {1}'.format(name, e), flush=True)
        continue
    ctx.set_newton(a.tol, 1000)
    th = np.tile(np.r_[a.theta0, np.full(1 if iso else a.d, np.log(np.sqrt(a.d)))], (a.batch, 1))
    th += np.random.RandomState(0).normal(scale=0.1, size=th.shape)  # (the base kind's draws)
    if kind & _native.COV_BIAS:
        th = np.hstack([th, np.full((a.batch, 1), a.log_beta)])
    t = {'gram': [], 'grad_reduce': [], 'laplace_grad': []}
    for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
        ctx.prof_read(_native.PROF_GRAM, reset=True)  # (a reset drops the records of every kind)
        ctx.prof_enable(1)
        _ok(hip.hipEventRecord(ev[0], ctx.stream_ptr))
        lml, grad, st, nit = ctx.laplace_grad(th)
        _ok(hip.hipEventRecord(ev[1], ctx.stream_ptr))
        _ok(hip.hipEventSynchronize(ev[1]))
        ctx.prof_enable(0)
        ms = ctypes.c_float()
        _ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]))
        ms_g, n_g, _ = ctx.prof_read(_native.PROF_GRAM)
        ms_r, n_r, _ = ctx.prof_read(_native.PROF_GRAD_REDUCE, reset=True)
        if st.any() or not np.all(np.isfinite(grad)) or n_g != 1 or n_r != 1:
            break  # (reported below: a kind that cannot be timed at these thetas is left out)
        if r:
            t['gram'].append(ms_g)
            t['grad_reduce'].append(ms_r)
            t['laplace_grad'].append(float(ms.value))
    ctx.close()
    if len(t['gram']) < a.reps:
        print('{0:18s} NOT TIMED: status {1}, iterations {2}, launches gram {3} / k_grad_reduce '
              '{4}'.format(name, st.tolist(), nit.tolist(), n_g, n_r), flush=True)
        continue
    row = {'kind': name, 'iterations': sorted(int(i) for i in nit)}
    for key, v in t.items():
        row[key + '_ms'] = float(np.median(v))
        row[key + '_spread_ms'] = float(max(v) - min(v))
    rows.append(row)
    print('{0:18s} gram {1:.3f} ms (spread {2:.3f})  k_grad_reduce {3:.3f} ms (spread {4:.3f})  '
          'laplace_grad {5:.2f} ms (spread {6:.2f})  iterations {7}'
          .format(name, row['gram_ms'], row['gram_spread_ms'], row['grad_reduce_ms'],
                  row['grad_reduce_spread_ms'], row['laplace_grad_ms'],
                  row['laplace_grad_spread_ms'], row['iterations']), flush=True)
out = {'library': _native.LIB_PATH, 'apm_version': version, 'n': a.n, 'd': a.d, 'batch': a.batch,
       'tol': a.tol, 'reps': a.reps, 'rows': rows}
print(json.dumps(out))
if a.json:
    with open(a.json, 'w') as f:
        json.dump(out, f, indent=1)
