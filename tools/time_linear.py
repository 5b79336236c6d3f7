"""Device time of the kernels the linear covariance term (APM_COV_LINEAR) adds work
to, with and without the flag: the Gram builder inside the Laplace theta-call (APM_PROF_GRAM) and
the gradient contraction (APM_PROF_GRAD_REDUCE: k_grad_reduce and, with the flag, k_grad_lin
behind it), each the library's own HIP event pair around its launches, inside
Context.laplace_grad; then Context.predict at --m test rows, whose k_gram_cross launches have no
event pair of their own: run the tool under `rocprofv3 --kernel-trace --stats -- python
tools/time_linear.py --cross-only` and read k_gram_cross's row (the whole call's HIP-event time
is printed as well). Median of `reps` calls after a cold one, max - min beside it, as
tools/time_kernels.py. Development tool; no threshold is attached."""
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

B, L = _native.COV_BIAS, _native.COV_LINEAR
KINDS = [('se_iso', _native.KERNEL_ISO), ('se_iso+linear', _native.KERNEL_ISO | L),
         ('se_ard', _native.KERNEL_ARD), ('se_ard+linear', _native.KERNEL_ARD | L),
         ('se_iso+bias', _native.KERNEL_ISO | B), ('se_iso+bias+linear', _native.KERNEL_ISO | B | L),
         ('se_ard+bias', _native.KERNEL_ARD | B), ('se_ard+bias+linear', _native.KERNEL_ARD | B | L)]

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=4096)
ap.add_argument('--d', type=int, default=32)
ap.add_argument('--m', type=int, default=4096, help='test rows of the predict call')
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--tol', type=float, default=1e-14, help='Newton tolerance of laplace_grad')
ap.add_argument('--theta0', type=float, default=0.0, help='log signal variance of the thetas')
ap.add_argument('--log-beta', type=float, default=1.5)
ap.add_argument('--log-lambda', type=float, default=-2.0)
ap.add_argument('--kinds', default='', help='comma-separated subset of the kind names')
ap.add_argument('--cross-only', action='store_true', help='the predict calls only')
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


def _timed(ctx, call):
    _ok(hip.hipEventRecord(ev[0], ctx.stream_ptr))
    out = call()
    _ok(hip.hipEventRecord(ev[1], ctx.stream_ptr))
    _ok(hip.hipEventSynchronize(ev[1]))
    ms = ctypes.c_float()
    _ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]))
    return out, float(ms.value)


lib = _native.load_library()
want = [k for k in a.kinds.split(',') if k]
X, y = utils.synthetic_gp_data(a.n, a.d, 20151009)
Xs = np.random.RandomState(1).normal(size=(a.m, a.d))
ev = [ctypes.c_void_p() for _ in range(2)]
for e in ev:
    _ok(hip.hipEventCreate(ctypes.byref(e)))
print('library {0}, N = {1}, D = {2}, {3} thetas, M = {4}, median of {5} after a cold call'
      .format(_native.LIB_PATH, a.n, a.d, a.batch, a.m, a.reps), flush=True)
rows = []
for name, kind in KINDS:
    if want and name not in want:
        continue
    iso = (kind & ~(B | L)) == _native.KERNEL_ISO
    ctx = _native.Context(X, y, kind, 1e-8, 1, max_batch=a.batch, n_slots=1, n_ubufs=1)
    th = np.tile(np.r_[a.theta0, np.full(1 if iso else a.d, np.log(np.sqrt(a.d)))], (a.batch, 1))
    th += np.random.RandomState(0).normal(scale=0.1, size=th.shape)  # (the base kind's draws)
    if kind & B:
        th = np.hstack([th, np.full((a.batch, 1), a.log_beta)])
    if kind & L:
        th = np.hstack([th, np.full((a.batch, 1), a.log_lambda)])
    t = {'gram': [], 'grad_reduce': [], 'laplace_grad': [], 'predict': []}
    ok = True
    for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
        if not a.cross_only:
            ctx.set_newton(a.tol, 1000)
            ctx.prof_read(_native.PROF_GRAM, reset=True)
            ctx.prof_enable(1)
            (lml, grad, st, nit), ms = _timed(ctx, lambda: ctx.laplace_grad(th))
            ctx.prof_enable(0)
            ms_g, n_g, _ = ctx.prof_read(_native.PROF_GRAM)
            ms_r, n_r, _ = ctx.prof_read(_native.PROF_GRAD_REDUCE, reset=True)
            if st.any() or not np.all(np.isfinite(grad)) or n_g != 1 or n_r != 1:
                print('{0:20s} NOT TIMED: status {1}, launches gram {2} / contraction {3}'
                      .format(name, st.tolist(), n_g, n_r), flush=True)
                ok = False
                break
            if r:
                t['gram'].append(ms_g)
                t['grad_reduce'].append(ms_r)
                t['laplace_grad'].append(ms)
        ctx.set_newton(1e-4, 1000)
        p, ms = _timed(ctx, lambda: ctx.predict(th, Xs))
        if p[3].any():
            print('{0:20s} NOT TIMED: predict status {1}'.format(name, p[3].tolist()), flush=True)
            ok = False
            break
        if r:
            t['predict'].append(ms)
    ctx.close()
    if not ok:
        continue
    row = {'kind': name}
    for key, v in t.items():
        if v:
            row[key + '_ms'] = float(np.median(v))
            row[key + '_spread_ms'] = float(max(v) - min(v))
    rows.append(row)
    print('{0:20s} '.format(name) + '  '.join(
        '{0} {1:.3f} ms (spread {2:.3f})'.format(k, row[k + '_ms'], row[k + '_spread_ms'])
        for k in t if k + '_ms' in row), flush=True)
out = {'library': _native.LIB_PATH, 'n': a.n, 'd': a.d, 'm': a.m, 'batch': a.batch, 'tol': a.tol,
       'reps': a.reps, 'rows': rows}
print(json.dumps(out))
if a.json:
    with open(a.json, 'w') as f:
        json.dump(out, f, indent=1)
