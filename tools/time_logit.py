"""Device time of the logistic likelihood against the probit's on the same data and thetas
(DESIGN.md §15): the IS theta-call, the cached u-call and Context.predict, each under both
likelihoods, with HIP events on the context's stream (apm_stream) around each call; the median of
`reps` runs after a cold call.

The two likelihoods converge in different numbers of Newton iterations, and a theta-call's time
is mostly its iterations: the counts are printed beside the times, and the theta-call's ratio is
also given per iteration. Development tool; no threshold is attached."""
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
ap.add_argument('--m', type=int, default=4096, help='test inputs of the predict call')
ap.add_argument('--n-imp', type=int, default=256)
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
Xs = np.random.RandomState(1).normal(size=(a.m, a.d))
th = np.tile(np.r_[a.theta0, np.full(a.d, np.log(np.sqrt(a.d)))], (a.batch, 1))
th += np.random.RandomState(0).normal(scale=0.1, size=th.shape)
B = a.batch
ev = [ctypes.c_void_p() for _ in range(2)]
for e in ev:
    _ok(hip.hipEventCreate(ctypes.byref(e)))


def measure(likelihood):
    ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, a.n_imp, max_batch=B, n_slots=B,
                          n_ubufs=2 * B, likelihood=likelihood)

    def timed(fn):
        _ok(hip.hipEventRecord(ev[0], ctx.stream_ptr))
        out = fn()
        _ok(hip.hipEventRecord(ev[1], ctx.stream_ptr))
        _ok(hip.hipEventSynchronize(ev[1]))
        ms = ctypes.c_float()
        _ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]))
        return float(ms.value), out

    ub = np.arange(B)
    for k in (0, 1):  # (at most max_batch buffers per call)
        ctx.u_normal(ub + k * B, np.full(B, 7), ub + k * B)
    t = {'theta': [], 'u': [], 'predict': []}
    for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
        ms_t, (val, st, nops) = timed(lambda: ctx.theta_eval(_native.EST_IS, th, ub, np.arange(B)))
        ms_u, (uval, ust) = timed(lambda: ctx.u_eval(np.arange(B), ub + B))
        ms_p, (mean, var, prob, pst, pit) = timed(lambda: ctx.predict(th, Xs))
        assert not st.any() and not ust.any() and not pst.any()
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(uval)) and np.all(np.isfinite(prob))
        its = nops - 3  # (n_cubic_ops = n_iter + 1 + 2)
        print('{0} rep {1}: theta-call {2:.2f} ms (Newton iterations {3})  u-call {4:.3f} ms  '
              'predict {5:.2f} ms (fp64 Newton iterations {6})'
              .format(likelihood, r, ms_t, sorted(its.tolist()), ms_u, ms_p,
                      sorted(pit.tolist())), flush=True)
        if r:
            t['theta'].append(ms_t)
            t['u'].append(ms_u)
            t['predict'].append(ms_p)
    ctx.close()
    out = {k: float(np.median(v)) for k, v in t.items()}
    out['iters'] = int(its.max())
    out['predict_iters'] = int(pit.max())
    return out


res = {lik: measure(lik) for lik in ('probit', 'logit')}
p, l = res['probit'], res['logit']
print('N = {0}, D = {1}, n_imp = {2}, {3} thetas, M = {4}; median of {5} after a cold call'
      .format(a.n, a.d, a.n_imp, B, a.m, a.reps))
print('| call | probit ms | logit ms | logit / probit | Newton iterations (max over the batch) |')
print('|---|---|---|---|---|')
print('| IS theta-call | {0:.2f} | {1:.2f} | {2:.3f} | {3} / {4} |'
      .format(p['theta'], l['theta'], l['theta'] / p['theta'], p['iters'], l['iters']))
print('| IS theta-call per Newton iteration | {0:.2f} | {1:.2f} | {2:.3f} | |'
      .format(p['theta'] / p['iters'], l['theta'] / l['iters'],
              (l['theta'] / l['iters']) / (p['theta'] / p['iters'])))
print('| cached u-call | {0:.3f} | {1:.3f} | {2:.3f} | |'
      .format(p['u'], l['u'], l['u'] / p['u']))
print('| predict, M = {0} | {1:.2f} | {2:.2f} | {3:.3f} | {4} / {5} |'
      .format(a.m, p['predict'], l['predict'], l['predict'] / p['predict'], p['predict_iters'],
              l['predict_iters']))
