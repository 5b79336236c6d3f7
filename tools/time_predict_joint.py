"""Device time of the joint Laplace / EP predictive (apm_predict_joint) beside the
marginal call (apm_predict / apm_ep_predict) at the same m: HIP events on the context's stream
(apm_stream) around each call, the median with the smallest and the largest of `reps` rounds after
a cold one; a round runs the four forms one after the other, so they alternate and see the same
machine. Three forms of the joint call are timed: the covariance alone, the draws' log predictive density alone (factor,
normals, draw kernel, reduction; nothing but `count` doubles comes back) and everything with the
draws copied to the host. The last line gives the work of one k_joint_draw launch computed from
the shapes, to be divided by the kernel's time from a kernel trace taken in a run of its own
(the trace slows the host, so the medians printed under it are not the figures to quote).
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
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--m', type=int, default=2048)
ap.add_argument('--n-draws', type=int, default=1024)
ap.add_argument('--reps', type=int, default=9)
ap.add_argument('--theta0', type=float, default=0.0, help='log signal variance of the thetas')
ap.add_argument('--fit', choices=('laplace', 'ep'), default='laplace')
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


B, S, m = a.batch, a.n_draws, a.m
X, y = utils.synthetic_gp_data(a.n, a.d, 20151009)
rng = np.random.RandomState(1)
Xs = 2.0 * rng.normal(size=(m, a.d))  # away from the training inputs and from each other
ys = np.where(rng.normal(size=m) > 0, 1.0, -1.0)
ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, 1, max_batch=B, n_slots=1, n_ubufs=1,
                      likelihood=a.likelihood, ep_quadrature=a.likelihood == 'logit')
approx = _native.JOINT_EP if a.fit == 'ep' else _native.JOINT_LAPLACE
marginal = ctx.ep_predict if a.fit == 'ep' else ctx.predict
th = np.tile(np.r_[a.theta0, np.full(a.d, np.log(np.sqrt(a.d)))], (B, 1))
th += np.random.RandomState(0).normal(scale=0.1, size=th.shape)
seeds = np.arange(B, dtype=np.uint64) + 20151009
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


forms = (
    ('marginal', lambda: marginal(th, Xs)),
    ('cov', lambda: ctx.predict_joint(approx, th, Xs)),
    ('lpd', lambda: ctx.predict_joint(approx, th, Xs, want_cov=False, n_draws=S, seeds=seeds,
                                      y_test=ys)),
    ('all', lambda: ctx.predict_joint(approx, th, Xs, n_draws=S, seeds=seeds, want_draws=True,
                                      y_test=ys)),
)
t = dict((k, []) for k, _ in forms)
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    line = []
    for k, fn in forms:
        ms, out = timed(fn)
        st = out[3] if k == 'marginal' else out[4]
        assert not st.any(), (k, st)
        if k != 'marginal':
            assert np.array_equal(out[0], mean)  # bitwise the marginal call's mean
        else:
            mean = out[0]
        line.append('{0} {1:.2f} ms'.format(k, ms))
        if r:
            t[k].append(ms)
    print('rep {0}: {1}'.format(r, '  '.join(line)), flush=True)
med = dict((k, float(np.median(v))) for k, v in t.items())
print('N {0} D {1} m {2} draws {3}, {4} thetas, {5}/{6}, {7} rounds:'.format(
    a.n, a.d, m, S, B, a.fit, a.likelihood, a.reps))
for k, _ in forms:
    # the ratio's range: this form's extremes over the marginal call's opposite extremes
    print('  {0:8s} median {1:8.2f} ms  (min {2:.2f}, max {3:.2f})  {4:.3f} x the marginal call '
          '({5:.3f} .. {6:.3f})'.format(k, med[k], min(t[k]), max(t[k]), med[k] / med['marginal'],
                                        min(t[k]) / max(t['marginal']),
                                        max(t[k]) / min(t['marginal'])))
mb, nst = (m + 63) // 64, (S + 63) // 64
flops = 2.0 * 64 ** 3 * (mb * (mb + 1) // 2) * nst * B
print('k_joint_draw: {0} tiles of depth 64 (mb {1}, draw tiles {2}, {3} chains) = {4:.3f} GFLOP '
      'per launch'.format((mb * (mb + 1) // 2) * nst * B, mb, nst, B, flops / 1e9))
ctx.close()
