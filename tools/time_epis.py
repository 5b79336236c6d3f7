"""Device time of the IS theta-call with the EP importance distribution (EST_IS_EP) against the one
with the Laplace posterior (EST_IS) at a given size, and of the u-call on a slot of each: HIP
events on the context's stream (apm_stream) around each call, the median of `reps` runs after a
cold one.

With --spread R it also prints, per theta, the standard deviation of the log-estimate over R draw
matrices (u-calls on the two slots) for both proposals: what the longer theta-call buys
(DESIGN.md §17). Development tool; no threshold is attached."""
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
ap.add_argument('--n-imp', type=int, default=64)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--theta0', type=float, default=0.0, help='log signal variance of the thetas')
ap.add_argument('--spread', type=int, default=32, help='draw matrices of the spread (0: none)')
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
ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, a.n_imp, max_batch=B, n_slots=2 * B,
                      n_ubufs=1)
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


SEED = 20151009
ub = [0] * B
sl_is, sl_ep = list(range(B)), list(range(B, 2 * B))
ctx.u_normal([0], [SEED], [0])
t = dict(is_theta=[], ep_theta=[], is_u=[], ep_u=[])
for r in range(a.reps + 1):  # rep 0 is cold (tile lists, first launches, lazy buffers)
    ms_i, (_, st_i, nop_i) = timed(lambda: ctx.theta_eval(_native.EST_IS, th, ub, sl_is))
    ms_e, (_, st_e, nop_e) = timed(lambda: ctx.theta_eval(_native.EST_IS_EP, th, ub, sl_ep))
    ms_ui, (_, su_i) = timed(lambda: ctx.u_eval(sl_is, ub))
    ms_ue, (_, su_e) = timed(lambda: ctx.u_eval(sl_ep, ub))
    assert not st_i.any() and not st_e.any() and not su_i.any() and not su_e.any()
    nit, nsw = nop_i - 3, (nop_e - 3) // 2
    print('rep {0}: EST_IS {1:.2f} ms ({2} Newton iterations)  EST_IS_EP {3:.2f} ms (sweeps {4})  '
          'u-call {5:.2f} / {6:.2f} ms'.format(r, ms_i, sorted(nit.tolist()), ms_e,
                                                sorted(nsw.tolist()), ms_ui, ms_ue), flush=True)
    if r:
        for k, v in (('is_theta', ms_i), ('ep_theta', ms_e), ('is_u', ms_ui), ('ep_u', ms_ue)):
            t[k].append(v)
m = dict((k, float(np.median(v))) for k, v in t.items())
print('median of {0}: theta-call EST_IS {1:.2f} ms  EST_IS_EP {2:.2f} ms  ratio {3:.2f}  '
      '({4:.2f} ms per sweep and chain batch)'.format(
          a.reps, m['is_theta'], m['ep_theta'], m['ep_theta'] / m['is_theta'],
          m['ep_theta'] / max(1, int(nsw.max()))))
print('median of {0}: u-call on EST_IS slots {1:.2f} ms  on EST_IS_EP slots {2:.2f} ms'.format(
    a.reps, m['is_u'], m['ep_u']))
if a.spread > 0:
    vals = np.empty((a.spread, 2, B))
    for k in range(a.spread):
        ctx.u_normal([0], [SEED], [1 + k])
        vals[k, 0], s0 = ctx.u_eval(sl_is, ub)
        vals[k, 1], s1 = ctx.u_eval(sl_ep, ub)
        assert not s0.any() and not s1.any()
    sd = vals.std(0)
    for b in range(B):
        print('theta {0}: sd of the log-estimate over {1} draw matrices: EST_IS {2:.4f}  '
              'EST_IS_EP {3:.4f}  ratio {4:.3f}'.format(b, a.spread, sd[0, b], sd[1, b],
                                                        sd[1, b] / sd[0, b]))
    print('spread: median sd EST_IS {0:.4f}  EST_IS_EP {1:.4f}  median variance ratio {2:.3f}'
          .format(float(np.median(sd[0])), float(np.median(sd[1])),
                  float(np.median((sd[1] / sd[0]) ** 2))))
