"""ctypes binding of libapm.so (include/apm.h) — the only way the Python layer reaches the GPU.

There is deliberately no CPU fallback: if the library is missing or no HIP device is visible,
every estimator / kernel entry point raises :class:`NativeUnavailableError`.
"""
import collections
import ctypes
import os
import threading

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get('APM_LIB', os.path.join(_PKG_ROOT, 'lib', 'libapm.so'))

# include/apm.h constants
KERNEL_ISO, KERNEL_ARD, KERNEL_PRECOMPUTED = 0, 1, 2
KERNEL_M32_ISO, KERNEL_M32_ARD, KERNEL_M52_ISO, KERNEL_M52_ARD = 3, 4, 5, 6
# the kinds with one length scale (theta has 2 entries; the others' has d + 1)
_ISO_KINDS = (KERNEL_ISO, KERNEL_M32_ISO, KERNEL_M52_ISO)
# APM_COV_BIAS: OR-ed onto one of the six device kinds, the constant term beta = exp(theta[-1])
# (theta has one more entry)
COV_BIAS = 16
# APM_COV_LINEAR: OR-ed onto KERNEL_ISO or KERNEL_ARD (with or without COV_BIAS), the linear term
# lambda x x^T with lambda = exp(theta[-1]); beta is then exp(theta[-2])
COV_LINEAR = 64


def theta_len(kind, d):
    """Entries of theta that covariance kind `kind` reads at d features."""
    return ((2 if (kind & ~(COV_BIAS | COV_LINEAR)) in _ISO_KINDS else d + 1)
            + (1 if kind & COV_BIAS else 0) + (1 if kind & COV_LINEAR else 0))

EST_IS, EST_PRIORMC, EST_LAPLACE = 0, 1, 2
EST_IS_EP = 3  # EST_IS with the EP fit's posterior as the importance distribution (probit)
LIK_PROBIT, LIK_LOGIT = 0, 1
_LIKELIHOODS = {'probit': LIK_PROBIT, 'logit': LIK_LOGIT}
APM_SUCCESS, APM_E_INVALID, APM_E_HIP, APM_E_NOMEM = 0, -1, -2, -3
STATUS_OK, STATUS_CHOL_K, STATUS_CHOL_B, STATUS_CHOL_C, STATUS_MAXITER = 0, 1, 2, 3, 4
STATUS_GUARD = 5
STATUS_EP_CAVITY = 6
PROF_GRAM, PROF_CHOL_UPDATE, PROF_UGEMM, PROF_CHOL_UPDATE32, PROF_STATS = 0, 1, 2, 3, 4
PROF_CHOL_UPDATE32_OUTER, PROF_CHOL_UPDATE_OUTER, PROF_DF_TIMEOUTS = 5, 6, 7
PROF_POST32_OUTER, PROF_POST64_RERUNS, PROF_TRSV_TIMEOUTS = 8, 9, 10
PROF_ICM_CHECKS, PROF_GUARD, PROF_GRAD_REDUCE, PROF_EP_SITES, PROF_NKINDS = 11, 12, 13, 14, 15
SPREAD_MAX_BLOCKS = 4096  # APM_SPREAD_MAX_BLOCKS: n_rep * nblk of one apm_is_spread call
PSIS_MAX_SAMPLES = 4096  # APM_PSIS_MAX_SAMPLES: the largest n_imp apm_is_loo_psis sorts
JOINT_LAPLACE, JOINT_EP = 0, 1  # APM_JOINT_*: the fit behind apm_predict_joint
JOINT_MAX_DRAWS = 4096  # APM_JOINT_MAX_DRAWS


class NativeUnavailableError(RuntimeError):
    """libapm.so or a HIP device is missing: the HIP path is mandatory (no CPU fallback)."""


class NativeError(RuntimeError):
    """A C-ABI call returned an APM_E_* code."""


_i64 = ctypes.c_int64
_p = ctypes.c_void_p
_d = ctypes.c_double
_i = ctypes.c_int

_SIGS = {
    'apm_version': (_i, []),
    'apm_device_count': (_i, []),
    'apm_global_error': (ctypes.c_char_p, []),
    'apm_create': (_p, [_i, _i, _p, _i64, _i64, _i64, _p, _d, _i64, _i64, _i64, _i64]),
    'apm_destroy': (None, [_p]),
    'apm_last_error': (ctypes.c_char_p, [_p]),
    'apm_padded_n': (_i64, [_p]),
    'apm_theta_len': (_i64, [_p]),
    'apm_set_newton': (_i, [_p, _d, _i64]),
    'apm_set_likelihood': (_i, [_p, _i]),
    'apm_likelihood': (_i, [_p]),
    'apm_stream': (_p, [_p]),
    'apm_u_upload': (_i, [_p, _i64, _p, _i64]),
    'apm_u_download': (_i, [_p, _i64, _p, _i64]),
    'apm_u_normal': (_i, [_p, _i64, _p, _p, _p]),
    'apm_u_combine': (_i, [_p, _i64, _p, _p, _p, _p, _p]),
    'apm_theta_eval': (_i, [_p, _i, _i64, _p, _i64, _p, _p, _p, _p, _p]),
    'apm_theta_eval_K': (_i, [_p, _i, _p, _i64, _i64, _i64, _p, _p, _p]),
    'apm_u_eval': (_i, [_p, _i64, _p, _p, _p, _p]),
    'apm_u_eval_diag': (_i, [_p, _i64, _p, _p, _i64, _p, _p, _p, _i64, _p]),
    'apm_is_spread': (_i, [_p, _i64, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _i64, _p]),
    'apm_is_loo': (_i, [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p]),
    'apm_is_loo_psis': (_i, [_p, _i64, _p, _p, _p, _p, _p, _i64, _p, _p, _i64, _p]),
    'apm_slot_read': (_i, [_p, _i64, _p, _i64, _p, _p, _p]),
    'apm_cache_acquire': (_i, [_p, _p]),
    'apm_cache_copy': (_i, [_p, _i64]),
    'apm_cache_release': (_i, [_p, _i64]),
    'apm_cache_refcount': (_i64, [_p, _i64]),
    'apm_gram': (_i, [_i, _i, _p, _i64, _i64, _i64, _p, _i64, _d, _p, _i64]),
    'apm_gram_cross': (_i, [_i, _i, _p, _i64, _p, _i64, _i64, _i64, _p, _i64, _p, _i64]),
    'apm_predict': (_i, [_p, _i64, _p, _i64, _p, _i64, _i64, _p, _p, _p, _i64, _p, _p]),
    'apm_is_predict': (_i, [_p, _i, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _i64,
                            _p, _p, _p]),
    'apm_laplace_grad': (_i, [_p, _i64, _p, _i64, _p, _p, _i64, _p, _p]),
    'apm_set_ep': (_i, [_p, _d, _d, _i64]),
    'apm_ep_eval': (_i, [_p, _i64, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _p]),
    'apm_ep_predict': (_i, [_p, _i64, _p, _i64, _p, _i64, _i64, _p, _p, _p, _i64, _p, _p]),
    'apm_ep_grad': (_i, [_p, _i64, _p, _i64, _p, _p, _i64, _p, _p]),
    'apm_predict_joint': (_i, [_p, _i, _i64, _p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _i64, _p,
                               _p, _p, _p, _p, _p, _p]),
    'apm_ep': (_i, [_i, _p, _i64, _i64, _p, _i, _d, _d, _i64, _p, _p, _p, _p, _p, _i64, _p, _p,
                    _p]),
    'apm_ep_lik': (_i, [_i, _i, _p, _i64, _i64, _p, _i, _d, _d, _i64, _p, _p, _p, _p, _p, _i64, _p,
                        _p, _p]),
    'apm_set_ep_quadrature': (_i, [_p, _i]),
    'apm_ep_quadrature': (_i, [_p]),
    'apm_laplace': (_i, [_i, _p, _i64, _i64, _p, _i, _i, _d, _i64, _p, _p, _i64, _p, _p, _p]),
    'apm_laplace_lik': (_i, [_i, _i, _p, _i64, _i64, _p, _i, _i, _d, _i64, _p, _p, _i64, _p, _p,
                             _p]),
    'apm_prof_enable': (_i, [_p, _i]),
    'apm_prof_marker': (_i, [_p, _i]),
    'apm_prof_read': (_i, [_p, _i, _p, _p, _p, _i]),
    'apm_guard_read': (_i, [_p, _i64, _p]),
    'apm_selftest_tile': (_i, [_i, _p, _p, _p]),
    'apm_selftest_philox': (_i, [_i, _i64, _p, _p]),
}

_lib = None
_lock = threading.Lock()


def exported_symbols():
    return sorted(_SIGS)


def load_library(check_device=True):
    """Load libapm.so (once). Raises NativeUnavailableError if absent or without a device."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NativeUnavailableError(
                    'libapm.so not found at {0}: build it with `python -c "import __graft_entry__'
                    ' as g; g.build()"` (no CPU fallback exists)'.format(LIB_PATH))
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    if check_device and _lib.apm_device_count() <= 0:
        raise NativeUnavailableError('no HIP device visible: the MI355X path is required '
                                     '(no CPU fallback exists)')
    return _lib


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _check(rc, ctx=None):
    if rc != 0:
        lib = load_library(check_device=False)
        msg = (lib.apm_last_error(ctx) if ctx else lib.apm_global_error()) or b''
        raise NativeError('libapm error {0}: {1}'.format(rc, msg.decode(errors='replace')))


def likelihood_code(likelihood):
    """APM_LIK_* of ``'probit'`` / ``'logit'``; anything else is a ValueError (raised before any
    device is touched, so a misspelt likelihood never falls back to the probit)."""
    try:
        return _LIKELIHOODS[likelihood]
    except (KeyError, TypeError):
        raise ValueError("likelihood must be 'probit' or 'logit', got {0!r}".format(likelihood))


def default_device():
    return int(os.environ.get('APM_DEVICE', os.environ.get('LOCAL_RANK', '0')))


def _device(device):
    return default_device() if device is None else device


# ----------------------------------------------------------------------------- stand-alone calls


def gram(kind, K, X, theta, epsilon, device=None):
    """Fill K (any writable float64 (n, n) array) with the Gram matrix of covariance kind `kind`
    (SE or Matern, iso or ARD) computed on the GPU."""
    lib = load_library()
    X = _f64(X)
    theta = _f64(np.atleast_1d(theta))
    n, d = X.shape
    if theta.shape[0] < theta_len(kind, d):
        # kernels.pyx indexes theta[k+1] / theta[1] with bounds checking -> IndexError
        raise IndexError('Out of bounds on buffer access (axis 0)')
    out = K if (isinstance(K, np.ndarray) and K.dtype == np.float64 and K.flags.c_contiguous
                and K.flags.writeable) else np.empty((n, n))
    _check(lib.apm_gram(_device(device), kind, _ptr(X), n, d, d, _ptr(theta), theta.shape[0],
                        float(epsilon), out.ctypes.data, n))
    if out is not K:
        K[...] = out
    return None


def gram_cross(kind, X_test, X, theta, device=None):
    """(m, n) cross-covariance k(X_test_i, X_j) of covariance kind `kind` on the GPU: no epsilon,
    also where a test point coincides with a training point."""
    lib = load_library()
    X, Xs = _f64(X), _f64(X_test)
    theta = _f64(np.atleast_1d(theta))
    n, d = X.shape
    if Xs.ndim != 2 or Xs.shape[1] != d:
        raise ValueError('X_test has shape {0}, expected (m, {1})'.format(Xs.shape, d))
    if theta.shape[0] < theta_len(kind, d):
        raise IndexError('Out of bounds on buffer access (axis 0)')
    Ks = np.empty((Xs.shape[0], n))
    _check(lib.apm_gram_cross(_device(device), kind, _ptr(Xs), Xs.shape[0], _ptr(X), n, d, d,
                              _ptr(theta), theta.shape[0], _ptr(Ks), n))
    return Ks


def laplace(K, y, calc_cov, calc_lml, diff_f_tol, max_iters, device=None, likelihood='probit'):
    lik = likelihood_code(likelihood)
    lib = load_library()
    K = _f64(K)
    y = _f64(y)
    n = K.shape[0]
    f = np.empty(n)
    C = np.empty((n, n)) if calc_cov else None
    lml = np.zeros(1)
    nit = np.zeros(1, dtype=np.int64)
    st = np.zeros(1, dtype=np.int32)
    dev = _device(device)
    tail = (_ptr(K), n, n, _ptr(y), int(bool(calc_cov)), int(bool(calc_lml)), float(diff_f_tol),
            int(max_iters), _ptr(f), _ptr(C), n, _ptr(lml), _ptr(nit), _ptr(st))
    if lik == LIK_PROBIT:  # (the entry point the reference's function maps onto)
        _check(lib.apm_laplace(dev, *tail))
    else:
        _check(lib.apm_laplace_lik(dev, lik, *tail))
    return f, C, float(lml[0]), int(nit[0]), int(st[0])


def ep(K, y, calc_cov, damping, diff_tol, max_sweeps, device=None, likelihood='probit'):
    """Stand-alone EP fit on a K of the caller's (include/apm.h apm_ep / apm_ep_lik):
    ``(mu, var, tau, nu, C, logz, n_sweeps, status)``, C None without calc_cov. The probit takes
    the closed-form tilted moments, the logit the quadrature rule."""
    lik = likelihood_code(likelihood)
    lib = load_library()
    K = _f64(K)
    y = _f64(y)
    n = K.shape[0]
    mu, var, tau, nu = (np.empty(n) for _ in range(4))
    C = np.empty((n, n)) if calc_cov else None
    logz = np.zeros(1)
    nsw = np.zeros(1, dtype=np.int64)
    st = np.zeros(1, dtype=np.int32)
    tail = (_ptr(K), n, n, _ptr(y), int(bool(calc_cov)), float(damping), float(diff_tol),
            int(max_sweeps), _ptr(mu), _ptr(var), _ptr(tau), _ptr(nu), _ptr(C), n, _ptr(logz),
            _ptr(nsw), _ptr(st))
    if lik == LIK_PROBIT:  # (the entry point that predates the likelihood argument)
        _check(lib.apm_ep(_device(device), *tail))
    else:
        _check(lib.apm_ep_lik(_device(device), lik, *tail))
    return mu, var, tau, nu, C, float(logz[0]), int(nsw[0]), int(st[0])


def selftest_tile(A, B, C, device=None):
    lib = load_library()
    A, B = _f64(A), _f64(B)
    C = _f64(C).copy()
    _check(lib.apm_selftest_tile(_device(device), _ptr(A), _ptr(B), _ptr(C)))
    return C


def selftest_philox(blocks, device=None):
    """Philox4x32-10 of (counter[4], key[2]) rows (uint32) through the device round function."""
    lib = load_library()
    inp = np.ascontiguousarray(blocks, dtype=np.uint32).reshape(-1, 6)
    out = np.empty((inp.shape[0], 4), dtype=np.uint32)
    _check(lib.apm_selftest_philox(_device(device), inp.shape[0], _ptr(inp), _ptr(out)))
    return out


# ----------------------------------------------------------------------------- context


class _Pool(object):
    def __init__(self, n):
        self.free = list(range(n - 1, -1, -1))
        self.refs = {}

    def acquire(self):
        if not self.free:
            raise NativeError('pool exhausted (raise n_slots / n_ubufs)')
        i = self.free.pop()
        self.refs[i] = 1
        return i

    def incref(self, i):
        self.refs[i] += 1

    def release(self, i):
        self.refs[i] -= 1
        if self.refs[i] == 0:
            del self.refs[i]
            self.free.append(i)


class _SlotPool(object):
    """Cache-slot owners kept by the library (apm_cache_acquire / _copy / _release): the same
    interface as _Pool, so a C caller and this layer share one ownership record."""

    def __init__(self, ctx):
        self.ctx = ctx

    def acquire(self):
        s = ctypes.c_int64(-1)
        _check(self.ctx.lib.apm_cache_acquire(self.ctx._h, ctypes.byref(s)), self.ctx._h)
        return int(s.value)

    def incref(self, i):
        _check(self.ctx.lib.apm_cache_copy(self.ctx._h, int(i)), self.ctx._h)

    def release(self, i):
        if self.ctx._h:
            _check(self.ctx.lib.apm_cache_release(self.ctx._h, int(i)), self.ctx._h)

    def refcount(self, i):
        return int(self.ctx.lib.apm_cache_refcount(self.ctx._h, int(i)))


class Context(object):
    """A device-resident problem (X, y, kernel, likelihood) with workspaces for up to
    `max_batch` chains. The likelihood (``'probit'`` / ``'logit'``) is fixed for the context's
    life: every cache slot it writes is read back under the same one."""

    def __init__(self, X, y, kernel_kind, epsilon, n_imp, max_batch=1, n_slots=4, n_ubufs=4,
                 device=None, likelihood='probit', ep_quadrature=False):
        lik = likelihood_code(likelihood)
        lib = load_library()
        self.lib = lib
        self.ep_quadrature = False
        self.device = _device(device)
        y = _f64(y)
        self.n = y.shape[0]
        if kernel_kind == KERNEL_PRECOMPUTED:
            Xp, d, ldx = None, 0, 0
        else:
            Xp = _f64(X)
            d, ldx = Xp.shape[1], Xp.shape[1]
        self.d = d
        self.kind = kernel_kind
        self.n_imp = int(n_imp)
        self.max_batch = int(max_batch)
        self._h = lib.apm_create(self.device, kernel_kind, _ptr(Xp), self.n, d, ldx, _ptr(y),
                                 float(epsilon), self.n_imp, self.max_batch, int(n_slots),
                                 int(n_ubufs))
        if not self._h:
            raise NativeError('apm_create failed: ' +
                              (lib.apm_global_error() or b'').decode(errors='replace'))
        self.likelihood = likelihood
        if lik != LIK_PROBIT:  # (the library's default)
            _check(lib.apm_set_likelihood(self._h, lik), self._h)
        if ep_quadrature:
            self.set_ep_quadrature(True)
        self.slots = _SlotPool(self)
        self.ubufs = _Pool(int(n_ubufs))
        # calls per batch size (bench.py reports the timed region's; launch shapes depend on it)
        self.batch_hist = {'u': collections.Counter(), 'theta': collections.Counter()}
        self.theta_len = int(lib.apm_theta_len(self._h))
        self.padded_n = int(lib.apm_padded_n(self._h))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.apm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream_ptr(self):
        return self.lib.apm_stream(self._h)

    def set_newton(self, tol, max_iters):
        _check(self.lib.apm_set_newton(self._h, float(tol), int(max_iters)), self._h)

    # --- U buffers
    def u_upload(self, ubuf, U):
        U = _f64(U)
        if U.shape != (self.n, self.n_imp):
            raise ValueError('u has shape {0}, expected {1}'.format(U.shape, (self.n, self.n_imp)))
        _check(self.lib.apm_u_upload(self._h, ubuf, _ptr(U), U.shape[1]), self._h)

    def u_download(self, ubuf):
        U = np.empty((self.n, self.n_imp))
        _check(self.lib.apm_u_download(self._h, ubuf, _ptr(U), self.n_imp), self._h)
        return U

    def u_normal(self, ubufs, seeds, counters):
        ub = np.ascontiguousarray(ubufs, dtype=np.int64)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        ct = np.ascontiguousarray(counters, dtype=np.uint64)
        _check(self.lib.apm_u_normal(self._h, ub.shape[0], _ptr(ub), _ptr(sd), _ptr(ct)), self._h)

    def u_combine(self, dst, a, b, ca, cb):
        dst, a, b = (np.ascontiguousarray(x, dtype=np.int64) for x in (dst, a, b))
        ca, cb = _f64(ca), _f64(cb)
        _check(self.lib.apm_u_combine(self._h, dst.shape[0], _ptr(dst), _ptr(a), _ptr(b), _ptr(ca),
                                      _ptr(cb)), self._h)

    # --- estimator calls
    def theta_eval(self, est, thetas, ubufs=None, slots=None):
        th = self._thetas(thetas, self.batch_hist['theta'])
        count = th.shape[0]
        out = np.full(count, np.nan)
        st = np.zeros(count, dtype=np.int32)
        nops = np.zeros(count, dtype=np.int64)
        ub = None if ubufs is None else np.ascontiguousarray(ubufs, dtype=np.int64)
        sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.int64)
        _check(self.lib.apm_theta_eval(self._h, est, count, _ptr(th), th.shape[1], _ptr(ub),
                                       _ptr(sl), _ptr(out), _ptr(st), _ptr(nops)), self._h)
        return out, st, nops

    def theta_eval_K(self, est, K, ubuf, slot):
        K = _f64(K)
        out = np.full(1, np.nan)
        st = np.zeros(1, dtype=np.int32)
        nops = np.zeros(1, dtype=np.int64)
        _check(self.lib.apm_theta_eval_K(self._h, est, _ptr(K), K.shape[1], int(ubuf), int(slot),
                                         _ptr(out), _ptr(st), _ptr(nops)), self._h)
        return out, st, nops

    def _thetas(self, thetas, hist=None):
        th = np.atleast_2d(_f64(thetas))
        if hist is not None:  # (a call is counted before its thetas are checked)
            hist[th.shape[0]] += 1
        if th.shape[1] < self.theta_len:
            # kernels.pyx indexes theta[k+1] / theta[1] with bounds checking -> IndexError
            raise IndexError('Out of bounds on buffer access (axis 0)')
        return th

    def _test_inputs(self, X_test):
        Xs = _f64(X_test)
        if Xs.ndim != 2 or Xs.shape[1] != self.d:
            raise ValueError('X_test has shape {0}, expected (m, {1})'.format(Xs.shape, self.d))
        return Xs

    def _batched(self, fn, th, trailing, args):
        """One library call per `max_batch` rows of th: NaN-filled float outputs (T,) + shape for
        every shape in `trailing`, int32 statuses and int64 counts (T,). `args(thp, out, st, cnt)`
        lists what follows (handle, count) in fn's argument order, given a batch's offset pointers
        (out: one per float output). Returns ``(*outputs, status, counts)``."""
        T = th.shape[0]
        outs = [np.full((T,) + tuple(shape), np.nan) for shape in trailing]
        st = np.zeros(T, dtype=np.int32)
        cnt = np.zeros(T, dtype=np.int64)
        for t0 in range(0, T, self.max_batch):
            _check(fn(self._h, min(self.max_batch, T - t0),
                      *args(th[t0:].ctypes.data, [o[t0:].ctypes.data for o in outs],
                            st[t0:].ctypes.data, cnt[t0:].ctypes.data)), self._h)
        return tuple(outs) + (st, cnt)

    def _predictive(self, fn, thetas, X_test):
        th, Xs = self._thetas(thetas), self._test_inputs(X_test)
        m = Xs.shape[0]
        return self._batched(fn, th, [(m,)] * 3, lambda thp, o, st, cnt: (
            thp, th.shape[1], _ptr(Xs), m, self.d, o[0], o[1], o[2], m, st, cnt))

    def _gradient(self, fn, thetas):
        th, P = self._thetas(thetas), self.theta_len
        return self._batched(fn, th, [(), (P,)], lambda thp, o, st, cnt: (
            thp, th.shape[1], o[0], o[1], P, st, cnt))

    def predict(self, thetas, X_test):
        """Laplace predictive at X_test (m, d) for every row of thetas, `max_batch` at a time:
        ``(mean, var, prob, status, n_iter)``, the first three (T, m) with NaN rows where
        status != 0 (include/apm.h apm_predict)."""
        return self._predictive(self.lib.apm_predict, thetas, X_test)

    def is_predict(self, est, thetas, ubufs, slots, X_test):
        """Importance-sampling predictive at X_test (m, d) for up to `max_batch` chains: the
        theta-call of :meth:`theta_eval` (`est` EST_IS or EST_IS_EP; the slots are written, log f
        is that call's bitwise) and then the self-normalised average over the importance samples
        of the chains' U buffers: ``(logf, prob, mean, var, ess, status, n_cubic_ops)``, prob /
        mean / var (count, m) and ess (count,) NaN where status != 0 (include/apm.h
        apm_is_predict)."""
        th, Xs = self._thetas(thetas), self._test_inputs(X_test)
        count, m = th.shape[0], Xs.shape[0]
        ub = np.ascontiguousarray(ubufs, dtype=np.int64)
        sl = np.ascontiguousarray(slots, dtype=np.int64)
        if ub.shape != (count,) or sl.shape != (count,):
            raise ValueError('one U buffer and one slot per theta')
        out = np.full(count, np.nan)
        prob, mean, var = (np.full((count, m), np.nan) for _ in range(3))
        ess = np.full(count, np.nan)
        st = np.zeros(count, dtype=np.int32)
        nops = np.zeros(count, dtype=np.int64)
        _check(self.lib.apm_is_predict(
            self._h, est, count, _ptr(th), th.shape[1], _ptr(ub), _ptr(sl), _ptr(Xs), m, self.d,
            _ptr(out), _ptr(prob), _ptr(mean), _ptr(var), m, _ptr(ess), _ptr(st), _ptr(nops)),
            self._h)
        return out, prob, mean, var, ess, st, nops

    def laplace_grad(self, thetas):
        """Laplace log marginal likelihood and its gradient with respect to theta for every row
        of thetas, `max_batch` at a time: ``(lml (T,), grad (T, P), status, n_iter)`` with NaN
        where status != 0 (include/apm.h apm_laplace_grad)."""
        return self._gradient(self.lib.apm_laplace_grad, thetas)

    def set_ep_quadrature(self, on):
        """EP's tilted moments by the quadrature rule (include/apm.h apm_set_ep_quadrature):
        needed for, and only then accepted on, a logit context."""
        _check(self.lib.apm_set_ep_quadrature(self._h, int(bool(on))), self._h)
        self.ep_quadrature = bool(on)

    def set_ep(self, damping=0.8, diff_tol=1e-8, max_sweeps=100, quadrature=None):
        """The EP settings of every later fit on the context. `quadrature` (True / False) is the
        switch of :meth:`set_ep_quadrature`, set first (a logit context is refused without it);
        None leaves the switch as the context has it (off unless ``ep_quadrature=True``)."""
        if quadrature is not None:
            self.set_ep_quadrature(quadrature)
        _check(self.lib.apm_set_ep(self._h, float(damping), float(diff_tol), int(max_sweeps)),
               self._h)

    def ep(self, thetas):
        """Expectation-propagation fit for every row of thetas, `max_batch` at a time:
        ``(logz (T,), mu, var, tau, nu (each (T, n)), status, n_sweeps)`` with NaN where
        status != 0 (include/apm.h apm_ep_eval)."""
        th, n = self._thetas(thetas), self.n
        return self._batched(self.lib.apm_ep_eval, th, [()] + [(n,)] * 4,
                             lambda thp, o, st, cnt: (thp, th.shape[1]) + tuple(o) + (n, st, cnt))

    def ep_predict(self, thetas, X_test):
        """EP predictive at X_test (m, d) for every row of thetas, `max_batch` at a time:
        ``(mean, var, prob, status, n_sweeps)``, the first three (T, m) with NaN rows where
        status != 0 (include/apm.h apm_ep_predict)."""
        return self._predictive(self.lib.apm_ep_predict, thetas, X_test)

    def predict_joint(self, approx, thetas, X_test, want_cov=True, n_draws=0, seeds=None,
                      counters=None, want_draws=False, y_test=None):
        """Joint Laplace (`approx` JOINT_LAPLACE) or EP (JOINT_EP) predictive at the block X_test
        (m <= padded n, d) for every row of thetas, `max_batch` at a time: ``(mean (T, m), cov
        (T, m, m), draws (T, n_draws, m), joint_lpd (T,), status, n_iter)``, NaN where status != 0
        (include/apm.h apm_predict_joint). cov is None unless `want_cov`, draws unless
        `want_draws`, joint_lpd unless labels `y_test` (m,) are given; the last two need
        `n_draws` > 0 and one Philox seed per theta (`counters` default to 0)."""
        th, Xs = self._thetas(thetas), self._test_inputs(X_test)
        T, m, S = th.shape[0], Xs.shape[0], int(n_draws)
        sampled = want_draws or y_test is not None
        sd = ct = ys = None
        if sampled:
            if seeds is None:
                raise ValueError('draws need one Philox seed per theta')
            sd = np.ascontiguousarray(np.atleast_1d(seeds), dtype=np.uint64)
            ct = (np.zeros(T, dtype=np.uint64) if counters is None
                  else np.ascontiguousarray(np.atleast_1d(counters), dtype=np.uint64))
            if sd.shape != (T,) or ct.shape != (T,):
                raise ValueError('one seed and one counter per theta')
        if y_test is not None:
            ys = _f64(y_test)
            if ys.shape != (m,):
                raise ValueError('y_test has shape {0}, expected ({1},)'.format(ys.shape, m))
        mean = np.full((T, m), np.nan)
        cov = np.full((T, m, m), np.nan) if want_cov else None
        draws = np.full((T, S, m), np.nan) if want_draws else None
        lpd = np.full(T, np.nan) if ys is not None else None
        st = np.zeros(T, dtype=np.int32)
        cnt = np.zeros(T, dtype=np.int64)
        off = lambda a, t0: a[t0:].ctypes.data if a is not None else None
        for t0 in range(0, T, self.max_batch):
            _check(self.lib.apm_predict_joint(
                self._h, int(approx), min(self.max_batch, T - t0), off(th, t0), th.shape[1],
                _ptr(Xs), m, self.d, off(mean, t0), m, off(cov, t0), m, S, off(sd, t0),
                off(ct, t0), off(draws, t0), _ptr(ys), off(lpd, t0), off(st, t0), off(cnt, t0)),
                self._h)
        return mean, cov, draws, lpd, st, cnt

    def ep_grad(self, thetas):
        """log Z_EP and its gradient with respect to theta for every row of thetas, `max_batch`
        at a time: ``(logz (T,), grad (T, P), status, n_sweeps)`` with NaN where status != 0
        (include/apm.h apm_ep_grad)."""
        return self._gradient(self.lib.apm_ep_grad, thetas)

    def u_eval(self, slots, ubufs):
        sl = np.ascontiguousarray(slots, dtype=np.int64)
        self.batch_hist['u'][sl.shape[0]] += 1
        ub = np.ascontiguousarray(ubufs, dtype=np.int64)
        out = np.full(sl.shape[0], np.nan)
        st = np.zeros(sl.shape[0], dtype=np.int32)
        _check(self.lib.apm_u_eval(self._h, sl.shape[0], _ptr(sl), _ptr(ub), _ptr(out), _ptr(st)),
               self._h)
        return out, st

    def _diag_args(self, slots, ubufs, n_rep, block):
        """The checks of u_eval_diag / is_spread, made before the library is called:
        ``(slots, ubufs, block, nblk)``."""
        sl = np.ascontiguousarray(slots, dtype=np.int64)
        ub = np.ascontiguousarray(ubufs, dtype=np.int64)
        if sl.ndim != 1 or ub.shape != sl.shape or not 1 <= sl.shape[0] <= self.max_batch:
            raise ValueError('one U buffer per slot, between 1 and max_batch = {0} chains'
                             .format(self.max_batch))
        block = self.n_imp if block is None else int(block)
        if not 1 <= block <= self.n_imp:
            raise ValueError('block = {0} outside [1, n_imp = {1}]'.format(block, self.n_imp))
        n_rep = int(n_rep)
        if n_rep < 1:
            raise ValueError('n_rep = {0} < 1'.format(n_rep))
        nblk = self.n_imp // block
        if n_rep * nblk > SPREAD_MAX_BLOCKS:
            raise ValueError('n_rep * nblk = {0} above {1} (APM_SPREAD_MAX_BLOCKS): split the '
                             'replicates over several calls'.format(n_rep * nblk,
                                                                    SPREAD_MAX_BLOCKS))
        return sl, ub, block, nblk

    def u_eval_diag(self, slots, ubufs, block=None):
        """The cached u-call of :meth:`u_eval` cut into blocks of `block` samples (None: n_imp,
        one block): ``(logf, ess, wmax, status)``, the first three (count, n_imp // block) - each
        block's estimate, weight ESS and largest normalised weight (include/apm.h
        apm_u_eval_diag). With one block, logf is u_eval's value bitwise."""
        sl, ub, block, nblk = self._diag_args(slots, ubufs, 1, block)
        count = sl.shape[0]
        logf, ess, wmax = (np.full((count, nblk), np.nan) for _ in range(3))
        st = np.zeros(count, dtype=np.int32)
        _check(self.lib.apm_u_eval_diag(self._h, count, _ptr(sl), _ptr(ub), block, _ptr(logf),
                                        _ptr(ess), _ptr(wmax), nblk, _ptr(st)), self._h)
        return logf, ess, wmax, st

    def is_spread(self, slots, ubufs, seeds, counters, n_rep, block=None):
        """`n_rep` independent replicates of the estimate at the slots' fixed state: replicate r
        redraws U buffer ubufs[i] from the Philox stream (seeds[i], counters[i] + r), as
        :meth:`u_normal` draws it, and evaluates it in blocks of `block` samples (None: n_imp):
        ``(logf, ess, wmax, status)``, the first three (count, n_rep, n_imp // block). The U
        buffers are scratch (they end holding the last replicate's draws); the slots are only
        read (include/apm.h apm_is_spread)."""
        sl, ub, block, nblk = self._diag_args(slots, ubufs, n_rep, block)
        n_rep = int(n_rep)
        count = sl.shape[0]
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        ct = np.ascontiguousarray(counters, dtype=np.uint64)
        if sd.shape != (count,) or ct.shape != (count,):
            raise ValueError('one seed and one counter per chain')
        logf, ess, wmax = (np.full((count, n_rep, nblk), np.nan) for _ in range(3))
        st = np.zeros(count, dtype=np.int32)
        _check(self.lib.apm_is_spread(self._h, count, _ptr(sl), _ptr(ub), _ptr(sd), _ptr(ct),
                                      n_rep, block, _ptr(logf), _ptr(ess), _ptr(wmax),
                                      n_rep * nblk, _ptr(st)), self._h)
        return logf, ess, wmax, st

    def is_loo(self, slots, ubufs):
        """Leave-one-out predictive densities at the training points from the importance samples
        of the cached u-call of :meth:`u_eval`: ``(logf, loo, lpd, ess_loo, gauss, ess, status)``,
        logf (u_eval's value bitwise) and ess (count,), the others (count, n): the exact
        ``log p(y_i | y_-i, theta)`` estimate, the in-sample density, the ESS of the LOO ratio and
        the Gaussian (cavity) LOO of the slot's approximation; NaN for a chain whose slot's last
        theta-call failed (include/apm.h apm_is_loo). Slots and U buffers are only read."""
        sl = np.ascontiguousarray(slots, dtype=np.int64)
        ub = np.ascontiguousarray(ubufs, dtype=np.int64)
        if sl.ndim != 1 or ub.shape != sl.shape or not 1 <= sl.shape[0] <= self.max_batch:
            raise ValueError('one U buffer per slot, between 1 and max_batch = {0} chains'
                             .format(self.max_batch))
        count, n = sl.shape[0], self.n
        logf, ess = np.full(count, np.nan), np.full(count, np.nan)
        loo, lpd, ess_loo, gauss = (np.full((count, n), np.nan) for _ in range(4))
        st = np.zeros(count, dtype=np.int32)
        _check(self.lib.apm_is_loo(self._h, count, _ptr(sl), _ptr(ub), _ptr(logf), _ptr(loo),
                                   _ptr(lpd), _ptr(ess_loo), _ptr(gauss), n, _ptr(ess), _ptr(st)),
               self._h)
        return logf, loo, lpd, ess_loo, gauss, ess, st

    def is_loo_psis(self, slots, ubufs, want_logratio=False):
        """Pareto-smoothed leave-one-out densities and the Pareto shape k-hat of the importance
        ratios' upper tails, from the importance samples of the cached u-call of :meth:`u_eval`:
        ``(logf, loo_psis, khat, khat_w, logratio, status)``, logf (u_eval's value bitwise) and
        khat_w (the tail shape of the weights themselves) (count,), loo_psis and khat (count, n);
        khat is NaN where the tail is too short to fit (fewer than 25 samples) or degenerate, and
        loo_psis is then the raw value. With `want_logratio` the log ratios ``log wbar_s - log
        p(y_i | f_si)`` come back as (count, n, n_imp), else None. NaN for a chain whose slot's
        last theta-call failed (include/apm.h apm_is_loo_psis). Slots and U buffers are only
        read."""
        sl = np.ascontiguousarray(slots, dtype=np.int64)
        ub = np.ascontiguousarray(ubufs, dtype=np.int64)
        if sl.ndim != 1 or ub.shape != sl.shape or not 1 <= sl.shape[0] <= self.max_batch:
            raise ValueError('one U buffer per slot, between 1 and max_batch = {0} chains'
                             .format(self.max_batch))
        if self.n_imp > PSIS_MAX_SAMPLES:
            raise ValueError('n_imp = {0} above {1} (APM_PSIS_MAX_SAMPLES)'
                             .format(self.n_imp, PSIS_MAX_SAMPLES))
        count, n = sl.shape[0], self.n
        logf, khat_w = np.full(count, np.nan), np.full(count, np.nan)
        loo_psis, khat = np.full((count, n), np.nan), np.full((count, n), np.nan)
        lr = np.full((count, n, self.n_imp), np.nan) if want_logratio else None
        st = np.zeros(count, dtype=np.int32)
        _check(self.lib.apm_is_loo_psis(self._h, count, _ptr(sl), _ptr(ub), _ptr(logf),
                                        _ptr(loo_psis), _ptr(khat), n, _ptr(khat_w), _ptr(lr),
                                        n * self.n_imp, _ptr(st)), self._h)
        return logf, loo_psis, khat, khat_w, lr, st

    def slot_read(self, slot):
        L = np.zeros((self.n, self.n))
        f = np.zeros(self.n)
        g = np.zeros(self.n)
        c = np.zeros(1)
        _check(self.lib.apm_slot_read(self._h, int(slot), _ptr(L), self.n, _ptr(f), _ptr(g),
                                      _ptr(c)), self._h)
        return L, f, g, float(c[0])

    def guard_read(self, count):
        """(count, 4) residuals r1..r4 of the last IS theta-call's guard (include/apm.h)."""
        r = np.zeros((int(count), 4))
        _check(self.lib.apm_guard_read(self._h, int(count), _ptr(r)), self._h)
        return r

    # --- profiling
    def prof_enable(self, on=True):
        """on: False/0 off, True/1 the roofline kinds, 2 every kind (apm.h)."""
        _check(self.lib.apm_prof_enable(self._h, int(on)), self._h)

    def prof_marker(self, marker_id):
        _check(self.lib.apm_prof_marker(self._h, int(marker_id)), self._h)

    def prof_read(self, kind, reset=False):
        ms = np.zeros(1)
        cnt = np.zeros(1, dtype=np.int64)
        wk = np.zeros(1)
        _check(self.lib.apm_prof_read(self._h, kind, _ptr(ms), _ptr(cnt), _ptr(wk), int(reset)),
               self._h)
        return float(ms[0]), int(cnt[0]), float(wk[0])
