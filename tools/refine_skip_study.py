"""Can the Newton loop skip the fp64 refinement of its early solves?

The IS theta-call's Newton iterations (latent_posterior_approximations.py:85-99) solve
B x = W^1/2 K b with an fp32 factor of B and refine x in fp64 (newton_solve.hip). An early iterate's
solve error is damped by the Newton map's contraction (its derivative vanishes at the mode), so an
unrefined solve there may leave f_post and n_iter unchanged. This study runs the iteration in
float64 with the solves of the iterations the rule marks as unrefined replaced by an fp32 solve
(numpy float32 Cholesky) whose error is also inflated by a relative `--noise` (the device's fp16x3
factor is ~4x less accurate than LAPACK's fp32 one), and reports n_iter and max|f - f_ref| / max|f_ref|
for the rule "refine iteration k iff diff_{k-1} < T" over thetas around the bench's posterior.

    python tools/refine_skip_study.py [--n 2048]
"""
import argparse
import os
import sys

import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))
sys.path.insert(0, os.path.join(REPO, 'oracle'))


def newton(K, y, T, noise, rng):
    f = np.zeros(y.shape[0])
    diffs, prev = [], np.inf
    for i in range(100):
        v = np.exp(-0.5 * f ** 2 - log_ndtr(y * f) - 0.5 * np.log(2 * np.pi))
        g = v * y
        W = v ** 2 + g * f
        s = W ** 0.5
        B = np.eye(len(y)) + s[:, None] * K * s[None, :]
        b = W * f + g
        r = s * K.dot(b)
        if prev < T:  # refined: fp64-accurate solve
            x = la.cho_solve((la.cholesky(B, lower=True), True), r)
        else:
            L32 = la.cholesky(B.astype(np.float32), lower=True)
            x = la.cho_solve((L32, True), r.astype(np.float32)).astype(np.float64)
            x *= 1 + noise * rng.standard_normal(x.shape)
        a = b - s * x
        fn = K.dot(a)
        diff = np.mean((fn - f) ** 2)
        diffs.append(diff)
        prev = diff
        f = fn
        if diff < 1e-4:
            break
    return f, i + 1, diffs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2048)
    ap.add_argument('--noise', type=float, default=1e-5)
    ap.add_argument('--T', type=float, nargs='*', default=[0.0, 0.01, 0.05, 0.2])
    ap.add_argument('--draws', type=int, default=12)
    a = ap.parse_args()
    import apm_oracle as orc
    from gpdemo.utils import synthetic_gp_data
    z = np.load(os.path.join(REPO, 'tests', 'golden', 'config2_ref.npz'))
    X, y = synthetic_gp_data(a.n, 32, int(z['data_seed']))
    kf = orc.make_kernel_func('ard', 1e-8)
    rng = np.random.RandomState(0)
    worst = {T: 0. for T in a.T}
    flips = {T: 0 for T in a.T}
    for q in range(a.draws):
        th = z['thetas'][3][:33].copy()
        th[0] = rng.uniform(1.5, 5.0)
        th[1:] += rng.normal(scale=0.7, size=32)
        K = np.empty((a.n, a.n))
        kf(K, X, th)
        f_ref, n_ref, d_ref = newton(K, y, np.inf, 0., rng)
        line = 'log_sigma %.2f n_iter %d diffs %s |' % (th[0], n_ref, ' '.join('%.0e' % d for d in d_ref))
        for T in a.T:
            f, n, _ = newton(K, y, T, a.noise, rng)
            e = np.abs(f - f_ref).max() / np.abs(f_ref).max()
            worst[T] = max(worst[T], e)
            flips[T] += n != n_ref
            line += ' T=%g: n %d err %.1e' % (T, n, e)
        print(line, flush=True)
    print('worst rel err', worst, 'n_iter flips', flips)


if __name__ == '__main__':
    main()
