"""What test_gpu_matern.py, test_gpu_bias.py and test_gpu_linear.py share beside the restatements:
the test inputs of their predictive checks and the conditions they put on the references alone
(stop margins, the oracle's own sensitivity to rounding in K) before a device result is compared.
A plain module."""
import numpy as np

import apm_oracle as orc
import cov_restatement as cr
import grad_restatement as gr


def far_test_inputs(c, m, far):
    """Normal rows; row 0 coincides with a training point and the last row is `far` away in every
    coordinate, so that S* underflows to exactly 0 (SE: 50; the Matern kinds decay exponentially
    only and need 1000)."""
    rng = np.random.RandomState(1000 + c['n'])
    Xs = rng.normal(size=(m, c['d']))
    Xs[0] = c['X'][7 % c['n']]
    Xs[-1] = c['X'][3 % c['n']] + far
    return Xs


def oracle_moves(X, y, ns, K, seed=1):
    """|change| of the oracle's IS log-estimate under 1-ulp symmetric relative noise in K."""
    def fixed(Kx):
        def fn(Kw, X_, theta_):
            Kw[...] = Kx
        return fn
    th = np.zeros(1)
    v0, _, _ = orc.is_estimate(X, y, fixed(K), ns, th)
    v1, _, _ = orc.is_estimate(X, y, fixed(cr.symmetric_ulp_noise(K, seed)), ns, th)
    return abs(v1 - v0)


def newton_margins(K, y, tol, grad_tol, n=2):
    """The restatement's Newton loop cannot stop one iteration away from the device's: a factor
    100 on both sides of the gradient's tolerance `grad_tol` (n = 1: 1.5 above), a factor 3 on
    both sides of any other."""
    df = gr.newton(K, y, tol)['diffs']
    if tol == grad_tol:
        assert df[-1] <= tol / 100.0 and df[-2] >= (1.5 if n == 1 else 100.0) * tol, df[-2:]
    else:
        assert df[-1] <= tol / 3.0 and (len(df) < 2 or df[-2] >= 3.0 * tol), df[-2:]


def ep_margins(fit):
    m = fit['m_hist']
    assert m[-1] < 0.99e-8 and (len(m) < 2 or m[-2] > 1.01e-8), m[-2:]


def worst(dev, ref):
    """The largest error of a device (mean, var, prob): mean and var relative to
    max(1, max|ref|), prob absolute."""
    out = 0.0
    for key, d in zip(('mean', 'var', 'prob'), dev):
        scale = 1.0 if key == 'prob' else max(1.0, np.abs(ref[key]).max())
        out = max(out, np.abs(d - ref[key]).max() / scale)
    return out
