"""numpy/scipy restatement of the joint Laplace / EP predictive at test inputs (DESIGN.md §31;
apm_predict_joint), shared by test_joint_predict_host.py and test_gpu_joint_predict.py. A plain
module, on top of cov_restatement.py (its Cov: K, k*, k** of a kind) and the Laplace and EP restatements
(the fit's last state L, W^1/2 or S^1/2, a).

    mean  = k* a
    Sigma = K**(Xs, Xs) - V^T V,   V = L^-1 (W^1/2 . k*^T)            (n, m)
    L_S   = chol(Sigma + eps I)
    f_r   = mean + L_S xi_r,       xi (m, n_draws) the normal stream in row-major order
    lpd   = logsumexp_r sum_j log p(ys_j | f_rj) - log n_draws

K** is the cross-Gram of the test inputs with themselves (no epsilon) with k** on its diagonal.
The second version (``*_ld``) repeats everything after the fit in ``np.longdouble`` with
hand-written triangular solves and Cholesky, as the yardstick of the fp64 version's rounding:
the tests bound the device's distance to the fp64 version by a multiple of the distance between
the two. The fit's state and the Gram matrices are the same fp64 numbers in both, and so is the
log-likelihood, which numpy has in fp64 only: it is evaluated at the long-double f rounded to fp64,
and summed in long double."""
import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr, logsumexp

import ep_quad_restatement as eq
import ep_restatement as ep
import grad_restatement as gr
import logit_restatement as lr

PROBIT, LOGIT = 'probit', 'logit'
LD = np.longdouble


def log_lik(lik, t):
    return lr.log_lik(t) if lik == LOGIT else log_ndtr(t)


def gram_test(cov, Xs, theta):
    """K**(Xs, Xs): the kind's covariance between the test points, bias and linear terms
    included, no epsilon, the prior variance k** on the diagonal."""
    Kss = cov.gram_cross(Xs, Xs, theta)
    Kss[np.diag_indices_from(Kss)] = cov.prior_var(Xs, theta)
    return Kss


def laplace_state(cov, X, y, theta, eps, tol=1e-4, max_iters=1000, lik=PROBIT):
    """dict(L, Ws, a, n_iter, diffs) of the Newton loop's last iteration."""
    nw = gr.newton(cov.gram(X, theta, eps), y, tol, max_iters,
                   lr.LOGIT if lik == LOGIT else gr.PROBIT)
    return dict(L=nw['L'], Ws=nw['Ws'], a=nw['a'], n_iter=nw['n_iter'], diffs=nw['diffs'])


def ep_state(cov, X, y, theta, eps, lik=PROBIT, quadrature=False, **ep_settings):
    """dict(L, Ws (S^1/2), a, n_iter (sweeps), diffs (the stop measure's history)) of the sweep
    the EP fit stopped at; the tilted moments in closed form (probit) or by the quadrature rule."""
    K = cov.gram(X, theta, eps)
    if quadrature or lik == LOGIT:
        fit = eq.ep_fit(K, y, lik=eq.LOGIT if lik == LOGIT else eq.PROBIT, **ep_settings)
    else:
        fit = ep.ep_fit(K, y, **ep_settings)
    return dict(L=fit['L'], Ws=fit['s'], a=fit['a'], n_iter=fit['n_sweeps'], diffs=fit['m_hist'])


def joint(Kss, Ks, st):
    """(mean (m,), Sigma (m, m)) at the rows of Ks (m, n) from a fit's state."""
    V = la.solve_triangular(st['L'], (Ks * st['Ws'][None, :]).T, lower=True)
    return Ks.dot(st['a']), Kss - V.T.dot(V)


def factor(Sigma, eps):
    return la.cholesky(Sigma + eps * np.eye(Sigma.shape[0]), lower=True)


def draws(mean, Sigma, eps, xi):
    """(n_draws, m): mean + L_S xi_r for the columns of xi (m, n_draws)."""
    return mean[None, :] + factor(Sigma, eps).dot(xi).T


def joint_lpd(f, ys, lik=PROBIT):
    return float(logsumexp(log_lik(lik, ys[None, :] * f).sum(1)) - np.log(f.shape[0]))


def at_test_inputs(cov, X, Xs, theta, st, eps, xi=None, ys=None, lik=PROBIT):
    """dict(mean, cov[, draws][, lpd]) of one theta from the fit's state."""
    mean, Sigma = joint(gram_test(cov, Xs, theta), cov.gram_cross(Xs, X, theta), st)
    out = dict(mean=mean, cov=Sigma)
    if xi is not None:
        out['draws'] = draws(mean, Sigma, eps, xi)
        if ys is not None:
            out['lpd'] = joint_lpd(out['draws'], ys, lik)
    return out


# ---- the same in long double --------------------------------------------------------------------

def solve_lower_ld(L, B):
    """L^-1 B by forward substitution, one row at a time, in long double."""
    L, X = np.asarray(L, dtype=LD), np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        if i:
            X[i] -= L[i, :i].dot(X[:i])
        X[i] /= L[i, i]
    return X


def cholesky_ld(A):
    """The lower Cholesky factor column by column, in long double."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        p = A[j, j] - L[j, :j].dot(L[j, :j])
        if not p > 0:
            raise np.linalg.LinAlgError('pivot {0} not positive'.format(j))
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def at_test_inputs_ld(cov, X, Xs, theta, st, eps, xi=None, ys=None, lik=PROBIT):
    """at_test_inputs with everything behind the fit's state and the Gram matrices in long
    double; the outputs stay long double."""
    Kss = gram_test(cov, Xs, theta).astype(LD)
    Ks = cov.gram_cross(Xs, X, theta).astype(LD)
    Ws, a = st['Ws'].astype(LD), st['a'].astype(LD)
    V = solve_lower_ld(st['L'], (Ks * Ws[None, :]).T)
    mean, Sigma = Ks.dot(a), Kss - V.T.dot(V)
    out = dict(mean=mean, cov=Sigma)
    if xi is not None:
        Ls = cholesky_ld(Sigma + LD(eps) * np.eye(Sigma.shape[0], dtype=LD))
        f = mean[None, :] + Ls.dot(xi.astype(LD)).T
        out['draws'] = f
        if ys is not None:
            lp = log_lik(lik, ys[None, :] * f.astype(np.float64)).astype(LD).sum(1)
            top = lp.max()
            out['lpd'] = top + np.log(np.exp(lp - top).sum()) - np.log(LD(f.shape[0]))
    return out


def gap(ref, ref_ld, key):
    """max |fp64 - long double| of one output of the two versions."""
    return float(np.max(np.abs(np.asarray(ref[key], dtype=LD) - ref_ld[key])))
