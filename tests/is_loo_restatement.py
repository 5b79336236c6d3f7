"""numpy statement of the leave-one-out predictive densities from the importance samples
(apm_is_loo), shared by test_is_loo_host.py and test_gpu_is_loo.py. A plain module.

Inputs are what a cache slot holds: f_post, W, z = C^-1 f_post, the factor C_chol (n x n lower) and
cst = 1/2 f_post^T z - 1/2 log|B|; the labels y, the draws U (n x S) and the likelihood. The log
weights are is_predict_restatement.log_weights', at its `samples` f_s = f_post + C_chol u_s, here
taken with the slot's own factor. Every sum over the samples is a logsumexp, so a padded column
(log wbar = -inf) and a weight that would underflow are treated alike: in log space."""
import numpy as np
from scipy.special import log_ndtr, logsumexp

import is_predict_restatement as ipr
import logit_restatement as lr


def slot_of(fit):
    """(f_post, W, z, C_chol, cst) of a proposal fit with the keys f, W, a, C_chol, logdet_B
    (epis_restatement.state / .laplace_state, logit_restatement.is_state)."""
    f, W = fit['f'], fit['W']
    z = fit['a'] + W * f
    return f, W, z, fit['C_chol'], 0.5 * f.dot(z) - 0.5 * fit['logdet_B']


def log_lik(t, likelihood='probit'):
    return lr.log_lik(t) if likelihood == 'logit' else log_ndtr(t)


def cavity(y, f_post, W, z, cdiag, likelihood='probit', check=True):
    """gauss_i = log int p(y_i | f) N(f | nu / tau, 1 / tau) df with tau = 1 / C_ii - W_i and
    nu = f_post_i / C_ii - z_i: dict(gauss, tau, m, v). tau > 0 holds in exact arithmetic (C < W^-1)
    and is asserted at every point unless check is False (then NaN where it fails)."""
    tau = 1.0 / cdiag - W
    nu = f_post / cdiag - z
    if check:
        assert (tau > 0.0).all(), tau.min()
    with np.errstate(divide='ignore', invalid='ignore'):
        m, v = nu / tau, 1.0 / tau
        if likelihood == 'logit':
            g = np.log(lr.logistic_normal(y * m, np.maximum(v, 0.0)))
        else:
            g = log_ndtr(y * m / np.sqrt(1.0 + v))
    return dict(gauss=np.where(tau > 0.0, g, np.nan), tau=tau, m=m, v=v)


def loo_quantities(y, f_post, W, z, C_chol, cst, U, likelihood='probit', n_real=None,
                   check=True):
    """dict(loo, lpd, ess_loo, gauss (n,), ess, logf, lw (S,), lp (n, S), tau): the section
    'Mathematics' of the feature. The first n_real columns of U (default: all) are the real
    samples; the others are padding with log wbar = -inf."""
    S = U.shape[1] if n_real is None else int(n_real)
    f_s = f_post[:, None] + C_chol.dot(U)
    fit = dict(f=f_post, W=W, a=z - W * f_post, logdet_B=f_post.dot(z) - 2.0 * cst)
    lw = ipr.log_weights(y, fit, f_s, likelihood)
    lwbar = np.where(np.arange(U.shape[1]) < S, lw - logsumexp(lw[:S]), -np.inf)
    lp = log_lik(y[:, None] * f_s, likelihood)
    with np.errstate(invalid='ignore'):
        t = np.where(np.isneginf(lwbar)[None], -np.inf, lwbar[None] - lp)
        tp = np.where(np.isneginf(lwbar)[None], -np.inf, lwbar[None] + lp)
    cav = cavity(y, f_post, W, z, (C_chol * C_chol).sum(1), likelihood, check)
    return dict(loo=-logsumexp(t, axis=1), lpd=logsumexp(tp, axis=1),
                ess_loo=np.exp(2.0 * logsumexp(t, axis=1) - logsumexp(2.0 * t, axis=1)),
                gauss=cav['gauss'], tau=cav['tau'], ess=np.exp(-logsumexp(2.0 * lwbar)),
                logf=logsumexp(lw[:S]) - np.log(S), lw=lw, lp=lp)


def loo_stderr(ess_loo):
    """Standard error of loo_i = -log R_i, R_i = sum_s rho_si, from ess_loo_i by the delta method:
    se(log R) = sd(R) / R, and for a sum of S independent terms sd(R)^2 is estimated by
    sum_s rho_s^2 (its mean-square term; the normaliser of wbar is held fixed), so
    se(loo_i) = sqrt(sum_s rho_si^2) / sum_s rho_si = 1 / sqrt(ess_loo_i)."""
    return 1.0 / np.sqrt(ess_loo)


def loo_stderr_ratio(lw, lp_i):
    """The same with the normaliser's own noise, as is_predict_restatement.prob_stderr takes a
    self-normalised average: with h_s = (1 / p_si) / R_i (whose estimate is 1),
    se(loo_i) = sqrt(sum_s wbar_s^2 (h_s - 1)^2)."""
    lwbar = lw - logsumexp(lw)
    h = np.exp(-lp_i - logsumexp(lwbar - lp_i))
    return float(np.sqrt((np.exp(2.0 * lwbar) * (h - 1.0) ** 2).sum()))
