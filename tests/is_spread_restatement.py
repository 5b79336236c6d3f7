"""float64 numpy restatement of the block quantities of apm_u_eval_diag / apm_is_spread
(DESIGN.md §20), shared by test_is_spread_host.py and test_gpu_is_spread.py. A plain module.

log w_s is epis_restatement.is_consistent's summand (the consistent form of DESIGN.md §3.2, any
state with f, W, a, C_chol and logdet_B), or the prior-MC one; the S samples are cut into
nblk = S // B blocks of B, leftover samples ignored."""
import numpy as np
from scipy.special import log_ndtr, logsumexp


def log_weights(y, st, ns, log_lik=log_ndtr):
    """log w_s of every column of ns, as is_consistent forms it before its log-mean-exp."""
    f_post, W = st['f'], st['W']
    z = st['a'] + W * f_post
    f_s = f_post[:, None] + st['C_chol'].dot(ns)
    t = log_lik(y[:, None] * f_s) + (0.5 * W[:, None] * f_s - z[:, None]) * f_s
    return t.sum(0) + 0.5 * f_post.dot(z) - 0.5 * st['logdet_B']


def log_weights_priormc(y, K_chol, ns, log_lik=log_ndtr):
    """log p(y | f_s) at f_s = L_K u_s: the prior-MC estimator's summand."""
    return log_lik(y[:, None] * K_chol.dot(ns)).sum(0)


def blocks(lw, B):
    """(logf, ess, wmax), each (S // B,), of the log weights lw (S,) in blocks of B."""
    lw = np.asarray(lw, dtype=np.float64)
    nblk = lw.shape[0] // B
    v = lw[:nblk * B].reshape(nblk, B)
    mx = v.max(1)
    ok = np.isfinite(mx)
    with np.errstate(invalid='ignore'):
        w = np.exp(v - np.where(ok, mx, 0.0)[:, None])
    sw = w.sum(1)
    logf = np.where(ok, mx + np.log(np.where(ok, sw, 1.0)), mx) - np.log(B)
    ess = np.where(ok, sw ** 2 / np.where(ok, (w ** 2).sum(1), 1.0), 0.0)
    wmax = np.where(ok, w.max(1) / np.where(ok, sw, 1.0), 0.0)
    return logf, ess, wmax


def log_mean_exp(x):
    x = np.asarray(x, dtype=np.float64)
    return logsumexp(x) - np.log(x.size)


def delta_sd(ess, B):
    """The one-call delta-method figure for the sd of a block estimate: sqrt(mean(1/ess - 1/B))."""
    ess = np.asarray(ess, dtype=np.float64)
    return float(np.sqrt(np.mean(1.0 / ess - 1.0 / B)))
