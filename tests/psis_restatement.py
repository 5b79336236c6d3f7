"""numpy statement of the Pareto-smoothed leave-one-out densities and the Pareto k-hat of the
importance ratios (apm_is_loo_psis), shared by test_psis_host.py and
test_gpu_psis.py. A plain module: steps 1-6 of include/apm.h on one row of log ratios.

`tail_shift` and `drop_prior` are the two mutations the GPU parity test must catch (M off by one,
the prior term of khat dropped); they are 0 / False everywhere else."""
import numpy as np
from scipy.special import logsumexp

LOG_DBL_MIN = float(np.log(np.finfo(np.float64).tiny))


def tail_size(n_finite):
    """M = min(floor(0.2 S'), ceil(3 sqrt(S'))), in integers."""
    s = int(n_finite)
    c = int(np.ceil(3.0 * np.sqrt(s)))
    while c > 0 and (c - 1) * (c - 1) >= 9 * s:
        c -= 1
    while c * c < 9 * s:
        c += 1
    return min(s // 5, c)


def gpd_fit(x, drop_prior=False):
    """(khat, sigma) of the generalised Pareto distribution fitted to the ascending excesses x
    (Zhang & Stephens 2009; the `loo` package's prior_bs = 3 and prior_k = 10)."""
    M = x.shape[0]
    m = 30 + int(np.floor(np.sqrt(M)))
    q = x[int(np.floor(M / 4.0 + 0.5)) - 1]
    j = np.arange(1, m + 1)
    with np.errstate(all='ignore'):
        b = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * q)
        k = np.log1p(-b[:, None] * x[None]).mean(1)
        L = M * (np.log(-b / k) - k - 1.0)
        omega = 1.0 / np.exp(L[None] - L[:, None]).sum(1)
        bh = (b * omega).sum()
        kh = np.log1p(-bh * x).mean()
        sigma = -kh / bh
    khat = kh if drop_prior else (M * kh + 5.0) / (M + 10.0)
    return float(khat), float(sigma)


def psis_row(t, tail_shift=0, drop_prior=False):
    """(loo_psis, khat, M) of one row of log ratios t; -inf entries have no ratio."""
    t = np.asarray(t, dtype=np.float64)
    t = t[~np.isneginf(t)]
    Sf = t.shape[0]
    M = tail_size(Sf)
    mx = t.max() if Sf else -np.inf
    raw = -(mx + logsumexp(t - mx)) if Sf else np.inf
    if M < 5:
        return raw, np.nan, M
    M += tail_shift
    ts = np.sort(t - mx)
    ec = np.exp(max(ts[Sf - M - 1], LOG_DBL_MIN))
    x = np.exp(ts[Sf - M:]) - ec
    if x[0] <= 0.0 or x[-1] <= x[0]:
        return raw, np.nan, M
    khat, sigma = gpd_fit(x, drop_prior)
    if not (np.isfinite(khat) and np.isfinite(sigma)):
        return raw, khat, M
    l1 = np.log1p(-(np.arange(1, M + 1) - 0.5) / M)
    q = -sigma * l1 if khat == 0.0 else sigma * np.expm1(-khat * l1) / khat
    r = np.minimum(q + ec, 1.0)
    return -(mx + np.log(np.exp(ts[:Sf - M]).sum() + r.sum())), khat, M


def psis_rows(t, **kw):
    """(loo_psis, khat) over the rows of t (n, S)."""
    out = [psis_row(row, **kw) for row in t]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])
