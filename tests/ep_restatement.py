"""numpy/scipy statement of parallel expectation propagation for the probit GP classifier
(apm_ep_eval / apm_ep_predict / apm_ep), shared by test_ep_host.py and
test_gpu_ep.py. A plain module: the normative algorithm the device code is compared with, the
predictive from the EP state, and sequential EP (Rasmussen & Williams Alg. 3.5) as an
independent route to the same fixed point."""
import numpy as np
import scipy.linalg as la
from scipy.special import log_ndtr, ndtr

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


class InvalidCavity(Exception):
    """A cavity precision was <= 0 or not finite (APM_STATUS_EP_CAVITY)."""


class NotConverged(Exception):
    """The stop rule was not met after max_sweeps sweeps (APM_STATUS_MAXITER)."""


def posterior(K, tau, nu):
    """Gaussian posterior from the sites: S^1/2, L = chol(I + S^1/2 K S^1/2), a, mu = K a and the
    marginal variances K_ii - sum_r V_ri^2 with V = L^-1 (S^1/2 K)."""
    n = tau.shape[0]
    s = np.sqrt(tau)
    L = la.cholesky(np.eye(n) + s[:, None] * K * s[None, :], lower=True)
    a = nu - s * la.cho_solve((L, True), s * K.dot(nu))
    mu = K.dot(a)
    V = la.solve_triangular(L, s[:, None] * K, lower=True)
    var = np.diag(K) - (V * V).sum(0)
    return s, L, a, mu, var


def tilted(y, mu_c, var_c):
    """z, r = phi(z)/Phi(z), and the tilted mean and variance of Phi(y f) N(f | mu_c, var_c)."""
    den = 1.0 + var_c
    z = y * mu_c / np.sqrt(den)
    r = np.exp(-0.5 * z * z - log_ndtr(z) - HALF_LOG_2PI)
    mu_h = mu_c + y * var_c * r / np.sqrt(den)
    var_h = var_c - var_c * var_c * r * (z + r) / den
    return z, r, mu_h, var_h


def ep_fit(K, y, damping=0.8, diff_tol=1e-8, max_sweeps=100):
    """Parallel EP. Returns the state of the converged sweep: logz, mu, var, tau, nu, a, L, s,
    n_sweeps, and m_hist (the stop measure of sweeps 2, 3, ...)."""
    n = y.shape[0]
    tau, nu = np.zeros(n), np.zeros(n)
    mu_prev, m_hist = None, []
    for t in range(1, int(max_sweeps) + 1):
        s, L, a, mu, var = posterior(K, tau, nu)
        with np.errstate(divide='ignore', invalid='ignore'):
            tau_c = 1.0 / var - tau
            nu_c = mu / var - nu
        if not np.all(np.isfinite(tau_c) & (tau_c > 0.0)):
            raise InvalidCavity('sweep {0}'.format(t))
        mu_c, var_c = nu_c / tau_c, 1.0 / tau_c
        z, r, mu_h, var_h = tilted(y, mu_c, var_c)
        if t >= 2:
            m = np.mean((mu - mu_prev) ** 2)
            m_hist.append(m)
            if m < diff_tol:
                rows = (log_ndtr(z) + 0.5 * np.log1p(tau / tau_c) + 0.5 * nu * mu
                        - 0.5 * nu * nu * var
                        + 0.5 * mu_c * tau_c * (tau * mu_c - 2.0 * nu) * var)
                logz = rows.sum() - np.log(np.diag(L)).sum()
                return dict(logz=logz, mu=mu, var=var, tau=tau, nu=nu, a=a, L=L, s=s,
                            n_sweeps=t, m_hist=m_hist)
        tau_new = np.maximum(1.0 / var_h - tau_c, 0.0)
        nu_new = mu_h / var_h - nu_c
        tau = (1.0 - damping) * tau + damping * tau_new
        nu = (1.0 - damping) * nu + damping * nu_new
        mu_prev = mu
    raise NotConverged('{0} sweeps'.format(max_sweeps))


def at_test_inputs(Ks, sigma, fit):
    """mean = Ks a, var = sigma - |L^-1 (S^1/2 . ks)|^2 and prob = Phi(mean / sqrt(1 + var)) at
    the rows of Ks from an EP state."""
    mu = Ks.dot(fit['a'])
    V = la.solve_triangular(fit['L'], (Ks * fit['s'][None, :]).T, lower=True)
    var = sigma - (V * V).sum(0)
    return dict(mean=mu, var=var, prob=ndtr(mu / np.sqrt(1.0 + var)))


def ep_sequential(K, y, n_sweeps=200, tol=1e-13):
    """Sequential EP (R&W Alg. 3.5): one site at a time with rank-one updates of Sigma, the
    posterior recomputed from the sites after every sweep. Stops when no site precision moved by
    more than tol in a sweep. Returns tau, nu, mu."""
    n = y.shape[0]
    tau, nu = np.zeros(n), np.zeros(n)
    Sigma, mu = K.copy(), np.zeros(n)
    for _ in range(n_sweeps):
        tau_old = tau.copy()
        for i in range(n):
            tau_c = 1.0 / Sigma[i, i] - tau[i]
            nu_c = mu[i] / Sigma[i, i] - nu[i]
            _, _, mu_h, var_h = tilted(y[i], nu_c / tau_c, 1.0 / tau_c)
            dtau = 1.0 / var_h - tau_c - tau[i]
            tau[i] += dtau
            nu[i] = mu_h / var_h - nu_c
            si = Sigma[:, i].copy()
            Sigma -= (dtau / (1.0 + dtau * si[i])) * np.outer(si, si)
            mu = Sigma.dot(nu)
        s = np.sqrt(tau)
        L = la.cholesky(np.eye(n) + s[:, None] * K * s[None, :], lower=True)
        V = la.solve_triangular(L, s[:, None] * K, lower=True)
        Sigma = K - V.T.dot(V)
        mu = Sigma.dot(nu)
        if np.max(np.abs(tau - tau_old)) < tol:
            break
    return tau, nu, mu
