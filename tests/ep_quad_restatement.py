"""numpy statement of EP with the tilted moments by quadrature (k_ep_sites_q,
apm_set_ep_quadrature, apm_ep_lik), shared by test_ep_quad_host.py and test_gpu_ep_quad.py. A
plain module. The rule reads its tables and constants from the generated header the kernel
includes (csrc/ep_quad.h), so the two share every number; the sweep is ep_restatement's with the
moments exchanged and log Z^ in the place of log Phi(z)."""
import os
import re

import numpy as np
from scipy.special import log_expit, log_ndtr

import ep_restatement as ep

PROBIT, LOGIT = 0, 1
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'auxiliary-pm-mcmc_amd',
                      'csrc', 'ep_quad.h')


def _read_header():
    txt = open(HEADER).read()
    out = {}
    for m in re.finditer(r'#define\s+(APM_EPQ_\w+)\s+(\S+)', txt):
        out[m.group(1)] = float(m.group(2))
    for m in re.finditer(r'double\s+(APM_EPQ_\w+)\[\w+\]\s*=\s*\{([^}]*)\}', txt):
        out[m.group(1)] = np.array([float(t) for t in m.group(2).replace('\n', ' ').split(',')
                                    if t.strip()])
    return out


T = _read_header()
V0 = T['APM_EPQ_V0']
assert len(T['APM_EPQ_GH_X']) == T['APM_EPQ_GH_N'] == 128
assert len(T['APM_EPQ_GL_XI']) == T['APM_EPQ_GL_N'] == 8 and T['APM_EPQ_PANELS'] == 16


def log_lik(lik, t):
    return log_expit(t) if lik == LOGIT else log_ndtr(t)


def _narrow(lik, m, s):
    """Gauss-Hermite on the cavity: the three sums with the largest exponent taken out."""
    d = np.sqrt(2.0) * s[:, None] * T['APM_EPQ_GH_X'][None, :]
    e = log_lik(lik, m[:, None] + d) + T['APM_EPQ_GH_LW'][None, :]
    E = e.max(1)
    a = np.exp(e - E[:, None])
    s0 = a.sum(1)
    return E + np.log(s0), (a * d).sum(1) / s0, (a * d * d).sum(1) / s0


def narrow_covered(lik, m, s):
    """The logit everywhere; the probit while the integrand's peak in the rule's variable,
    x* = -m s / (sqrt2 (1 + s^2)), is below X_MAX."""
    if lik == LOGIT:
        return np.ones(m.shape, dtype=bool)
    return -m * s <= T['APM_EPQ_X_MAX'] * np.sqrt(2.0) * (1.0 + s * s)


def wide_range(lik, m, s):
    """T_in, T of the correction integral and whether the site is in the covered region. The
    logit's part at t = -u is N(u | c, s^2) / (1 + e^-u) up to a constant, c = -m - s^2: T is
    where that Gaussian is e^(-TAIL^2 / 2) below its peak (c > 0) or below its value at 0."""
    t_in = T['APM_EPQ_T_IN_LOGIT'] if lik == LOGIT else T['APM_EPQ_T_IN_PROBIT']
    if lik == LOGIT:
        c = -m - s * s
        ts = T['APM_EPQ_TAIL'] * s
        t_end = np.maximum(2.0 * t_in, c + np.where(c > 0.0, ts, np.sqrt(c * c + ts * ts)))
        ok = ((t_end - t_in) <= 8.0 * T['APM_EPQ_H_MAX'] * s) & (
            (c >= 0.0) | (m >= -T['APM_EPQ_A_MAX'] * s))
    else:
        t_end = np.full_like(m, 2.0 * t_in)
        ok = -m <= np.minimum(T['APM_EPQ_PEAK_MAX'] * (1.0 + s * s), T['APM_EPQ_M_MAX'])
    return t_in, t_end, ok


def _wide(lik, m, s):
    """p = H + r: the step's closed-form moments about m plus composite Gauss-Legendre of the
    correction on [0, T_in] and [T_in, T], eight panels each, scaled by the largest exponent."""
    t_in, t_end, _ = wide_range(lik, m, s)
    xi, lw = T['APM_EPQ_GL_XI'], T['APM_EPQ_GL_LW']
    p = np.arange(8)
    frac = (p[:, None] + xi[None, :]).reshape(-1) / 8.0   # 64 nodes of 8 panels on a unit range
    lwn = np.tile(lw, 8) - np.log(8.0)
    u = np.concatenate([t_in * frac[None, :] * np.ones_like(m)[:, None],
                        t_in + (t_end - t_in)[:, None] * frac[None, :]], 1)
    lW = np.concatenate([np.log(t_in) + lwn[None, :] * np.ones_like(m)[:, None],
                         np.log(t_end - t_in)[:, None] + lwn[None, :]], 1)
    M, S = m[:, None], s[:, None]
    alpha = m / s
    base = log_lik(lik, -u) + lW - np.log(S) - HALF_LOG_2PI
    lm = base - (u + M) ** 2 / (2.0 * S * S)   # the node at t = -u
    lp = base - (u - M) ** 2 / (2.0 * S * S)   # the node at t = +u
    lP = log_ndtr(alpha)
    E = np.maximum(lP, np.maximum(lm.max(1), lp.max(1)))
    am, ap = np.exp(lm - E[:, None]), np.exp(lp - E[:, None])
    dm, dp = -(u + M), u - M
    s0 = (am - ap).sum(1)
    s1 = (dm * am - dp * ap).sum(1)
    s2 = (dm * dm * am - dp * dp * ap).sum(1)
    P = np.exp(lP - E)
    ph = np.exp(-0.5 * alpha * alpha - HALF_LOG_2PI - E)
    z = P + s0
    return E + np.log(z), (s * ph + s1) / z, (s * s * (P - alpha * ph) + s2) / z


def tilted_quad(lik, y, mu_c, var_c):
    """log Z^, the tilted mean and variance of p(y f) N(f | mu_c, var_c) by the rule, and the
    mask of sites inside the covered region. Arrays of one length."""
    y, mu_c, var_c = (np.atleast_1d(np.asarray(v, dtype=float)) for v in (y, mu_c, var_c))
    m, s = y * mu_c, np.sqrt(var_c)
    lz, e1, e2 = np.empty_like(m), np.empty_like(m), np.empty_like(m)
    covered = np.ones(m.shape, dtype=bool)
    nar = var_c <= V0
    if nar.any():
        lz[nar], e1[nar], e2[nar] = _narrow(lik, m[nar], s[nar])
        covered[nar] = narrow_covered(lik, m[nar], s[nar])
    if (~nar).any():
        lz[~nar], e1[~nar], e2[~nar] = _wide(lik, m[~nar], s[~nar])
        covered[~nar] = wide_range(lik, m[~nar], s[~nar])[2]
    return lz, mu_c + y * e1, e2 - e1 * e1, covered


def ep_fit(K, y, lik=LOGIT, damping=0.8, diff_tol=1e-8, max_sweeps=100):
    """ep_restatement.ep_fit with the moments by quadrature. Adds to its result: covered (every
    site of every sweep was inside the rule's region), n_narrow / n_wide of the last sweep, and
    the cavity of the last sweep (mu_c, var_c)."""
    n = y.shape[0]
    tau, nu = np.zeros(n), np.zeros(n)
    mu_prev, m_hist, covered = None, [], True
    for t in range(1, int(max_sweeps) + 1):
        s, L, a, mu, var = ep.posterior(K, tau, nu)
        with np.errstate(divide='ignore', invalid='ignore'):
            tau_c = 1.0 / var - tau
            nu_c = mu / var - nu
        if not np.all(np.isfinite(tau_c) & (tau_c > 0.0)):
            raise ep.InvalidCavity('sweep {0}'.format(t))
        mu_c, var_c = nu_c / tau_c, 1.0 / tau_c
        lz, mu_h, var_h, cov = tilted_quad(lik, y, mu_c, var_c)
        covered = covered and bool(cov.all())
        if t >= 2:
            m = np.mean((mu - mu_prev) ** 2)
            m_hist.append(m)
            if m < diff_tol:
                rows = (lz + 0.5 * np.log1p(tau / tau_c) + 0.5 * nu * mu - 0.5 * nu * nu * var
                        + 0.5 * mu_c * tau_c * (tau * mu_c - 2.0 * nu) * var)
                logz = rows.sum() - np.log(np.diag(L)).sum()
                return dict(logz=logz, mu=mu, var=var, tau=tau, nu=nu, a=a, L=L, s=s,
                            n_sweeps=t, m_hist=m_hist, covered=covered, mu_c=mu_c, var_c=var_c,
                            n_narrow=int((var_c <= V0).sum()), n_wide=int((var_c > V0).sum()))
        tau_new = np.maximum(1.0 / var_h - tau_c, 0.0)
        nu_new = mu_h / var_h - nu_c
        tau = (1.0 - damping) * tau + damping * tau_new
        nu = (1.0 - damping) * nu + damping * nu_new
        mu_prev = mu
    raise ep.NotConverged('{0} sweeps'.format(max_sweeps))


def ep_sequential(K, y, lik=LOGIT, n_sweeps=200, tol=1e-13):
    """ep_restatement.ep_sequential (R&W Alg. 3.5) with the moments by quadrature."""
    import scipy.linalg as la
    n = y.shape[0]
    tau, nu = np.zeros(n), np.zeros(n)
    Sigma, mu = K.copy(), np.zeros(n)
    for _ in range(n_sweeps):
        tau_old = tau.copy()
        for i in range(n):
            tau_c = 1.0 / Sigma[i, i] - tau[i]
            nu_c = mu[i] / Sigma[i, i] - nu[i]
            _, mu_h, var_h, _ = tilted_quad(lik, y[i], nu_c / tau_c, 1.0 / tau_c)
            dtau = 1.0 / var_h[0] - tau_c - tau[i]
            tau[i] += dtau
            nu[i] = mu_h[0] / var_h[0] - nu_c
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


def at_test_inputs(Ks, sigma, fit, lik=LOGIT):
    """ep_restatement.at_test_inputs; the logit's prob is the average of sigma at N(mean, var)
    by the 400-node Gauss-Hermite rule."""
    out = ep.at_test_inputs(Ks, sigma, fit)
    if lik == LOGIT:
        from scipy.special import expit, roots_hermite
        x, w = roots_hermite(400)
        f = out['mean'][:, None] + np.sqrt(2.0 * np.maximum(out['var'], 0.0))[:, None] * x
        out['prob'] = (expit(f) * w).sum(1) / np.sqrt(np.pi)
    return out


def exact_moments(lik, y, mu_c, var_c, dps=40):
    """log Z^, mean and variance of p(y f) N(f | mu_c, var_c) by mpmath.quad at `dps` digits."""
    import mpmath as mp
    mp.mp.dps = dps
    m, s = mp.mpf(y) * mp.mpf(mu_c), mp.sqrt(mp.mpf(var_c))

    def lik_f(t):
        if lik == LOGIT:
            return 1 / (1 + mp.exp(-t))
        return mp.erfc(-t / mp.sqrt(2)) / 2

    def g(k):
        return lambda t: lik_f(t) * (t - m) ** k * mp.exp(-(t - m) ** 2 / (2 * s * s))
    # The integrand is below N(t | m, s^2), and its mass lies between m and the point the
    # likelihood tilts it up to where t < 0 (the logit's e^t: m + s^2, the probit's Gaussian tail:
    # m / (1 + s^2)), never past 0: 14 deviations either side of that leave out less than e^-98
    # of it. Pieces of half a deviation, and of one unit on [-45, 45] where the likelihood itself
    # varies; Gauss-Legendre per piece (tanh-sinh over long pieces of a narrow Gaussian was found
    # to return 1e-7 errors while reporting none).
    lo = m - 14 * s
    up = m + s * s if lik == LOGIT else m / (1 + s * s)
    hi = max(m, min(up, mp.mpf(0))) + 14 * s
    pts = [lo + s * k / 2 for k in range(int(mp.ceil(2 * (hi - lo) / s)))] + [hi]
    pts += [mp.mpf(k) for k in range(-45, 46) if lo < k < hi]
    pts = sorted(set(pts))
    z, d1, d2 = (mp.quad(g(k), pts, method='gauss-legendre') for k in range(3))
    e1, e2 = d1 / z, d2 / z
    return (float(mp.log(z / (s * mp.sqrt(2 * mp.pi)))), float(mp.mpf(mu_c) + mp.mpf(y) * e1),
            float(e2 - e1 * e1))
