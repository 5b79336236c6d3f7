"""numpy restatement of the covariance kinds and the per-theta reference
pipelines built on them, shared by the host and the GPU tests. A plain module: one description of
a kind, ``Cov(family, kind, bias, linear)``, as the library has one in ``kernel_kind_of``.

The base kind (family 'se' | '32' | '52', kind 'iso' | 'ard') has theta-length P0 (2 for iso,
d + 1 for ARD): s = exp(theta_0), tau_k = exp(theta_{k+1}) (ARD) or exp(theta_1) for every k (iso)
and r^2 = sum_k ((x_ik - x_jk)/tau_k)^2, summed over k in a plain loop in order,

    family 'se':  S = s exp(-r^2 / 2)                             G = S
    family '32':  S = s (1 + sqrt3 r) exp(-sqrt3 r)               G = 3 s exp(-sqrt3 r)
    family '52':  S = s (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)     G = 5/3 s (1 + sqrt5 r) exp(-sqrt5 r)

A constant term appends log beta to theta, a linear term (SE only, after the constant one where
both are present) log lambda; theta[:P0] keep their meaning. The dot products are on the raw
inputs:

    K_ij  = S_ij [+ beta] [+ lambda x_i . x_j]          data pairs
    K_ii  = (s [+ beta]) [+ lambda |x_i|^2] + epsilon   one point set's Gram only
    k*_ij = S*_ij [+ beta] [+ lambda x*_i . x_j]        the cross-Gram, no epsilon (also where two
                                                        points coincide)
    k**_i = s [+ beta] [+ lambda |x*_i|^2]              the prior variance, per test row
    dK/dtheta_0     = S (s on the diagonal: the jitter does not depend on theta)
    dK/dtheta_{k+1} = G_ij ((x_ik - x_jk)/tau_k)^2      (ARD; iso: the sum over k), zero diagonal
    dK/dlog beta    = beta                              every data pair, the diagonal included
    dK/dlog lambda  = lambda x_i . x_j                  every data pair, the diagonal included

The oracle's C Gram knows the SE family only. The SE kind without a term is that Gram called with
epsilon, and its S is K - epsilon I; the SE kinds with a term take the C Gram at epsilon = 0 and
set the diagonal; Matern is computed here from r^2. Each keeps its own expression: the three do
not agree to the bit ((s + epsilon) - epsilon is not s).
"""
import math

import numpy as np

import apm_oracle as orc
import ep_grad_restatement as eg
import ep_restatement as ep
import grad_restatement as gr
import predict_restatement as pr

FAMILIES = ('se', '32', '52')
MATERN = ('32', '52')
FAMILY_KINDS = [(f, k) for f in FAMILIES for k in ('iso', 'ard')]
LINEAR_KINDS = [('iso', False), ('ard', False), ('iso', True), ('ard', True)]  # (kind, bias)
SQRT3, SQRT5 = math.sqrt(3.0), math.sqrt(5.0)
COV_BIAS, COV_LINEAR = 16, 64
_BASE = {('se', 'iso'): 0, ('se', 'ard'): 1, ('32', 'iso'): 3, ('32', 'ard'): 4, ('52', 'iso'): 5,
         ('52', 'ard'): 6}
WRONG = ('eps_in_dk0', 'plus_beta')


def _tau(kind, theta, d):
    return np.exp(theta[1:d + 1]) if kind == 'ard' else np.full(d, math.exp(theta[1]))


def r2(kind, A, B, theta):
    """(len(A), len(B)) scaled squared distances, the sum over k in order."""
    tau = _tau(kind, theta, A.shape[1])
    out = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        out += ((A[:, None, k] - B[None, :, k]) / tau[k]) ** 2
    return out


def cov_S(family, sigma, q):
    """The covariance function of the scaled squared distance q = r^2."""
    if family == 'se':
        return sigma * np.exp(-0.5 * q)
    r = np.sqrt(q)
    if family == '32':
        return sigma * ((1.0 + SQRT3 * r) * np.exp(-SQRT3 * r))
    if family == '52':
        return sigma * ((1.0 + SQRT5 * r + (5.0 / 3.0) * q) * np.exp(-SQRT5 * r))
    raise ValueError('family must be one of {0}'.format(FAMILIES))


def cov_G(family, sigma, q):
    """The weight of the Matern length-scale derivatives."""
    r = np.sqrt(q)
    if family == '32':
        return 3.0 * sigma * np.exp(-SQRT3 * r)
    if family == '52':
        return (5.0 / 3.0) * sigma * ((1.0 + SQRT5 * r) * np.exp(-SQRT5 * r))
    raise ValueError('family must be one of {0}'.format(MATERN))


def _se_bound(Sref):
    """test_gpu_kernels' rule relative to the exponent: 2e-15 max(1, |log S|) |S|."""
    return 2e-15 * np.maximum(1.0, np.abs(np.log(np.maximum(Sref, 1e-300)))) * np.abs(Sref)


def _matern_bound(kind, A, B, theta, Kref):
    """Per-entry bound on |K - Kref| for a device Gram in the direct form on pre-scaled
    coordinates a_k = x_ik / tau_k, c_k = x_jk / tau_k, with u = 2^-53:

        delta(r^2) = 4 u sum_k (|a_k| + |c_k|) |a_k - c_k| + (D + 2) u r^2
        |K - Kref| <= |Kref| (8 u + 2 delta(r^2))

    (|d log S / d r^2| <= 3/2 for both families.)"""
    u = 2.0 ** -53
    D = A.shape[1]
    tau = _tau(kind, theta, D)
    s1 = np.zeros((A.shape[0], B.shape[0]))
    q = np.zeros_like(s1)
    for k in range(D):
        a, c = A[:, None, k] / tau[k], B[None, :, k] / tau[k]
        s1 += (np.abs(a) + np.abs(c)) * np.abs(a - c)
        q += (a - c) ** 2
    delta = 4.0 * u * s1 + (D + 2) * u * q
    return np.abs(Kref) * (8.0 * u + 2.0 * delta)


class Cov(object):
    """One covariance kind: the base family and iso / ARD, with or without the constant and the
    linear term."""

    def __init__(self, family, kind, bias=False, linear=False):
        if (family, kind) not in _BASE:
            raise ValueError('family must be one of {0}, kind iso or ard'.format(FAMILIES))
        if linear and family != 'se':
            raise ValueError('the linear term goes with the SE kinds only')
        self.family, self.kind, self.bias, self.linear = family, kind, bool(bias), bool(linear)
        self.flagged = self.bias or self.linear
        # the C-ABI's value: APM_KERNEL_* [| APM_COV_BIAS] [| APM_COV_LINEAR]
        self.native_kind = (_BASE[family, kind] | (COV_BIAS if bias else 0)
                            | (COV_LINEAR if linear else 0))
        # the name gpdemo.kernels.make_kernel_func and the batched samplers know the base kind by
        self.name = kind if family == 'se' else 'matern{0}_{1}'.format(family, kind)

    def __repr__(self):
        return 'Cov({0.family!r}, {0.kind!r}, bias={0.bias}, linear={0.linear})'.format(self)

    def n_base(self, d):
        return d + 1 if self.kind == 'ard' else 2

    def theta_len(self, d):
        return self.n_base(d) + self.bias + self.linear

    def split(self, theta, d):
        """(the base kind's theta, beta, lambda), 0.0 for an absent term; a theta shorter than
        theta_len(d) is an IndexError."""
        theta = np.asarray(theta, dtype=np.float64)
        p0 = self.n_base(d)
        if theta.shape[0] < self.theta_len(d):
            raise IndexError('theta too short')
        beta = math.exp(theta[p0]) if self.bias else 0.0
        lam = math.exp(theta[p0 + self.bias]) if self.linear else 0.0
        return theta[:p0], beta, lam

    def _oracle_gram(self, X, theta, eps):
        K = np.empty((X.shape[0], X.shape[0]))
        orc.c_gram(self.kind, K, X, np.asarray(theta, dtype=np.float64), eps)
        return K

    def base_S(self, X, th0):
        """S of the base kind on one point set: no epsilon, s = exp(theta_0) on the diagonal."""
        if self.family == 'se':
            S = self._oracle_gram(X, th0, 0.0)
        else:
            S = cov_S(self.family, math.exp(th0[0]), r2(self.kind, X, X, th0))
        S[np.diag_indices_from(S)] = math.exp(th0[0])
        return S

    def base_cross(self, Xs, X, th0):
        return cov_S(self.family, math.exp(th0[0]), r2(self.kind, Xs, X, th0))

    def gram(self, X, theta, eps):
        """K on one point set, epsilon on its diagonal."""
        if self.family == 'se' and not self.flagged:
            return self._oracle_gram(X, theta, eps)
        th0, beta, lam = self.split(theta, X.shape[1])
        K = self.base_S(X, th0) + beta
        diag = math.exp(th0[0]) + beta
        if self.linear:
            G = X.dot(X.T)
            K = K + lam * G
            diag = diag + lam * G.diagonal()
        K[np.diag_indices_from(K)] = diag + eps
        return K

    def gram_cross(self, Xs, X, theta):
        """(m, n) cross-covariance k*, no epsilon."""
        th0, beta, lam = self.split(theta, X.shape[1])
        Ks = self.base_cross(Xs, X, th0) + beta
        return Ks + lam * Xs.dot(X.T) if self.linear else Ks

    def prior_var(self, Xs, theta):
        """k**: a scalar, or with the linear term one value per test row (m,)."""
        th0, beta, lam = self.split(theta, Xs.shape[1])
        kss = math.exp(th0[0]) + beta
        return kss + lam * (Xs * Xs).sum(axis=1) if self.linear else kss

    def dK(self, X, theta, eps, wrong=None, K=None):
        """The P dense matrices dK/dtheta_j (epsilon is part of none of them). ``wrong`` selects
        one of the two wrong readings that the tests must tell apart: 'eps_in_dk0' keeps epsilon
        on the diagonal of dK/dtheta_0, 'plus_beta' takes theta_0's weight from K's own entries,
        S + beta. ``K``: the SE kind without a term forms S from this Gram and not from its own."""
        assert wrong is None or wrong in WRONG
        n, d = X.shape
        th0, beta, lam = self.split(theta, d)
        plain_se = self.family == 'se' and not self.flagged
        if self.family == 'se':
            if plain_se:
                K = self.gram(X, theta, eps) if K is None else K
                S = K - eps * np.eye(n)
            else:
                S = self.base_S(X, th0)
            G = S
            tau = np.exp(th0[1:])
            sq = [((X[:, None, k] - X[None, :, k]) / tau[k if self.kind == 'ard' else 0]) ** 2
                  for k in range(d)]
        else:
            sigma = math.exp(th0[0])
            q = r2(self.kind, X, X, th0)
            S = cov_S(self.family, sigma, q)
            S[np.diag_indices_from(S)] = sigma
            G = cov_G(self.family, sigma, q)
            tau = _tau(self.kind, th0, d)
            sq = [((X[:, None, k] - X[None, :, k]) / tau[k]) ** 2 for k in range(d)]
        if wrong == 'eps_in_dk0':
            out = [K.copy() if plain_se else S + eps * np.eye(n)]
        else:
            out = [S + beta if wrong == 'plus_beta' else S]
        if self.kind == 'ard':
            out.extend(G * s for s in sq)
        else:
            out.append(G * sum(sq))
        if self.bias:
            out.append(np.full((n, n), beta))
        if self.linear:
            out.append(lam * X.dot(X.T))
        return out

    def gram_bound(self, A, B, theta, Kref):
        """Per-entry bound on |K - Kref| of a device Gram or cross-Gram (u = 2^-53): the base
        kind's bound on S - for SE the rule relative to the exponent, for Matern the bound derived
        from the arithmetic - plus, with a term, 3 u |Kref| for the exp of its log-parameter, the
        sum and the epsilon, plus for the linear term (d + 2) u lambda sum_k |a_ik b_jk|, the
        forward bound of the chain of d fmas with the product's and lambda's roundings."""
        u = 2.0 ** -53
        d = A.shape[1]
        th0, beta, lam = self.split(theta, d)
        Sref = self.base_cross(A, B, th0) if self.flagged else Kref
        if self.family == 'se':
            bound = _se_bound(Sref)
        else:
            bound = _matern_bound(self.kind, A, B, th0, Sref)
        if self.flagged:
            bound = bound + 3.0 * u * np.abs(Kref)
        if self.linear:
            bound = bound + (d + 2) * u * lam * np.abs(A).dot(np.abs(B).T)
        return bound

    def kernel_func(self, eps):
        """``kernel_func(K, X, theta)`` for the oracle's is_estimate / priormc_estimate /
        laplace_estimate."""
        def fn(K, X, theta):
            K[...] = self.gram(X, theta, eps)
        return fn


# The per-theta pipelines: K, k*, k** and dK of the kind, handed to the shared Newton loop, EP fit
# and contractions.

def lml(cov, X, y, theta, eps, tol=1e-24):
    return gr.newton(cov.gram(X, theta, eps), y, tol)['lml']


def laplace_grad(cov, X, y, theta, eps, tol=1e-14, max_iters=1000, wrong=None):
    """dict(lml, grad (P,), n_iter, diffs, f) at theta."""
    K = cov.gram(X, theta, eps)
    return gr.laplace_grad(K, cov.dK(X, theta, eps, wrong, K=K), y, tol, max_iters)


def predictive(cov, X, y, Xs, theta, eps, tol=1e-4):
    return pr.predictive(cov.gram(X, theta, eps), cov.gram_cross(Xs, X, theta), y,
                         cov.prior_var(Xs, theta), tol=tol)


def ep_logz(cov, X, y, theta, eps, **ep_settings):
    return ep.ep_fit(cov.gram(X, theta, eps), y, **ep_settings)['logz']


def ep_grad(cov, X, y, theta, eps, wrong=None, K=None, **ep_settings):
    """dict(logz, grad (P,), n_sweeps, m_hist, fit) at theta; ep_settings are ep_fit's (damping,
    diff_tol, max_sweeps). K: the Gram to fit on instead of building it from theta (it must be
    theta's: the iso / ARD identity puts both sides on one set of bits)."""
    if K is None:
        K = cov.gram(X, theta, eps)
    return eg.ep_grad(K, cov.dK(X, theta, eps, wrong, K=K), y, **ep_settings)


def ep_predictive(cov, X, y, Xs, theta, eps, **ep_settings):
    fit = ep.ep_fit(cov.gram(X, theta, eps), y, **ep_settings)
    out = ep.at_test_inputs(cov.gram_cross(Xs, X, theta), cov.prior_var(Xs, theta), fit)
    out['n_sweeps'] = fit['n_sweeps']
    return out


def symmetric_ulp_noise(K, seed):
    """K with 1-ulp symmetric relative noise: K_ij (1 + 2^-52 e_ij), e symmetric in {-1, 0, 1}."""
    rng = np.random.RandomState(seed)
    e = np.tril(rng.randint(-1, 2, size=K.shape).astype(np.float64))
    e = e + np.tril(e, -1).T
    return K * (1.0 + 2.0 ** -52 * e)
