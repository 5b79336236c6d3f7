"""Host side of the Laplace predictive path (gpdemo/predict.py): the module imports without a
device, refuses a kernel it cannot build on the device, and its array math (posterior average,
test log predictive density) matches a direct numpy evaluation, tails included."""
import math

import numpy as np
import pytest
from scipy.special import ndtr


def test_imports_without_a_device_and_rejects_foreign_kernels():
    import gpdemo.predict as prd
    X = np.zeros((4, 2))
    with pytest.raises(NotImplementedError):
        prd.LaplacePredictor(X, np.ones(4), lambda K, X, theta: None, np.zeros((3, 2)))


def test_posterior_average_is_the_mean_over_kept_samples():
    import gpdemo.predict as prd
    rng = np.random.RandomState(0)
    prob = rng.uniform(size=(11, 5))
    assert np.array_equal(prd.posterior_average(prob), prob.mean(0))
    assert np.array_equal(prd.posterior_average(prob, burn=3, thin=2), prob[3::2].mean(0))
    with pytest.raises(ValueError):
        prd.posterior_average(prob, burn=11)


def test_log_predictive_density_vs_direct_numpy():
    import gpdemo.predict as prd
    rng = np.random.RandomState(1)
    T, M = 7, 9
    mean = rng.normal(scale=2.0, size=(T, M))
    var = rng.uniform(0.01, 3.0, size=(T, M))
    y = np.where(rng.normal(size=M) > 0, 1.0, -1.0)
    z = mean / np.sqrt(1.0 + var)
    direct = np.mean(np.log(np.mean(ndtr(y[None] * z), axis=0)))  # moderate z: no tail trouble
    got = prd.log_predictive_density(mean, var, y)
    assert abs(got - direct) <= 1e-13 * max(1.0, abs(direct))
    d2 = np.mean(np.log(np.mean(ndtr(y[None] * z[2::3]), axis=0)))
    assert abs(prd.log_predictive_density(mean, var, y, burn=2, thin=3) - d2) <= 1e-13 * abs(d2)
    with pytest.raises(ValueError):
        prd.log_predictive_density(mean, var, y[:-1])


def test_log_predictive_density_tails():
    """z = -40 for a positive label: Phi underflows (the naive log gives -inf); z = +40: Phi
    rounds to 1 and the naive log to 0. Both keep their leading asymptotic term."""
    import gpdemo.predict as prd
    var = np.full((2, 2), 3.0)
    mean = np.array([[-80.0, 80.0], [-80.0, 80.0]])  # z = -+40 in both samples
    y = np.array([1.0, 1.0])
    with np.errstate(divide='ignore'):
        assert np.log(ndtr(-40.0)) == -np.inf
    got = prd.log_predictive_density(mean, var, y)
    # log Phi(-z) ~ -z^2/2 - log(z sqrt(2 pi)) + log(1 - 1/z^2 + 3/z^4), z = 40
    lo = -800.0 - math.log(40.0 * math.sqrt(2.0 * math.pi)) + math.log1p(-1 / 1600. + 3 / 2.56e6)
    hi = -math.exp(lo)  # log Phi(40) = log1p(-Phi(-40))
    assert math.isfinite(got)
    assert abs(got - 0.5 * (lo + hi)) <= 1e-8 * abs(lo)
    # samples that disagree wildly: the log-mean-exp keeps the dominant sample
    mean2 = np.array([[-80.0], [0.0]])
    got2 = prd.log_predictive_density(mean2, np.full((2, 1), 3.0), np.array([1.0]))
    assert abs(got2 - math.log(0.25)) <= 1e-14
