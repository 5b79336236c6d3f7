# -*- coding: utf-8 -*-
"""GP probit-classification pieces of the APM hot path, backed by libapm.so (HIP, gfx950).

Module layout mirrors the reference's ``gpdemo`` package: ``kernels`` (Gram builders),
``latent_posterior_approximations`` (Laplace), ``estimators`` (log-marginal-likelihood
estimators), ``utils`` (priors, adaptation schedule, I/O); ``predict`` (the Laplace predictive
distribution at held-out inputs), ``gradients`` (the gradient of the Laplace log marginal
likelihood with respect to theta) and ``loo`` (leave-one-out predictive densities from the
importance samples) have no reference counterpart."""
from .gradients import LaplaceGradient  # noqa: E402,F401
